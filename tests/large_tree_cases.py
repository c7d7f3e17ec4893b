"""Trees beyond 64 leaves for the null and its simulators, a plain helper module shared by tests/test_large_tree_cases.py
(CPU: the oracle-only preconditions), tests/test_gpu_large_tree_simulators.py and tests/test_gpu_large_tree_null.py.

Each tree is the smallest instance of something that only a larger tree reaches (B = branches, nn = B + 1 nodes):

    u65       synthetic.random_tree(65)        B 127   the last B on the register arm of null_pattern_moments_kernel
    r65       model_sets.rooted_random_tree    B 128   exactly kMomentRows (a rooted tree: a binary root)
    u66       synthetic.random_tree(66)        B 129   the first B on the fallback arm (pattern_moments); T = 66: five
                                                       16-taxon pieces of a packed column, the last one holding 2 taxa
    u131      synthetic.random_tree(131)       B 259   more than 256 nodes; T = 131: nine pieces, the last holding 3 taxa
    bal128    tree_shapes._balanced(128)       B 254   T a multiple of 16; 64 cherries, the message table on
                                                       (64 x 4 x 76 800 B = 18.75 MiB, under the 32 MiB limit)
    cat130    tree_shapes._caterpillar(130)    B 258   129 levels, a node whose parent was just drawn on every level, one cherry
    multi140  _random_multifurcating(140)      B 196   2 to 5 children everywhere, at size
    myo       tests/golden/myoglobin.npz       B 197   the reference's own example tree with its own model (the table its
                                                       build held, Gamma(4) at the fitted alpha)

Models: p4 = synthetic.protein_model(0.5, 4) on every tree; p1 (one class), p6 (six classes: the simulator's other launch
shapes) and k2 (two substitution types from a signed register, as test_gpu_cherry_msg._engines builds them) on chosen
trees; d4 / d5 / d6 / d2 = synthetic.dna_model(0.7, ncat): 16 and 20 class-fused device states, six classes as two passes
of 20 fused states (the second one padded), and with two classes the unfused 4 states.

Null inputs: every case has (nrep, ram) = (3, 53) -- an odd ram: the byte stores of the chain simulator and
null_pattern_key_kernel -- and (2, 48) -- a multiple of 4: null_pattern_key4_kernel --, drawn by the null itself, and one
supplied alignment with forced repeats (`with_patterns`: 171 distinct columns over 3 x 2 x 37 sites, two full tiles and a
partial one), because on trees this large nearly every simulated column is distinct.

The reference of a null is composed here from the oracle's pieces -- oracle.simulate, oracle.map_sites once per alignment,
oracle.stat_pair per pair and kind, the minima -- so that four statistics share one mapping; test_large_tree_cases.py
proves the composition equal to oracle.null_intra byte for byte."""
import os
from collections import OrderedDict
from functools import lru_cache

import numpy as np

import oracle
from comap_amd import protein_models as pm, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> (B, nn, T) as the table above states them
SIZES = {"u65": (127, 128, 65), "r65": (128, 129, 65), "u66": (129, 130, 66), "u131": (259, 260, 131),
         "bal128": (254, 255, 128), "cat130": (258, 259, 130), "multi140": (196, 197, 140), "myo": (197, 198, 100)}
TREE_SEED = {"u65": 6501, "r65": 6502, "u66": 6601, "u131": 13101, "bal128": 12801, "cat130": 13001, "multi140": 14001}
PROTEIN_TREES = list(SIZES)
MOMENT_TREES = ["u65", "r65", "u66"]                    # B = 127, 128 | 129: both sides of kMomentRows = 128
PROTEIN_CASES = [f"{t}-p4" for t in PROTEIN_TREES]
OTHER_PROTEIN_CASES = ["u66-p1", "u66-k2"]
DNA_CASES = [f"{t}-d{n}" for t in ("u131", "bal128") for n in (4, 5, 6)] + ["u131-d2", "bal128-d2"]
NULL_CASES = PROTEIN_CASES + OTHER_PROTEIN_CASES + DNA_CASES
SIM_CASES = [f"{t}-p4" for t in ("u66", "u131", "bal128", "cat130", "multi140", "myo")] + ["u131-p6"]
UNFUSED_CASE = "u131-p4"                                # the unfused, inter-gene and continuous-rate nulls
ALL_CASES = NULL_CASES + [c for c in SIM_CASES if c not in NULL_CASES]

NULL_INPUTS = {"3x53": (3, 53), "2x48": (2, 48)}        # drawn by the null itself: (nrep, ram)
FORCED = "forced"                                       # the supplied alignment with repeats
FORCED_SHAPE, FORCED_PATTERNS = (3, 37), 171
INPUTS = list(NULL_INPUTS) + [FORCED]
KINDS = (0, 4, 1, 3)                                    # Correlation, Covariance (the moments kernel), Compensation, Cosinus

# the simulators (tests/test_gpu_large_tree_simulators.py)
SIM_SEED, SIM_G0, SIM_N = 987654321, 12345, 700         # eng.simulate: an odd g0
CHAIN_SEED = 4711
H = 512                                                 # half a batch of the chain kernel: a thread draws a pair of sites
CHAIN_CALLS = [(0, 1, 1), (0, 1, H + 1), (1, 2, 4 * H + 2), (2, 4, 3 * H)]   # (rep_begin, rep_end, rep_ram)
# the unfused nulls of UNFUSED_CASE
MI_BOUNDS = np.array([0.0, 1e-4, 1e-3, 0.01, 0.05, 0.3, 1.0, 50.0])
UNFUSED = dict(seed=515, nrep=2, ram=33)
INTER = dict(seed=4242, rep_begin=1, rep_end=3, ram=35, blen_scale=1.3)
CONTINUOUS = dict(seed=5, rep_begin=2, rep_end=4, ram=33, alpha=0.5, p_inv=0.1)


def null_seed(case):
    return 7100 + ALL_CASES.index(case)


# ---------------------------------------------------------------------------------------------- trees and models
@lru_cache(maxsize=None)
def tree(name):
    """-> (parent, blen, leaf_of_taxon): post-order, root last, blen[root] = 0"""
    if name == "myo":
        myo = np.load(os.path.join(GOLDEN, "myoglobin.npz"))
        return (np.asarray(myo["parent"], dtype=np.int32), np.asarray(myo["blen"], dtype=np.float64),
                np.asarray(myo["leaf_of_taxon"], dtype=np.int32))
    seed = TREE_SEED[name]
    if name.startswith("u"):
        return synthetic.random_tree(int(name[1:]), seed)
    if name == "r65":
        from model_sets import rooted_random_tree
        return rooted_random_tree(65, seed)
    if name == "multi140":
        from test_traversal_program import _random_multifurcating
        return _random_multifurcating(140, seed)
    from tree_shapes import _balanced, _caterpillar
    rng = np.random.default_rng(seed)
    if name == "bal128":
        parent, lot = _balanced(128)
        blen = np.maximum(rng.exponential(0.1, size=len(parent)), 1e-6)
    else:
        parent, lot = _caterpillar(130)
        blen = rng.uniform(0.02, 0.3, size=len(parent))
    blen[-1] = 0.0
    return parent, blen, lot


def cherries(name):
    """the non-root nodes with exactly two children, both leaves"""
    from tree_shapes import Shape
    parent, _, lot = tree(name)
    return Shape(name, parent, lot).cherries()


@lru_cache(maxsize=None)
def model(case):
    """-> (Q, pi, rates, probs, Bk or None, clamp_negative)"""
    name, m = case.split("-")
    if name == "myo":
        myo = np.load(os.path.join(GOLDEN, "myoglobin.npz"))
        Q, pi = pm.jtt92_bpp2x()
        rates, probs = pm.gamma_rates(float(myo["alpha"]), 4)
        assert m == "p4" and int(myo["ncat"]) == 4
        return Q, pi, rates, probs, None, True
    if m[0] == "d":
        mdl = synthetic.dna_model(0.7, int(m[1:]))
        return mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], None, True
    mdl = synthetic.protein_model(0.5, 4 if m == "k2" else int(m[1:]))
    Bk, clamp = None, True
    if m == "k2":
        W1 = np.random.default_rng(4).uniform(-1, 1, size=mdl["Q"].shape)
        Bk = np.stack([synthetic.weighted_register(mdl["Q"], W1), synthetic.weighted_register(mdl["Q"], np.abs(W1))])
        clamp = False
    return mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk, clamp


def null_kinds(case):
    """the statistics a case's null is run with"""
    m = case.split("-")[1]
    if m == "k2":
        return (1,)
    if m == "p4":
        return KINDS
    return (0, 1)                                          # one pass from moments, and the generic pair_stat_strided


@lru_cache(maxsize=None)
def oracle_of(case, blen_scale=1.0):
    parent, blen, lot = tree(case.split("-")[0])
    Q, pi, rates, probs, Bk, clamp = model(case)
    return oracle.Model(parent, blen * blen_scale, lot, Q, pi, rates, probs, Bk=Bk, nonneg=clamp)


def new_engine(case, table=True, blen_scale=1.0):
    """an engine of the case, not cached (the scratch guard takes hold of contexts created after it is switched on);
    table: with the cherry message table of 20-state models (engine.cherry_msg)"""
    from comap_amd import engine
    parent, blen, lot = tree(case.split("-")[0])
    Q, pi, rates, probs, Bk, clamp = model(case)
    was = engine.cherry_msg()
    try:
        engine.cherry_msg(table)
        return engine.Engine(parent, blen * blen_scale, lot, Q, pi, rates, probs, Bk=Bk, clamp_negative=clamp)
    finally:
        engine.cherry_msg(was)


_engines = OrderedDict()       # case -> {(table, blen_scale): Engine}; the engines of the two cases used last stay open


def engine_of(case, table=True, blen_scale=1.0):
    """the case's engine, cached per case as test_gpu_simulator_chain._setup does; a tree of 260 nodes holds a workspace
    per wave, so only the two cases used last keep their engines"""
    mine = _engines.setdefault(case, {})
    _engines.move_to_end(case)
    while len(_engines) > 2:
        for eng in _engines.popitem(last=False)[1].values():
            eng.close()
    key = (bool(table), float(blen_scale))
    if key not in mine:
        mine[key] = new_engine(case, table, blen_scale)
    return mine[key]


# ---------------------------------------------------------------------------------------------- alignments
def with_patterns(T, S, npat, nrep, ram, seed):
    """[nrep][2][T][ram] alignments with exactly npat distinct columns: the first npat sites are the patterns in order, the
    others repeat patterns drawn at random (so duplicates point into every tile)"""
    rng = np.random.default_rng(seed)
    n = nrep * 2 * ram
    assert npat <= n
    cols = set()
    while len(cols) < npat:
        cols.add(bytes(rng.integers(0, S, size=T, dtype=np.uint8)))
    pats = np.frombuffer(b"".join(sorted(cols)), dtype=np.uint8).reshape(npat, T)
    pats = pats[rng.permutation(npat)]
    which = np.concatenate([np.arange(npat), rng.integers(0, npat, size=n - npat)])
    sites = pats[which]                                                   # [n][T], g = (rep * 2 + h) * ram + j
    return np.ascontiguousarray(sites.reshape(nrep, 2, ram, T).transpose(0, 1, 3, 2))


def columns(sup):
    """[nrep][2][T][ram] -> the columns of sites g = (rep * 2 + h) * ram + j, one row each"""
    return np.ascontiguousarray(sup.transpose(0, 1, 3, 2).reshape(-1, sup.shape[2]))


def distinct(sup):
    return len(np.unique(columns(sup), axis=0))


def shape_of(inp):
    return FORCED_SHAPE if inp == FORCED else NULL_INPUTS[inp]


def as_supplied(aln, nrep, ram):
    """[T][nrep * 2 * ram] columns g = (rep * 2 + h) * ram + j -> [nrep][2][T][ram]"""
    return np.ascontiguousarray(aln.reshape(aln.shape[0], nrep, 2, ram).transpose(1, 2, 0, 3))


@lru_cache(maxsize=None)
def alignments(case, inp):
    """the null's alignments [nrep][2][T][ram]: the oracle's draws of the ranges the null draws for itself, or the forced
    repeats (the columns of which are uniform random: no tree makes them impossible)"""
    om = oracle_of(case)
    nrep, ram = shape_of(inp)
    if inp == FORCED:
        return with_patterns(om.T, om.S, FORCED_PATTERNS, nrep, ram, 900 + ALL_CASES.index(case))
    return as_supplied(oracle.simulate(om, null_seed(case), 0, nrep * 2 * ram)[0], nrep, ram)


# ---------------------------------------------------------------------------------------------- references
def _minimum(a, b):
    return np.where(b < a, b, a)         # batch 0 first, then "<" (AnalysisTools.cpp:643-652)


def compose(om1, om2, sup):
    """map batch 0 of every replicate under om1 and batch 1 under om2 -> dict(counts = ([n, B, K], [n, B, K]), logL [2, n],
    nmin, prmin, rcmin), pair q = rep * ram + j"""
    nrep, _, _, ram = sup.shape
    side = []
    for h, om in enumerate((om1, om2)):
        aln = np.ascontiguousarray(sup[:, h].transpose(1, 0, 2).reshape(sup.shape[2], nrep * ram))
        side.append(oracle.map_sites(om, aln))
    a, b = side
    return dict(counts=(a["counts"], b["counts"]), logL=np.stack([a["logL"], b["logL"]]),
                nmin=_minimum(a["norm"], b["norm"]), prmin=_minimum(a["post_rate"], b["post_rate"]),
                rcmin=_minimum(a["rate_class"], b["rate_class"]).astype(np.int32))


def stat_of(ref, kind, params=None):
    a, b = ref["counts"]
    return np.array([oracle.stat_pair(kind, a[q], b[q], params) for q in range(len(a))])


@lru_cache(maxsize=None)
def mapped(case, inp):
    om = oracle_of(case)
    return compose(om, om, alignments(case, inp))


@lru_cache(maxsize=None)
def reference(case, inp, kind):
    """what oracle.null_intra gives for the case's input -> dict(stat, nmin, prmin, rcmin)"""
    ref = mapped(case, inp)
    return dict(stat=stat_of(ref, kind), nmin=ref["nmin"], prmin=ref["prmin"], rcmin=ref["rcmin"])


def mi_params(bounds=MI_BOUNDS):
    return np.concatenate([[float(len(bounds))], np.asarray(bounds, dtype=np.float64)])


def branch_weights(B):
    return np.random.default_rng(B).uniform(0.2, 2.0, size=B)


@lru_cache(maxsize=None)
def unfused_mapped():
    k = UNFUSED
    om = oracle_of(UNFUSED_CASE)
    return compose(om, om, as_supplied(oracle.simulate(om, k["seed"], 0, k["nrep"] * 2 * k["ram"])[0], k["nrep"], k["ram"]))


def continuous_alignments(want_near=False):
    k = CONTINUOUS
    nrep = k["rep_end"] - k["rep_begin"]
    out = oracle.simulate_continuous(oracle_of(UNFUSED_CASE), k["seed"], k["rep_begin"] * 2 * k["ram"], nrep * 2 * k["ram"],
                                     k["alpha"], k["p_inv"], want_near=want_near)
    sup = as_supplied(out[0], nrep, k["ram"])
    return (sup, out[2]) if want_near else sup


# ---------------------------------------------------------------------------------------------- simulator ranges
def discrete_ranges():
    """[(label, oracle model, seed, g0, n)]: every range of global site indices that a GPU test of these files has the
    discrete simulator draw and compares bit for bit"""
    out = []
    for case in SIM_CASES:
        om = oracle_of(case)
        out.append((f"simulate:{case}", om, SIM_SEED, SIM_G0, SIM_N))
        out += [(f"chain:{case}:{rb}-{re}x{ram}", om, CHAIN_SEED, rb * 2 * ram, (re - rb) * 2 * ram) for rb, re, ram in CHAIN_CALLS]
    for case in NULL_CASES:
        for inp, (nrep, ram) in NULL_INPUTS.items():
            out.append((f"null:{case}:{inp}", oracle_of(case), null_seed(case), 0, nrep * 2 * ram))
    k = UNFUSED
    out.append(("unfused", oracle_of(UNFUSED_CASE), k["seed"], 0, k["nrep"] * 2 * k["ram"]))
    k = INTER
    g0, n = k["rep_begin"] * 2 * k["ram"], (k["rep_end"] - k["rep_begin"]) * 2 * k["ram"]
    out.append(("inter1", oracle_of(UNFUSED_CASE), k["seed"], g0, n))
    out.append(("inter2", oracle_of(UNFUSED_CASE, k["blen_scale"]), k["seed"], g0, n))
    return out
