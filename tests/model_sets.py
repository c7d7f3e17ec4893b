"""Non-homogeneous model sets for the tests (a plain helper module): the shared cases of tests/test_gpu_model_sets.py,
their simulator inputs, and the builders of the engine and of the oracle's ModelSet from a case.

Every case has three reversible generators with their own frequencies, root frequencies that are none of them, the first
two children of the root on generators 0 and 1, and every generator on some branch.  The cases (states x classes -> the
device layout they reach):

    p20x4   protein matrix-core walk, pattern null by default     9 leaves, rooted, random
    p20x6   six classes: the largest two-piece node block         the same tree
    p20x9   nine classes: the largest protein model with tables   the same tree
    n4x4    class-fused nucleotide walk, cherry tables            the same tree
    n4x5    fuse 5                                                13 leaves, balanced (six cherries)
    n4x2    unfused nucleotide                                    6 leaves
    c61x2   plain kernels, continuous simulator above 20 states   6 leaves
    s7x2    plain kernels (mapping only)                          6 leaves
    c61x1, w64x1   simulator only: the widest models with tables  6 leaves
    s7x50          simulator only: no tables (like c61x2)         6 leaves
    p20x3:<shape>, n4x4:<shape>                                   the rooted 2-, 3- and 4-leaf shapes of SHAPES

The simulator inputs are listed here, not in the GPU tests, so that tests/test_oracle_model_sets.py can bound the share of
fragile sites of every one of them and prove that a simulator which ignored the set would not reproduce them."""
from functools import lru_cache

import numpy as np

import oracle
from comap_amd import protein_models as pm, synthetic
from tree_shapes import _balanced, by_name, rooted_catalogue

SHAPES = ["(x,x)", "((x,x),x)", "(x,x,x)", "((x,x),(x,x))", "((x,x),x,x)"]      # (x,x,x) and ((x,x),x,x): a multifurcating root
TABLE = ["p20x4", "n4x4", "n4x5", "n4x2", "c61x2"] + [f"{m}:{s}" for s in SHAPES for m in ("p20x3", "n4x4")]
MAPPING_CASES = TABLE[:5] + ["s7x2"] + TABLE[5:]
SIMULATOR_CASES = TABLE
CONTINUOUS_CASES = ["p20x4", "n4x4", "c61x2"]
NULL_CASES = ["p20x4", "n4x4"]
IUPAC = np.array([1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15, 15], dtype=np.uint32)   # A C G T R Y S W K M B D H V N -


def rooted_random_tree(ntaxa, seed, mean_blen=0.15):
    """random rooted binary tree (random joins of two subtrees) -> (parent, blen, leaf_of_taxon), post-order, root last"""
    rng = np.random.default_rng(seed)
    trees = [t for t in range(ntaxa)]                    # nested tuples, leaves are taxon numbers
    while len(trees) > 1:
        i, j = sorted(rng.choice(len(trees), size=2, replace=False))
        b = trees.pop(j)
        trees[i] = (trees[i], b)
    parent, lot = [], np.zeros(ntaxa, dtype=np.int32)

    def visit(u):
        kids = [visit(c) for c in u] if isinstance(u, tuple) else []
        me = len(parent)
        parent.append(-1)
        for c in kids:
            parent[c] = me
        if not kids:
            lot[u] = me
        return me
    visit(trees[0])
    blen = np.maximum(rng.exponential(mean_blen, size=len(parent)), 1e-3)
    blen[-1] = 0.0
    return np.array(parent, dtype=np.int32), blen, lot


def _generators(S, seed):
    """three reversible generators of mean rate 1, each with its own frequencies and its own exchangeabilities: those of
    the JTT / GTR base model at 20 and 4 states, random ones at any other size, times symmetric random factors
    -> (Qs [3, S, S], pis [3, S])"""
    rng = np.random.default_rng(seed)
    if S in (20, 4):
        base = synthetic.protein_model() if S == 20 else synthetic.dna_model()
        R = np.asarray(base["Q"]) / np.asarray(base["pi"])[None, :]
    else:
        R = rng.uniform(0.2, 2.0, size=(S, S))
    R = (R + R.T) / 2
    Qs, pis = [], []
    for _ in range(3):
        pi = rng.dirichlet(np.full(S, 8.0))
        F = rng.uniform(0.5, 1.5, size=(S, S))             # symmetric factors: the generator stays reversible
        Q = R * (F + F.T) / 2 * pi[None, :]
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
        Qs.append(Q / -(pi * np.diag(Q)).sum())
        pis.append(pi)
    return np.array(Qs), np.array(pis)


def _tree(name, seed):
    if ":" in name:
        sh = by_name(name.split(":")[1], rooted_catalogue(2, 4))
        blen = np.random.default_rng(seed).uniform(0.03, 0.5, size=sh.nn)
        blen[-1] = 0.0
        return sh.parent, blen, sh.lot
    if name == "n4x5":
        parent, lot = _balanced(13)
        blen = np.random.default_rng(seed).uniform(0.03, 0.4, size=len(parent))
        blen[-1] = 0.0
        return parent, blen, lot
    return rooted_random_tree(9 if name in ("p20x4", "p20x6", "p20x9", "n4x4") else 6, 31)


@lru_cache(maxsize=None)
def case(name, variant=0):
    """the case of that name; variant 1: the second data set of the two-data-set null -- the same topology with other
    generators, another assignment of them, other root frequencies and scaled branch lengths"""
    S, C = {"p": 20, "n": 4, "c": 61, "s": 7, "w": 64}[name[0]], int(name.split(":")[0].split("x")[1])
    seed = sum(map(ord, name)) + 1000 * variant
    rng = np.random.default_rng(seed)
    parent, blen, lot = _tree(name, sum(map(ord, name)))
    if variant:
        blen = blen * rng.uniform(0.5, 1.5, size=len(blen))
    Qs, pis = _generators(S, seed)
    nn = len(parent)
    mob = rng.integers(0, 3, size=nn).astype(np.int32)
    kids = np.flatnonzero(parent == nn - 1)
    mob[kids[0]], mob[kids[1]] = (0, 1) if not variant else (2, 0)
    if nn > 3:
        mob[[b for b in range(nn - 1) if b not in kids[:2]][0]] = 2 if not variant else 1
    rates, probs = pm.gamma_rates(0.6 + 0.3 * variant, C)
    return dict(name=name, S=S, C=C, parent=parent, blen=blen, lot=lot, Qs=Qs, pis=pis, mob=mob,
                root=rng.dirichlet(np.full(S, 5.0)), rates=np.asarray(rates), probs=np.asarray(probs))


def long_case():
    """p20x4 with branches eight times as long and nearly equal rates: simulated columns are then all distinct, which the
    clustering needs (equal columns give distances that tie or not depending on rounding)"""
    c = dict(case("p20x4"))
    rates, probs = pm.gamma_rates(5.0, 4)
    c.update(name="p20x4:long", blen=c["blen"] * 8.0, rates=np.asarray(rates), probs=np.asarray(probs))
    return c


def registers(c, K=1):
    """Bks [3, K, S, S]: the total register of every generator, or (K = 2) split into two types that add up to it"""
    B0 = np.array([synthetic.weighted_register(q) for q in c["Qs"]])
    if K == 1:
        return B0[:, None]
    ts = np.triu(np.ones((c["S"], c["S"])), 1)
    ts = ts + ts.T
    ts[:, ::2] = 0                                      # type 0 = into odd states, type 1 = the rest
    return np.stack([B0 * ts, B0 * (1 - ts)], axis=1)


def oracle_of(c, mob=None, root=None, **kw):
    return oracle.ModelSet(c["parent"], c["blen"], c["lot"], c["Qs"], c["pis"], c["rates"], c["probs"],
                           c["mob"] if mob is None else mob, c["root"] if root is None else root, **kw)


def engine_of(c, **kw):
    from comap_amd import engine
    return engine.Engine(c["parent"], c["blen"], c["lot"], c["Qs"], c["pis"], c["rates"], c["probs"], model_of_branch=c["mob"],
                         root_freqs=c["root"], **kw)


def alignment(c, nsites=70, ambiguous=False):
    """nsites columns: two thirds simulated under the set, the rest uniform random; with ambiguous, 15 % of the cells
    carry an ambiguity code (IUPAC ids 4 .. 15 at 4 states, the unknown S elsewhere)"""
    sim, _ = oracle.simulate(oracle_of(c), 4321, 10 ** 7, nsites - nsites // 3)
    rng = np.random.default_rng(c["S"] + nsites)
    aln = np.concatenate([sim, rng.integers(0, c["S"], size=(len(c["lot"]), nsites // 3)).astype(np.uint8)], axis=1)
    if ambiguous:
        hit = rng.random(aln.shape) < 0.15
        aln[hit] = rng.integers(4, 16, size=int(hit.sum()), dtype=np.uint8) if c["S"] == 4 else c["S"]
    return np.ascontiguousarray(aln)


# ---------------------------------------------------------------------------------------------- simulator inputs
SIM_SEED, SIM_G0, SIM_N = 987654321, 12345, 3000          # eng.simulate of every simulator case (an odd g0)
GATHER = dict(seed=77, rep_begin=3, rep_end=5, rep_ram=700)
CHAIN = [("p20x4", dict(seed=77, rep_begin=0, rep_end=1, rep_ram=37_500)),     # 75 000 sites: the LDS-table kernel's threshold
         ("p20x6", dict(seed=77, rep_begin=1, rep_end=3, rep_ram=18_751))]     # 75 004 sites, an odd rep_ram, two replicates
# the LDS-table kernel at a few thousand sites (tests/test_gpu_simulator_chain.py): models with a node block of 23 040,
# 19 456 and 18 544 bytes (three 16-byte pieces per thread), and two without tables (28 000 and 37 088 bytes; the limit
# is 24 576)
CHAIN_EDGE_CASES = ["p20x9", "w64x1", "c61x1", "s7x50", "c61x2"]
CHAIN_EDGE_CALLS = [(0, 1, 513), (1, 2, 2050), (2, 4, 1536)]                   # (rep_begin, rep_end, rep_ram)
CHAIN_EDGE_SEED = 4711
CONTINUOUS = dict(seed=77, g0=1000, n=600, rates=((0.5, 0.0), (1.7, 0.2)))
CONTINUOUS_NULL = dict(seed=5, rep_begin=2, rep_end=4, rep_ram=64, alpha=0.5, p_inv=0.1)
NULL = dict(seed=777, nrep=3, rep_ram=50)
NULL_INTER = dict(seed=4242, rep_begin=1, rep_end=3, rep_ram=70)
CLUSTER = dict(seed=123, rep_begin=2, rep_end=4, nsites=40)
CANDIDATES = dict(seed=2024, rep_ram=48)                    # batches 0 .. 15 at the most are bounded below
MICA = dict(seed=77, nrep=2, rep_ram=64)


def _null_range(rep_begin, rep_end, rep_ram, **_):
    return rep_begin * 2 * rep_ram, (rep_end - rep_begin) * 2 * rep_ram


def discrete_inputs():
    """[(label, case, seed, g0, n)]: every range of global site indices that a GPU test has the discrete simulator draw"""
    out = [(f"simulate:{n}", case(n), SIM_SEED, SIM_G0, SIM_N) for n in SIMULATOR_CASES]
    out += [(f"gather:{n}", case(n), GATHER["seed"], *_null_range(**GATHER)) for n in SIMULATOR_CASES]
    out += [(f"chain:{n}", case(n), kw["seed"], *_null_range(**kw)) for n, kw in CHAIN]
    out += [(f"chain-edge:{n}:{rb}", case(n), CHAIN_EDGE_SEED, *_null_range(rb, re, ram)) for n in CHAIN_EDGE_CASES
            for rb, re, ram in CHAIN_EDGE_CALLS]
    for n in NULL_CASES:
        out.append((f"null:{n}", case(n), NULL["seed"], 0, NULL["nrep"] * 2 * NULL["rep_ram"]))
        out.append((f"supplied:{n}", case(n), 5, 0, NULL["nrep"] * 2 * NULL["rep_ram"]))
        out.append((f"inter1:{n}", case(n), NULL_INTER["seed"], *_null_range(**NULL_INTER)))
        out.append((f"inter2:{n}", case(n, 1), NULL_INTER["seed"], *_null_range(**NULL_INTER)))
    c = case("p20x4")
    out.append(("cluster", long_case(), CLUSTER["seed"], CLUSTER["rep_begin"] * CLUSTER["nsites"],
                (CLUSTER["rep_end"] - CLUSTER["rep_begin"]) * CLUSTER["nsites"]))
    out.append(("candidates", c, CANDIDATES["seed"], 0, 16 * CANDIDATES["rep_ram"]))
    out.append(("mica", c, MICA["seed"], 0, MICA["nrep"] * 2 * MICA["rep_ram"]))
    return out


def continuous_inputs():
    """[(label, case, seed, g0, n, alpha, p_inv)] of the continuous-rate simulator"""
    out = []
    for n in CONTINUOUS_CASES:
        for a, p in CONTINUOUS["rates"]:
            out.append((f"continuous:{n}:{a}", case(n), CONTINUOUS["seed"], CONTINUOUS["g0"], CONTINUOUS["n"], a, p))
        k = CONTINUOUS_NULL
        out.append((f"continuous-null:{n}", case(n), k["seed"], *_null_range(k["rep_begin"], k["rep_end"], k["rep_ram"]),
                    k["alpha"], k["p_inv"]))
    return out


def fragile(near):
    return np.asarray(near) < oracle.FRAGILE
