"""The models, rate sets and tree profiles of tests/golden/operator_edges.npz, a plain helper module shared by the fixture's
generator (tests/golden/make_operator_edge_fixture.py), tests/test_operator_edges.py (CPU) and
tests/test_gpu_operator_edges.py: branch lengths and rates at the edges of what build_branch_matrices
(comap_amd/csrc/cmx_host_model.cpp) is given -- zero, 1e-100, 1e-12, saturated --, rate-zero classes and degenerate spectra.

Conventions are the engine's: nodes in post-order, root last, branch b = the branch above node b.

    tree "t4"   ((a,b),(c,d)):   a 0, b 1, ab 2, c 3, d 4, cd 5, root 6     ("the internal branch": 2)
    tree "t5"   ((a,b),(c,d),e): a 0, b 1, ab 2, c 3, d 4, cd 5, e 6, root 7 (a trifurcating root)

    profile 1   terminal branch a at 0                  5   terminal branch c at 1e-100
            2   the cherry (a, b): both at 0            6   terminal a and internal ab at 150 (past where the old form failed)
            3   the internal branch ab at 0             7   terminal c at 10000 (Bio++'s upper bound)
            4   every branch at 1e-12                   8   terminal b at 120 (the old form still finite: bits pinned)

tests/golden/null_walk_edges.npz (make_null_walk_fixture.py; DEEP_CASES) adds a tree whose walk stores and loads workspace
vectors, uses the LDS slot and a wait plan, and has cherries with more than the root above them:

    tree "t12"  ((((a,b),c),d),((e,f),(g,h)),(i,(j,(k,l)))):  a 0, b 1, ab 2, c 3, abc 4, d 5, abcd 6, e 7, f 8, ef 9, g 10,
                h 11, gh 12, efgh 13, i 14, j 15, k 16, l 17, kl 18, jkl 19, ijkl 20, root 21: a trifurcating root, four
                inlined cherries, a ladder above (a, b) and one below i, a balanced quartet; ordinary lengths in [0.05, 0.4]

    profile q1  the cherry (a, b): both at 0; terminal k at 1e-100
            q2  the branch above (a, b) at 0; the branch above ((e,f),(g,h)) and terminal g at 150
            q3  the six branches inside ((e,f),(g,h)) at 1e-12: counts of 1e-12 beside counts of order 1 in one vector
            q4  terminal c at 10000; the branch above (k, l) at 120
"""
import numpy as np

import oracle
from comap_amd import protein_models as pm, synthetic

NSITES = 70          # one full 64-site block and a partial one; four 16-site tiles and one of 6
TREES = {
    "t4": (np.array([2, 2, 6, 5, 5, 6, -1], dtype=np.int32), np.array([0.05, 0.12, 0.2, 0.3, 0.08, 0.15, 0.0]),
           np.array([0, 1, 3, 4], dtype=np.int32)),
    "t5": (np.array([2, 2, 7, 5, 5, 7, 7, -1], dtype=np.int32), np.array([0.05, 0.12, 0.2, 0.3, 0.08, 0.15, 0.25, 0.0]),
           np.array([0, 1, 3, 4, 6], dtype=np.int32)),
}
_T12_BLEN = np.round(np.random.default_rng(1212).uniform(0.05, 0.4, size=22), 3)
_T12_BLEN[-1] = 0.0
TREES["t12"] = (np.array([2, 2, 4, 4, 6, 6, 21, 9, 9, 13, 12, 12, 13, 21, 20, 19, 18, 18, 19, 20, 21, -1], dtype=np.int32),
                _T12_BLEN, np.array([0, 1, 3, 5, 7, 8, 10, 11, 14, 15, 16, 17], dtype=np.int32))
DEEP_PROFILES = {"q1": {0: 0.0, 1: 0.0, 16: 1e-100}, "q2": {2: 0.0, 13: 150.0, 10: 150.0},
                 "q3": {b: 1e-12 for b in range(7, 13)}, "q4": {3: 10000.0, 18: 120.0}}
PROFILES = {1: {0: 0.0}, 2: {0: 0.0, 1: 0.0}, 3: {2: 0.0}, 4: "all 1e-12", 5: {3: 1e-100}, 6: {0: 150.0, 2: 150.0},
            7: {3: 10000.0}, 8: {1: 120.0}}
# times at which the operators themselves are stored (S <= 20): the profiles' lengths and their products with the Gamma(4)
# rates' top class (2.894), and ordinary ones between
OPERATOR_TIMES = [0.0, 1e-100, 1e-12, 1e-3, 0.3, 12.0, 120.0, 150.0, 347.0, 434.0, 10000.0, 28940.0]
OPERATOR_TIMES_DEGENERATE = [0.0, 1e-12, 0.3, 120.0, 434.0, 28940.0]


def blen_of(tree, profile):
    blen = TREES[tree][1].copy()
    p = DEEP_PROFILES[profile] if profile in DEEP_PROFILES else PROFILES[profile]
    if isinstance(p, str):
        blen[:-1] = 1e-12
    else:
        for b, t in p.items():
            blen[b] = t
    return blen


def _jukes_cantor_like(S, perturbed):
    """all non-zero eigenvalues equal (-S / (S - 1)); perturbed: the exchangeabilities moved by 1e-13 relative, so that the
    eigenvalues differ by about that much"""
    exch = np.ones((S, S))
    if perturbed:
        u = np.random.default_rng(1300 + S).uniform(-1.0, 1.0, size=(S, S))
        exch = exch * (1.0 + 1e-13 * (u + u.T) / 2)
    return pm.reversible_generator(exch, np.full(S, 1.0 / S))


def generator(name):
    """-> (Q, pi, Bk [K, S, S] or None for the total register, clamp_negative)"""
    Bk, clamp = None, True
    if name == "dna":
        m = synthetic.dna_model(0.5, 4)
        Q, pi = m["Q"], m["pi"]
    elif name in ("protein", "protein_k2", "protein_signed"):
        m = synthetic.protein_model(0.5, 4)
        Q, pi = m["Q"], m["pi"]
        x = np.arange(20)
        if name == "protein_k2":        # the total register split by the parity of y - x
            odd = (np.abs(x[None, :] - x[:, None]) % 2 == 1)
            Bk = np.stack([synthetic.weighted_register(Q, odd.astype(np.float64)),
                           synthetic.weighted_register(Q, (~odd).astype(np.float64))])
        elif name == "protein_signed":  # W(x, y) = (y - x) / 10: antisymmetric, counts of either sign
            Bk, clamp = synthetic.weighted_register(Q, (x[None, :] - x[:, None]) / 10.0)[None], False
    elif name.startswith("jc"):         # jc4, jc20, jcp4, jcp20
        Q, pi = _jukes_cantor_like(int(name.lstrip("jcp")), name.startswith("jcp"))
    elif name in ("s7", "s61"):
        Q, pi = pm.synthetic_reversible(int(name[1:]), 161)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(Q), np.ascontiguousarray(pi), Bk, clamp


def rate_set(name):
    """g4: Gamma(4), alpha = 0.5; ig5: Invariant + Gamma(4), class 0 at rate 0 with probability 0.2; c1: one class"""
    r, p = pm.gamma_rates(0.5, 4)
    if name == "g4":
        return np.asarray(r, dtype=np.float64), np.asarray(p, dtype=np.float64)
    if name == "ig5":
        return np.concatenate([[0.0], r]), np.concatenate([[0.2], 0.8 * np.asarray(p)])
    if name == "c1":
        return np.array([1.0]), np.array([1.0])
    raise KeyError(name)


# (generator, rate set, tree, profiles): the smallest selection that reaches every consumer of the operators -- the 20-state
# walk (64-site and class-split), the fused 16- and 20-state nucleotide layouts and the unfused one, the plain kernels
# (S = 7), the wide kernels (S = 61), K = 2 and a signed register, every profile at S = 4 and S = 20
GRID = [
    ("dna", "g4", "t4", (1, 2, 3, 4, 5, 6, 7, 8)),
    ("dna", "ig5", "t5", (1, 2, 6, 7)),
    ("dna", "c1", "t4", (1, 3, 6)),
    ("jc4", "g4", "t4", (1, 6)),
    ("jcp4", "g4", "t4", (1, 6)),
    ("protein", "g4", "t5", (1, 2, 3, 4, 5, 6, 7, 8)),
    ("protein", "ig5", "t4", (2, 6)),
    ("protein", "c1", "t4", (7,)),
    ("jc20", "g4", "t4", (1, 6)),
    ("jcp20", "g4", "t4", (1, 6)),
    ("protein_k2", "g4", "t4", (6,)),
    ("protein_signed", "g4", "t4", (1, 6)),
    ("s7", "g4", "t5", (1, 3, 6, 7)),
    ("s7", "ig5", "t4", (2,)),
    ("s61", "g4", "t4", (1, 4, 6, 8)),
]
CASES = [f"{g}-{r}-{t}-p{p}" for g, r, t, ps in GRID for p in ps]
# the cases of null_walk_edges.npz: 45 columns each, no unknowns; counts, logL, post_rate, rate_class, class_clear only
DEEP_NSITES = 45
DEEP_GRID = [
    ("protein", "g4", ("q1", "q2", "q3", "q4")),
    ("protein", "ig5", ("q1", "q2")),
    ("jc20", "g4", ("q2",)),
    ("protein_k2", "g4", ("q2",)),
    ("protein_signed", "g4", ("q1",)),
    ("dna", "g4", ("q1", "q2", "q3", "q4")),
    ("dna", "ig5", ("q1", "q2")),
    ("dna", "c1", ("q1", "q2")),
    ("jc4", "g4", ("q2",)),
]
DEEP_CASES = [f"{g}-{r}-t12-{q}" for g, r, qs in DEEP_GRID for q in qs]
OPERATOR_MODELS = ["dna", "jc4", "jcp4", "protein", "protein_signed", "jc20", "jcp20", "s7"]


ANCESTRAL_CASES = ["protein-g4-t5-p1", "protein-g4-t5-p3", "protein-g4-t5-p6"]     # 20 states: P is stored for these too


def ancestral_times():
    """the distinct r_c t_b of ANCESTRAL_CASES, ascending: fixture keys anc.protein.t / anc.protein.P"""
    ts = set()
    for name in ANCESTRAL_CASES:
        i = Inputs(name)
        ts.update(float(i.blen[b]) * float(r) for b in range(len(i.blen) - 1) for r in i.rates)
    return sorted(ts)


def ancestral_P(fix, c):
    """P [C, B, S, S] of a stored case: its own for S <= 7, looked up by time for the 20-state ANCESTRAL_CASES"""
    if "P" in c:
        return c["P"]
    ts = list(fix["anc.protein.t"])
    return np.array([[fix["anc.protein.P"][ts.index(float(t) * float(r))] for t in c["blen"][:-1]] for r in c["rates"]])


def has_variants(name):
    """the cases that also hold the three other nijt options: no time (profiles 1, 2, the rate-zero class) and saturated
    branches (6, 7), where every conditional count N = J / P the options read is defined; on the 1e-12 and 1e-100 branches
    (4, 5) P's entries are below its own rounding and a single N(x, y) is not.  Up to 20 states (the generator's minutes)."""
    return not name.startswith("s61") and ("-ig5-" in name or name[-1] in "1267")


def operator_times(gen):
    return OPERATOR_TIMES_DEGENERATE if gen.startswith("jc") else OPERATOR_TIMES


class Inputs:
    """what a case is computed from; the alignment is drawn by oracle.simulate under the case's own tree, so no site is
    impossible under it (zero-length sisters come out equal, sites of the rate-zero class constant); a few symbols are set
    to unknown afterwards"""

    def __init__(self, name):
        gen, rs, tree, prof = name.split("-")
        self.deep = prof in DEEP_PROFILES
        self.name, self.gen, self.rs, self.tree, self.profile = name, gen, rs, tree, prof if self.deep else int(prof[1:])
        self.parent, _, self.lot = TREES[tree]
        self.blen = blen_of(tree, self.profile)
        self.Q, self.pi, self.Bk, self.clamp = generator(gen)
        self.rates, self.probs = rate_set(rs)
        self.S = len(self.pi)
        self.seed = 9500 + DEEP_CASES.index(name) if self.deep else 9000 + CASES.index(name)

    def oracle_model(self, method=oracle.METHOD_UNIF):
        return oracle.Model(self.parent, self.blen, self.lot, self.Q, self.pi, self.rates, self.probs, Bk=self.Bk,
                            method=method, nonneg=self.clamp)

    def draw(self):
        """-> (aln [T, NSITES] with the unknowns set, the drawn classes); a DEEP_CASES case: DEEP_NSITES, no unknowns"""
        if self.deep:
            return oracle.simulate(self.oracle_model(), self.seed, 0, DEEP_NSITES)
        aln, cls = oracle.simulate(self.oracle_model(), self.seed, 0, NSITES)
        aln = aln.copy()
        aln[1, 5] = aln[2, 40] = aln[0, 66] = aln[len(self.lot) - 1, 69] = self.S
        return aln, cls


STAR_LEAVES = 62     # scaled_cases.star shrunk to the fewest leaves at which scaled_reference rescales a site under ig5 rates


def star_case(nleaves=STAR_LEAVES):
    """-> (scaled_cases.star(nleaves), rates, probs, aln): 8 sites drawn under Invariant + Gamma(4): the constant ones from
    class 0; on the variable ones class 0 has likelihood exactly 0 and, at STAR_LEAVES, the fastest class is rescaled"""
    import scaled_cases as sc
    base = sc.star(nleaves)
    rates, probs = rate_set("ig5")
    om = oracle.Model(base.parent, base.blen, base.lot, base.Q, base.pi, rates, probs)
    return base, rates, probs, np.ascontiguousarray(oracle.simulate(om, 78, 0, 8)[0])


def load(fix, name):
    """the stored case `name` of the opened fixture as a dict"""
    return {k[len(name) + 1:]: fix[k] for k in fix.files if k.startswith(name + ".")}


def register_of(c):
    """Bk as Engine and oracle.Model take it (None: the total register)"""
    return c["Bk"] if c["Bk"].size else None
