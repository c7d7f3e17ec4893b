"""Tiny, rooted and degenerate trees on the host (no GPU): the catalogue of tests/tree_shapes.py -- every rooted shape of
2..7 leaves in both child orders, random_tree's unrooted forms, each with five branch-length variants (all 0.1, a zero leaf
branch, a zero internal branch, a saturated 5.0 branch, all 1e-6).

* The walk: `debug_walk` compiles what the mapping kernel reads and self-checks both walks numerically (verify_walk); here
  also the cherry count (recomputed from `parent`), every taxon in the leaf operators, and the operator / load counts
  against the returned schedules, for protein G4, fused DNA G4, fused DNA with 5 classes and DNA with two substitution
  types.
* The oracle: pinned on these shapes WITHOUT its pruning, by brute force over every assignment of internal states, with
  scipy's expm for P(t) and the Van Loan block exponential expm([[Q, B], [0, Q]] r t)[:S, S:] / P for the conditional
  counts (B = Q o W off the diagonal; the guards non-finite -> 0 and, unweighted, negative -> 0 as in oracle.c).  The
  count of branch b is the joint posterior of (class, state at the father, state at the son) times N_c(x, y), summed:
  the class average the Myoglobin goldens pin."""
import itertools

import numpy as np
import pytest
import scipy.linalg

import oracle
from comap_amd import engine, synthetic
from tree_shapes import catalogue

SHAPES = catalogue(2, 7)
IDS = [s.name for s in SHAPES]


def _model(name):
    """-> (model dict, Bk or None, fused)"""
    if name == "protein_g4":
        return synthetic.protein_model(0.5, 4), None, False
    if name == "dna_g4":
        return synthetic.dna_model(0.7, 4), None, True
    if name == "dna_5cls":
        return synthetic.dna_model(0.7, 5), None, True
    assert name == "dna_2types"
    m = synthetic.dna_model(0.7, 4)
    W1 = np.random.default_rng(4).uniform(-1, 1, size=(4, 4))
    return m, np.stack([synthetic.weighted_register(m["Q"], W1), synthetic.weighted_register(m["Q"], np.abs(W1))]), True


MODELS = ["protein_g4", "dna_g4", "dna_5cls", "dna_2types"]


def _walk(shape, blen, mdl, Bk):
    return engine.debug_walk(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_walk_compiles_and_self_checks(shape, model):
    mdl, Bk, fused = _model(model)
    K = 1 if Bk is None else len(Bk)
    ncherry = len(shape.cherries()) if fused else 0
    for vname, blen in shape.blen_variants():
        d = _walk(shape, blen, mdl, Bk)                # fails unless both walks reproduce a direct pruning computation
        assert d["cherry_tables"] == ncherry, (vname, d["cherry_tables"], ncherry)
        ops = d["msched"]
        assert ((ops[:, 1] >= -1) & (ops[:, 1] < shape.ntaxa)).all()
        leaf_ops = ops[ops[:, 1] >= 0]
        assert set(leaf_ops[:, 1].tolist()) == set(range(shape.ntaxa))     # every taxon's branch is applied
        assert len(leaf_ops) == d["leaf_ops"] and len(ops) - len(leaf_ops) == d["products"]
        assert len(leaf_ops) >= 3 * shape.ntaxa
        assert d["loads"] == len(d["ldsched"])
        if len(d["ldsched"]):
            _, counts = np.unique(d["ldsched"] & 0x40ffffff, return_counts=True)
            assert counts.max() <= 2
        assert d["loads"] <= d["stores"] * 2 and (d["stores"] == 0) == (d["loads"] == 0)
        if not fused:
            assert d["products_tables"] == 0 and d["leaf_ops_tables"] == 0                   # no table walk at all
        elif ncherry == 0:
            assert d["products_tables"] == d["products"] and d["leaf_ops_tables"] == d["leaf_ops"]   # the same stream
        else:
            assert d["products_tables"] <= d["products"] and d["leaf_ops_tables"] <= d["leaf_ops"]
            if K == 1:       # a cherry with tables: its message is 1 op instead of 3, its outside visit 3 K instead of 5 + 3 K
                assert d["products_tables"] + d["leaf_ops_tables"] == d["products"] + d["leaf_ops"] - ncherry * 9


def test_catalogue_covers_what_the_tests_rely_on():
    from tree_shapes import rooted_shapes
    assert [len(rooted_shapes(n)) for n in range(1, 8)] == [1, 1, 2, 5, 12, 33, 90]        # OEIS A000669
    n = {k: sum(1 for s in SHAPES if s.ntaxa == k and s.rooted) for k in range(2, 8)}
    assert all(len(rooted_shapes(k)) < n[k] < 2 * len(rooted_shapes(k)) for k in range(3, 8))   # + mirrored child orders
    names = set(IDS)
    for s in ("(x,x)", "((x,x),x)", "(x,(x,x))", "(x,x,x)", "((x,x),(x,x))", "(((x,x),x),x)", "((x,x,x),(x,x,x))"):
        assert s in names, s
    for s in SHAPES:
        assert s.parent[-1] == -1 and (s.parent[:-1] > np.arange(s.nn - 1)).all()           # post-order, root last
        assert sorted(s.lot.tolist()) == np.flatnonzero(s.is_leaf()).tolist()
        for _, bl in s.blen_variants():
            assert bl[-1] == 0.0 and (bl >= 0).all()
    # taxa are not numbered in post-order everywhere
    assert sum(1 for s in SHAPES if not np.array_equal(s.lot, np.sort(s.lot))) > len(SHAPES) // 2


# ------------------------------------------------------------------------------------------------ the brute-force oracle
def _van_loan(Q, Bm, t):
    """(P, J): P = expm(Q t), J = int_0^t expm(Q s) B expm(Q (t - s)) ds from one block exponential"""
    S = Q.shape[0]
    big = np.zeros((2 * S, 2 * S))
    big[:S, :S] = Q
    big[:S, S:] = Bm
    big[S:, S:] = Q
    E = scipy.linalg.expm(big * t)
    return scipy.linalg.expm(Q * t), E[:S, S:]


def _brute_map(parent, blen, lot, Q, pi, rates, probs, Bk, nonneg, aln):
    """every assignment of internal states enumerated: logL, post_rate, the class likelihoods p_c L_c, counts [N, B, K]"""
    nn, S, C, K = len(parent), len(pi), len(rates), len(Bk)
    T, N = aln.shape
    root, B = nn - 1, nn - 1
    leaf = np.zeros(nn, dtype=bool)
    leaf[lot] = True
    internal = np.flatnonzero(~leaf)
    P = np.zeros((C, B, S, S))
    Nc = np.zeros((C, B, K, S, S))
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(C):
            for b in range(B):
                for k in range(K):
                    P[c, b], J = _van_loan(Q, Bk[k], blen[b] * rates[c])
                    n = J / P[c, b]
                    n[~np.isfinite(n)] = 0.0
                    if nonneg:
                        n[n < 0] = 0.0
                    Nc[c, b, k] = n
    cfg = np.array(list(itertools.product(range(S), repeat=len(internal))), dtype=np.int64).reshape(-1, len(internal))
    M = len(cfg)
    st = np.zeros((N, M, nn), dtype=np.int64)
    st[:, :, internal] = cfg[None]
    for t in range(T):
        st[:, :, lot[t]] = aln[t][:, None]
    w = probs[:, None, None] * pi[st[:, :, root]][None]                     # [C, N, M]
    for b in range(B):
        w = w * P[:, b][:, st[:, :, parent[b]], st[:, :, b]]
    Lc = w.sum(axis=2)                                                       # p_c L_c  [C, N]
    L = Lc.sum(axis=0)
    counts = np.zeros((N, B, K))
    for b in range(B):
        for k in range(K):
            counts[:, b, k] = (w * Nc[:, b, k][:, st[:, :, parent[b]], st[:, :, b]]).sum(axis=(0, 2)) / L
    return dict(logL=np.log(L), post_rate=(rates[:, None] * Lc).sum(axis=0) / L, Lc=Lc, counts=counts)


def _columns(T, S, rng, n_random):
    """every column pattern when there are few, else random columns"""
    if S ** T <= 400:
        return np.array(list(itertools.product(range(S), repeat=T)), dtype=np.uint8).T.copy()
    return rng.integers(0, S, size=(T, n_random)).astype(np.uint8)


BRUTE = [s for s in SHAPES if s.ntaxa <= 5]
# (logL rtol, counts rtol) per branch-length variant; post_rate gets 10 x the first.  The oracle's P(t) = V e^{lambda t} V^-1
# is accurate to ~1e-15 ABSOLUTE (7e-16 for DNA, 4e-15 for the 20-state model), so where a likelihood rests on small
# entries of P -- a zero branch (P = V V^-1 = I + O(1e-16), not I) or 1e-6 branches (off-diagonal entries of 1e-7 .. 1e-10)
# -- its relative accuracy is that over the entry, and the tolerance follows it.  Everywhere else: 1e-12.
_TOL = {"b0.1": (1e-12, 1e-10), "inner0": (1e-12, 1e-10), "sat5": (1e-12, 1e-10), "leaf0": (1e-10, 1e-8),
        "b1e-6": {4: (1e-9, 1e-7), 20: (1e-7, 1e-5)}}


@pytest.mark.parametrize("shape", BRUTE, ids=[s.name for s in BRUTE])
def test_oracle_mapping_equals_brute_force(shape):
    models = ["dna_g4", "dna_5cls", "dna_2types"] + (["protein_g4"] if shape.ntaxa <= 3 else [])
    rng = np.random.default_rng(shape.nn * 7 + shape.ntaxa)
    for model in models:
        mdl, Bk, _ = _model(model)
        S = len(mdl["pi"])
        nonneg = Bk is None
        Bk = Bk if Bk is not None else synthetic.weighted_register(mdl["Q"])[None]
        aln = _columns(shape.ntaxa, S, rng, 64 if S == 4 else 40)
        for vname, blen in shape.blen_variants():
            om = oracle.Model(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk,
                              nonneg=nonneg)
            o = oracle.map_sites(om, aln)
            r = _brute_map(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk, nonneg, aln)
            where = f"{model} {vname}"
            rt, rc = _TOL[vname] if vname != "b1e-6" else _TOL[vname][S]
            np.testing.assert_allclose(o["logL"], r["logL"], rtol=rt, err_msg=where)
            np.testing.assert_allclose(o["post_rate"], r["post_rate"], rtol=10 * rt, err_msg=where)
            # the arg-max class: the oracle's pick must be a maximum of p_c L_c (to the tolerance: equal classes are ties)
            best = r["Lc"].max(axis=0)
            picked = r["Lc"][o["rate_class"], np.arange(aln.shape[1])]
            assert (picked >= best * (1 - 10 * rt)).all(), where
            clear = np.sort(r["Lc"], axis=0)[-2] < best * (1 - 1e3 * rt)
            assert clear.mean() > 0.5 and np.array_equal(o["rate_class"][clear], r["Lc"].argmax(axis=0)[clear]), where
            np.testing.assert_allclose(o["counts"], r["counts"], rtol=rc, atol=1e-13, err_msg=where)
            np.testing.assert_allclose(o["norm"], np.sqrt((r["counts"].sum(axis=2) ** 2).sum(axis=1)), rtol=rc,
                                       atol=1e-13, err_msg=where)
            # a zero-length branch carries no substitution
            zero = np.flatnonzero(blen[:-1] == 0.0)
            assert (o["counts"][:, zero] == 0.0).all(), where


def test_two_taxon_tree_with_equal_branches():
    """the degenerate input of tests/test_gpu_tiny_trees.py.  On (x,x) with equal branch lengths reversibility makes the
    branch above taxon 0 at column (a, b) carry what the branch above taxon 1 carries at column (b, a); at a constant
    column the two totals are therefore equal in exact arithmetic, the centred vector is zero and the correlation 0 / 0"""
    from tree_shapes import by_name
    s = by_name("(x,x)", SHAPES)
    blen = s.blen_variants()[0][1]
    for model in MODELS:
        mdl, Bk, _ = _model(model)
        S = len(mdl["pi"])
        aln = _columns(2, S, None, 0)                                   # every (a, b)
        Bk = synthetic.weighted_register(mdl["Q"])[None] if Bk is None else Bk
        om = oracle.Model(s.parent, blen, s.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk)
        o = oracle.map_sites(om, aln)
        r = _brute_map(s.parent, blen, s.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk, True, aln)
        swap = aln[0].astype(int) * S + aln[1] == (aln[1].astype(int) * S + aln[0])[:, None]   # [i, j]: column j = column i swapped
        j = swap.argmax(axis=1)
        b0, b1 = s.lot                                                  # the branches above taxon 0 and taxon 1
        np.testing.assert_allclose(r["counts"][:, b0], r["counts"][j, b1], rtol=1e-12, atol=1e-15)
        const = aln[0] == aln[1]
        tot = o["counts"].sum(axis=2)
        np.testing.assert_allclose(tot[const, b0], tot[const, b1], rtol=1e-12)
        assert (np.abs(tot[~const, b0] - tot[~const, b1]) > 1e-6 * tot[~const].max()).any()   # not equal in general
