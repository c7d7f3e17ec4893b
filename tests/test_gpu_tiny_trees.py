"""-m gpu: tiny, rooted and degenerate trees (tests/tree_shapes.py, 2..6 leaves, one Engine per shape and model) against
the oracle: the observed mapping, the fused null, the cherry-table walk against the generic walk, and at 2, 3 and 4
leaves the other null paths, the pair loop with p-values and the pair statistics at B = 2, 3, 4 branches (B < 4 leaves
padding rows in the Gram kernel's operand).  Tolerances are _check_map's and the parity module's.

The degenerate-input rule.  The correlation centres a site's per-branch vector; where that centred vector is zero in
exact arithmetic -- on (x,x) with equal branches at every constant column, on a star with equal branches at a constant
column -- what either side computes is 0 / 0 of rounding noise: NaN, or a value of magnitude 1 at B = 2.  Such a vector
is recognised on the ORACLE's vector as a centred norm below 1e-9 of the vector's own norm (true differences on these
trees are > 1e-3 of it).  For a pair with such a site both sides must give NaN or a value in [-1, 1] (to 1e-12);
everywhere else NaN patterns and values must match as usual (rel_close, unchanged)."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from test_gpu_parity import _check_map
from tree_shapes import by_name, catalogue

pytestmark = pytest.mark.gpu

SHAPES = catalogue(2, 6)
MODELS = ["protein_g4", "dna_g4", "dna_5cls", "dna_2types"]


def _model(name):
    """-> (model dict, Bk or None)"""
    if name == "protein_g4":
        return synthetic.protein_model(0.5, 4), None
    if name == "dna_g4":
        return synthetic.dna_model(0.7, 4), None
    if name == "dna_5cls":
        return synthetic.dna_model(0.7, 5), None
    m = synthetic.dna_model(0.7, 4)
    W1 = np.random.default_rng(4).uniform(-1, 1, size=(4, 4))
    return m, np.stack([synthetic.weighted_register(m["Q"], W1), synthetic.weighted_register(m["Q"], np.abs(W1))])


def _pair(shape, model, variant):
    """(engine, oracle model, blen, S, kind of the null statistic)"""
    mdl, Bk = _model(model)
    vs = dict(shape.blen_variants())
    blen = vs[variant] if isinstance(variant, str) else list(vs.values())[variant % len(vs)]
    kw = {} if Bk is None else dict(Bk=Bk)
    eng = engine.Engine(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"],
                        clamp_negative=Bk is None, **kw)
    om = oracle.Model(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], nonneg=Bk is None, **kw)
    return eng, om, blen, len(mdl["pi"]), (engine.STAT_CORRELATION if Bk is None else engine.STAT_COMPENSATION)


def _degenerate(counts):
    """sites whose type-0 per-branch vector has a zero-norm centred vector (up to rounding): [N] bool"""
    v = np.asarray(counts)[:, :, 0]
    c = v - v.mean(axis=1, keepdims=True)
    return np.linalg.norm(c, axis=1) <= 1e-9 * np.linalg.norm(v, axis=1)


def _stat_close(g, o, deg_pairs, rtol=1e-6, atol=1e-12):
    """the module's rule: pairs with a degenerate site -> NaN or [-1, 1] on both sides; the rest as usual"""
    g, o = np.asarray(g, dtype=np.float64), np.asarray(o, dtype=np.float64)
    assert g.shape == o.shape == deg_pairs.shape
    for x in (g[deg_pairs], o[deg_pairs]):
        ok = np.isnan(x) | (np.abs(x) <= 1 + 1e-12)
        assert ok.all(), x[~ok]
    rel_close(g[~deg_pairs], o[~deg_pairs], rtol, atol)


def _alignment(om, S, T, seed):
    """40 simulated columns (mostly constant on short branches) + 24 uniform random ones"""
    sim, _ = oracle.simulate(om, seed, 0, 40)
    rnd = np.random.default_rng(seed).integers(0, S, size=(T, 24)).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([sim, rnd], axis=1))


def _null_vectors(om, seed, nrep, ram, supplied=None):
    """the oracle's per-site vectors of the two batches of every replicate (global site index ((r*2 + h)*ram + j))"""
    out = []
    for r in range(nrep):
        hs = []
        for h in range(2):
            a = supplied[r, h] if supplied is not None else oracle.simulate(om, seed, (r * 2 + h) * ram, ram)[0]
            hs.append(oracle.map_sites(om, a)["counts"])
        out.append(hs)
    return out


def _null_degenerate(vecs):
    return np.concatenate([_degenerate(v0) | _degenerate(v1) for v0, v1 in vecs])


# ------------------------------------------------------------------------------------------------ every shape, every model
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_mapping_null_and_table_walk(shape, model):
    """one Engine; the branch-length variant rotates over shapes and models so that every variant meets every size"""
    idx = SHAPES.index(shape) + MODELS.index(model)
    eng, om, blen, S, kind = _pair(shape, model, idx)
    aln = _alignment(om, S, shape.ntaxa, 100 + idx)
    _check_map(eng.map_sites(aln), oracle.map_sites(om, aln))
    # the fused null: 3 replicates of 33 sites
    nrep, ram, seed = 3, 33, 7 + idx
    g, o = eng.null_intra(kind, seed, 0, nrep, ram), oracle.null_intra(om, kind, seed, 0, nrep, ram)
    deg = _null_degenerate(_null_vectors(om, seed, nrep, ram)) if kind == engine.STAT_CORRELATION else np.zeros(nrep * ram, bool)
    _stat_close(g["stat"], o["stat"], deg)
    rel_close(g["nmin"], o["nmin"], 1e-6)
    rel_close(g["prmin"], o["prmin"], 1e-9)
    assert np.array_equal(g["rcmin"], o["rcmin"])
    if S == 4:
        # the cherry-table walk (null kernel on supplied alignments) against the generic walk (observed kernel) at 1e-11
        nrep, ram = 2, 29
        sup = np.stack([np.stack([eng.simulate(5 + idx, (r * 2 + h) * ram, ram)[0] for h in range(2)]) for r in range(nrep)])
        nl = eng.null_intra(kind, 0, 0, nrep, ram, supplied=sup)
        for r in range(nrep):
            m0, m1 = eng.map_sites(sup[r, 0]), eng.map_sites(sup[r, 1])
            sl = slice(r * ram, (r + 1) * ram)
            rel_close(nl["nmin"][sl], np.minimum(m0["norm"], m1["norm"]), 1e-11, 1e-300)
            rel_close(nl["prmin"][sl], np.minimum(m0["post_rate"], m1["post_rate"]), 1e-12)
            assert np.array_equal(nl["rcmin"][sl], np.minimum(m0["rate_class"], m1["rate_class"]))
            st = np.array([oracle.stat_pair(kind, m0["counts"][j], m1["counts"][j]) for j in range(ram)])
            d = _degenerate(m0["counts"]) | _degenerate(m1["counts"]) if kind == engine.STAT_CORRELATION else np.zeros(ram, bool)
            _stat_close(nl["stat"][sl], st, d, 1e-8, 1e-11)
    eng.synchronize()


def test_the_root_child_cherry_shapes_take_the_table_walk():
    """((x,x),x) and (x,(x,x)): the root's child is an inlined cherry, first or second"""
    for name in ("((x,x),x)", "(x,(x,x))"):
        eng, _, _, _, _ = _pair(by_name(name, SHAPES), "dna_g4", "b0.1")
        info = eng.info()
        assert info["cherry_tables"] == 1 and info["device_states"] == 16


# ------------------------------------------------------------------------------------------------ 2, 3 and 4 leaves
SMALL = ["(x,x)", "((x,x),x)", "(x,x,x)", "((x,x),(x,x))", "(((x,x),x),x)"]


@pytest.mark.parametrize("name", SMALL)
def test_unfused_null_mi_bounds(name):
    """the bounds statistic takes null_unfused_dev (simulate -> map -> diagonal pairs)"""
    eng, om, _, _, _ = _pair(by_name(name, SHAPES), "dna_g4", "sat5")
    bounds = np.array([-0.5, 0.02, 0.1, 0.3, 1.0, 1e4])
    g = eng.null_intra(engine.STAT_DISCRETE_MI_BOUNDS, 31, 0, 3, 37, threshold=bounds)
    o = oracle.null_intra(om, oracle.ST_DISCRETE_MI, 31, 0, 3, 37, params=np.concatenate([[len(bounds)], bounds]))
    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
    rel_close(g["nmin"], o["nmin"], 1e-6)
    assert np.array_equal(g["rcmin"], o["rcmin"])
    eng.synchronize()


@pytest.mark.parametrize("name,model", [("(x,x)", "protein_g4"), ("(x,x,x)", "dna_g4"), ("((x,x),x)", "dna_5cls"),
                                        ("((x,x),(x,x))", "dna_g4")])
def test_continuous_rate_null(name, model):
    """the continuous-rate null against the oracle's null on the engine's own continuous-rate alignments (the simulator
    itself is compared in test_gpu_parity)"""
    shape = by_name(name, SHAPES)
    eng, om, _, _, kind = _pair(shape, model, "leaf0")
    nrep, ram, seed = 3, 31, 8
    g = eng.null_intra_continuous(kind, seed, 0, nrep, ram, 0.6)
    aln, _ = eng.simulate_continuous(seed, 0, nrep * 2 * ram, 0.6)
    sup = np.ascontiguousarray(aln.reshape(shape.ntaxa, nrep, 2, ram).transpose(1, 2, 0, 3))
    o = oracle.null_intra(om, kind, 0, 0, nrep, ram, supplied=sup)
    _stat_close(g["stat"], o["stat"], _null_degenerate(_null_vectors(om, 0, nrep, ram, sup)))
    rel_close(g["nmin"], o["nmin"], 1e-6)
    assert np.array_equal(g["rcmin"], o["rcmin"])


@pytest.mark.parametrize("name", ["(x,x)", "(x,(x,x))", "(x,x,x)", "((x,x),(x,x))", "((x,x),x,x)"])
@pytest.mark.parametrize("average,joint", [(False, True), (True, False), (False, False)])
def test_mapping_variant_nulls(name, average, joint):
    """nijt.average / joint = no: the null is simulate -> map with the variant -> score site j against site j, rebuilt from
    the oracle's simulator, the oracle's variant mapping and its statistic.  Sites whose arg-max (ancestral pair or
    marginal state) is a tie within 1e-9 may be decided either way by rounding and are left out."""
    shape = by_name(name, SHAPES)
    eng, om, _, _, _ = _pair(shape, "dna_g4", "sat5")
    eng.set_mapping_options(average, joint)
    nrep, ram, seed = 3, 33, 21
    g = eng.null_intra(engine.STAT_CORRELATION, seed, 0, nrep, ram)
    want, clear, deg = [], [], []
    for r in range(nrep):
        ms = []
        for h in range(2):
            a, _ = oracle.simulate(om, seed, (r * 2 + h) * ram, ram)
            m = oracle.map_sites_noavg(om, a) if joint else oracle.map_sites_marginal(om, a, average)
            ms.append(m)
        want.append([oracle.stat_pair(0, ms[0]["counts"][j], ms[1]["counts"][j]) for j in range(ram)])
        ok = np.ones(ram, bool)
        if not average:
            for m in ms:
                ok &= (m["margin"] > 1e-9).all(axis=1)
        clear.append(ok)
        deg.append(_degenerate(ms[0]["counts"]) | _degenerate(ms[1]["counts"]))
    want, clear, deg = np.concatenate(want), np.concatenate(clear), np.concatenate(deg)
    assert clear.mean() > 0.5
    _stat_close(g["stat"][clear], want[clear], deg[clear])
    eng.set_mapping_options(True, True)
    g2, o2 = eng.null_intra(0, seed, 0, nrep, ram), oracle.null_intra(om, 0, seed, 0, nrep, ram)
    _stat_close(g2["stat"], o2["stat"], _null_degenerate(_null_vectors(om, seed, nrep, ram)))


@pytest.mark.parametrize("name", ["(x,x)", "(x,x,x)", "((x,x),x)", "((x,x),(x,x))", "((x,x,x),x)"])
def test_intra_rows_with_pvalues(name):
    shape = by_name(name, SHAPES)
    eng, om, _, S, _ = _pair(shape, "protein_g4", "b0.1")
    aln = _alignment(om, S, shape.ntaxa, 55)
    n = aln.shape[1]
    m, mo = eng.map_sites(aln), oracle.map_sites(om, aln)
    nl = eng.null_intra(0, 3, 0, 5, 41)
    st = eng.pair_stats(0, m["counts"])
    deg = _degenerate(mo["counts"])
    iu = np.triu_indices(n, 1)
    _stat_close(st[iu], oracle.pair_stats_intra(0, mo["counts"])[iu], (deg[:, None] | deg[None, :])[iu])
    rows, total = eng.intra_rows(0, m["counts"], m["rate_class"], m["post_rate"], m["norm"], nl["stat"], nl["nmin"], 4)
    assert total == len(rows) == n * (n - 1) // 2
    assert np.array_equal(rows["i"], iu[0]) and np.array_equal(rows["j"], iu[1])
    assert np.array_equal(rows["stat"], st[iu], equal_nan=True)
    pv, ns = oracle.intra_pvalues(st, m["norm"], 4, nl["stat"], nl["nmin"])
    assert np.array_equal(rows["nsim"], ns[iu])
    assert np.array_equal(rows["pvalue"], pv[iu], equal_nan=True)
    assert np.array_equal(rows["rc_min"], np.minimum(m["rate_class"][iu[0]], m["rate_class"][iu[1]]))
    rel_close(rows["n_min"], np.minimum(mo["norm"][iu[0]], mo["norm"][iu[1]]), 1e-6)


# ------------------------------------------------------------------------------------------------ B = 2, 3, 4 branches
@pytest.mark.parametrize("name,B", [("(x,x)", 2), ("(x,x,x)", 3), ("((x,x),x)", 4)])
@pytest.mark.parametrize("kind", range(8))
def test_pair_stats_at_two_to_four_branches(name, B, kind):
    """B < 4: the Gram kernel's operand has Bp = 4 rows, the last 4 - B of them padding.  Vectors: random (K = 1 and 2),
    and the tree's own mapped ones (where the correlation of (x,x) is degenerate)"""
    shape = by_name(name, SHAPES)
    assert shape.nn - 1 == B
    rng = np.random.default_rng(B * 10 + kind)
    for model in ("protein_g4", "dna_2types"):
        eng, om, _, S, _ = _pair(shape, model, "b0.1")
        K = eng.K
        c = rng.exponential(0.3, size=(70, B, K))
        c[5] = c[4] * 2.0                                        # proportional vectors: correlation exactly 1
        c[6, :, 0] = 0.25                                        # a constant vector: its centred vector is 0
        if kind in (2, 5):
            c = c * 4.0                                          # ">= 1" / ">= 0.99" events
        aln = _alignment(om, S, shape.ntaxa, 9)
        mapped = oracle.map_sites(om, aln)["counts"]
        for counts in (c, mapped):
            kw, p1, p2 = {}, None, None
            if kind == engine.STAT_CORRECTED_CORRELATION:
                mv, mv2 = counts[:, :, 0].mean(axis=0), counts[:, :, 0].mean(axis=0) * 0.5 + 0.01
                kw = dict(mean_vectors=mv)
                p1, p2 = np.concatenate([mv, mv]), np.concatenate([mv, mv2])
            deg = _degenerate(counts) if kind in (0, 4) else np.zeros(len(counts), bool)
            g = eng.pair_stats(kind, counts, **kw)
            o = oracle.pair_stats_intra(kind, counts, p1)
            iu = np.triu_indices(len(counts), 1)
            _stat_close(g[iu], o[iu], (deg[:, None] | deg[None, :])[iu]) if kind == 0 else rel_close(g[iu], o[iu], 1e-6, 1e-12)
            h = len(counts) // 2
            if kind == engine.STAT_CORRECTED_CORRELATION:
                kw = dict(mean_vectors=np.stack([mv, mv2]))
            gi = eng.pair_stats(kind, counts[:h], counts[h:], **kw)
            oi = oracle.pair_stats_inter(kind, counts[:h], counts[h:], p2)
            _stat_close(gi, oi, deg[:h, None] | deg[None, h:]) if kind == 0 else rel_close(gi, oi, 1e-6, 1e-12)
        eng.synchronize()
