"""Per-branch weights of the statistics on the device (cmx_set_statistic_weights, DESIGN.md A.7, weighted) against the numpy
restatement of tests/weighted_reference.py, through every entry point that scores substitution vectors; the kinds that
ignore weights and every unweighted call stay bit for bit what they were."""
import numpy as np
import pytest
import torch

import weighted_reference as wr
from comap_amd import engine
from conftest import make_case
from oracle import cluster as oc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-11, 1e-13
WEIGHTED = [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_COSINUS, engine.STAT_COVARIANCE,
            engine.STAT_CORRECTED_CORRELATION, engine.STAT_EUCLIDIAN_DISTANCE]


def _engine(case):
    return engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])


def _weights(B, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.2, 3.0, size=B)
    w[rng.choice(B, size=max(1, B // 5), replace=False)] = 0.0
    return w


@pytest.fixture(scope="module", params=[20, 4], ids=["protein", "dna"])
def setup(request):
    S = request.param
    case = make_case(11, 90, S, 70 + S)
    eng = _engine(case)
    m = eng.map_sites(case["aln"])
    w = _weights(eng.B, S)
    yield dict(case=case, eng=eng, m=m, counts=m["counts"], w=w, wn=wr.normalise(w))
    eng.set_statistic_weights(None)


def _mv(kind, counts):
    if kind != engine.STAT_CORRECTED_CORRELATION:
        return None
    mv = counts.sum(2).mean(0)
    return np.stack([mv, 0.5 * mv])


def _close(got, ref):
    ok, worst = wr.close(got, ref, RTOL, ATOL)
    assert ok, worst


def _check_same(a, b):
    assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------------------------------------ pair statistics
@pytest.mark.parametrize("kind", WEIGHTED)
def test_pair_stats_intra_and_inter_match_the_restatement(setup, kind):
    eng, c, wn = setup["eng"], setup["counts"], setup["wn"]
    mv = _mv(kind, c)
    eng.set_statistic_weights(setup["w"])
    got = eng.pair_stats(kind, c, mean_vectors=mv)
    _close(got, wr.matrix_gram(kind, c, wn, mv=mv))
    c1, c2 = c[:37], c[37:]
    got = eng.pair_stats(kind, c1, c2, mean_vectors=mv)
    _close(got, wr.matrix_gram(kind, c1, wn, c2, mv=mv))
    eng.set_statistic_weights(None)


def test_constant_sites_give_nan_like_the_restatement(setup):
    eng, wn = setup["eng"], setup["wn"]
    c = setup["counts"][:20].copy()
    c[[3, 11], :, 0] = 0.0
    eng.set_statistic_weights(setup["w"])
    for kind in (engine.STAT_CORRELATION, engine.STAT_COSINUS):
        got = eng.pair_stats(kind, c)
        assert np.isnan(got[3, 11]) and np.isnan(got[3, 4])
        _close(got, wr.matrix_gram(kind, c, wn))
    eng.set_statistic_weights(None)


def test_stored_weights_are_normalised(setup):
    eng = setup["eng"]
    assert eng.statistic_weights() is None
    eng.set_statistic_weights(setup["w"])
    assert np.array_equal(eng.statistic_weights(), setup["wn"])
    eng.set_statistic_weights(None)
    assert eng.statistic_weights() is None


@pytest.mark.parametrize("kind", [engine.STAT_COSUBSTITUTION, engine.STAT_DISCRETE_MI, engine.STAT_DISCRETE_MI_BOUNDS])
def test_ignoring_kinds_are_bit_identical(setup, kind):
    eng, c = setup["eng"], setup["counts"]
    thr = np.array([0.0, 0.5, 1.0, 2.0, 1e4]) if kind == engine.STAT_DISCRETE_MI_BOUNDS else 0.99
    a = eng.pair_stats(kind, c, threshold=thr)
    eng.set_statistic_weights(setup["w"])
    b = eng.pair_stats(kind, c, threshold=thr)
    g = eng.group_stats(kind, c, [[0, 1, 2], [5, 9]], threshold=thr)
    eng.set_statistic_weights(None)
    _check_same(a, b)
    _check_same(g, eng.group_stats(kind, c, [[0, 1, 2], [5, 9]], threshold=thr))


# ------------------------------------------------------------------------------------------------ rows and records
def _dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)


@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_COVARIANCE])
def test_rows_and_records_equal_the_dense_weighted_statistic(setup, kind):
    eng, m, c = setup["eng"], setup["m"], setup["counts"]
    n, ncls = c.shape[0], 4
    eng.set_statistic_weights(setup["w"])
    nl = eng.null_intra(kind, 77, 0, 3, 40)
    st = eng.pair_stats(kind, c)
    pv, ns = eng.intra_pvalues(st, m["norm"], ncls, nl["stat"], nl["nmin"])
    iu = np.triu_indices(n, 1)
    d_counts = _dev(c.reshape(n, -1).T)
    d_norm, d_rc, d_pr = _dev(m["norm"]), _dev(m["rate_class"], torch.int32), _dev(m["post_rate"])
    d_ns, d_nm = _dev(nl["stat"]), _dev(nl["nmin"])
    npairs = n * (n - 1) // 2
    rows = torch.empty(npairs * engine.PAIR_ROW.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    eng.intra_rows_range_dev(kind, d_counts, d_rc, d_pr, d_norm, d_ns, d_nm, ncls, rows, count)
    comp = torch.empty(npairs * engine.PAIR_COMPACT.itemsize, dtype=torch.uint8, device="cuda")
    eng.intra_compact_range_dev(kind, d_counts, d_norm, d_ns, d_nm, ncls, comp)
    torch.cuda.synchronize()
    eng.set_statistic_weights(None)
    r = rows.cpu().numpy().view(engine.PAIR_ROW)
    assert int(count.item()) == npairs
    assert np.array_equal(r["i"], iu[0]) and np.array_equal(r["j"], iu[1])
    _check_same(r["stat"], st[iu])
    _check_same(r["pvalue"], pv[iu])
    assert np.array_equal(r["nsim"], ns[iu])
    x = engine.expand_compact_rows(n, 0, n, m["rate_class"], m["post_rate"], m["norm"], comp.cpu().numpy())
    _check_same(x["stat"], st[iu])
    _check_same(x["pvalue"], pv[iu])
    _close(st, wr.matrix_gram(kind, c, setup["wn"]))


def test_kept_gram_blocks_follow_new_weights(setup):
    eng, m, c = setup["eng"], setup["m"], setup["counts"]
    n, kind = c.shape[0], engine.STAT_CORRELATION
    d_counts, d_norm = _dev(c.reshape(n, -1).T), _dev(m["norm"])
    npairs = n * (n - 1) // 2

    def compact(prefetch_first, w_before, w_after):
        eng.set_statistic_weights(w_before)
        if prefetch_first:
            eng.intra_gram_prefetch_dev(kind, d_counts, n)
        if w_after is not w_before:       # (setting the same weights again would discard the kept blocks too)
            eng.set_statistic_weights(w_after)
        out = torch.empty(npairs * engine.PAIR_COMPACT.itemsize, dtype=torch.uint8, device="cuda")
        eng.intra_compact_range_dev(kind, d_counts, d_norm, None, None, 4, out)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(engine.PAIR_COMPACT)["stat"].copy()

    w2 = _weights(eng.B, 99)
    fresh = compact(False, w2, w2)
    _check_same(compact(True, None, w2), fresh)               # kept unweighted blocks, then weights set
    _check_same(compact(True, setup["w"], w2), fresh)         # kept blocks of other weights
    _check_same(compact(True, w2, w2), fresh)                 # kept blocks of these weights are used
    unw = compact(False, None, None)
    _check_same(compact(True, w2, None), unw)                 # kept weighted blocks, then weights cleared
    iu = np.triu_indices(n, 1)
    _close(fresh, wr.matrix_gram(kind, c, wr.normalise(w2))[iu])
    eng.set_statistic_weights(None)


@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_COSINUS])
def test_inter_rows_carry_the_weighted_statistic(setup, kind):
    """cmx_inter_rows with weights set, both of its ways to the statistic: the row blocks of the Gram (70 x 33 sites: one
    full 64-column step and a tail) and, for independant comparisons, the diagonal pairs scored lane by lane.  No filter
    drops a pair, so the rows are every pair in (i, j) order with the restatement's value."""
    eng, m, wn = setup["eng"], setup["m"], setup["wn"]

    def part(lo, hi):
        return {k: m[k][lo:hi] for k in ("counts", "rate_class", "post_rate", "norm")}

    eng.set_statistic_weights(setup["w"])
    a, b = part(0, 70), part(57, 90)
    rows, count = eng.inter_rows(kind, a, b)
    d1, d2 = part(0, 45), part(45, 90)
    diag, ndiag = eng.inter_rows(kind, d1, d2, engine.InterFilters(independent_comparisons=True))
    eng.set_statistic_weights(None)
    assert count == len(rows) == 70 * 33
    assert np.array_equal(rows["i"], np.repeat(np.arange(70), 33)) and np.array_equal(rows["j"], np.tile(np.arange(33), 70))
    _close(rows["stat"].reshape(70, 33), wr.matrix_gram(kind, a["counts"], wn, b["counts"]))
    assert np.array_equal(rows["n_min"], np.minimum.outer(a["norm"], b["norm"]).ravel())
    assert ndiag == len(diag) == 45
    assert np.array_equal(diag["i"], np.arange(45)) and np.array_equal(diag["j"], np.arange(45))
    _close(diag["stat"], np.diag(wr.matrix_gram(kind, d1["counts"], wn, d2["counts"])))
    assert np.array_equal(diag["rc_min"], np.minimum(d1["rate_class"], d2["rate_class"]))


# ------------------------------------------------------------------------------------------------ groups, clustering
@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_COSINUS, engine.STAT_COVARIANCE])
def test_group_stats_match_the_restatement(setup, kind):
    eng, c, wn = setup["eng"], setup["counts"], setup["wn"]
    groups = [[0, 1], [2, 3, 4], [10, 20, 30, 40, 50], list(range(60, 75))]
    eng.set_statistic_weights(setup["w"])
    got = eng.group_stats(kind, c, groups)
    eng.set_statistic_weights(None)
    _close(got, np.array([wr.group_brute(kind, c, g, wn) for g in groups]))


@pytest.mark.parametrize("dist", [oc.DIST_CORRELATION, oc.DIST_COMPENSATION, oc.DIST_EUCLIDIAN])
def test_cluster_sites_use_the_weighted_distance(setup, dist):
    eng, c, wn = setup["eng"], setup["counts"], setup["wn"]
    kind = {oc.DIST_CORRELATION: wr.CORRELATION, oc.DIST_COMPENSATION: wr.COMPENSATION, oc.DIST_EUCLIDIAN: wr.EUCLIDIAN}[dist]
    # one site per distinct alignment column: duplicated columns tie at distance ~0, where the last bit decides the joins
    _, first = np.unique(setup["case"]["aln"], axis=1, return_index=True)
    c = c[np.sort(first)]
    eng.set_statistic_weights(setup["w"])
    g = eng.cluster_sites(dist, oc.LINK_AVERAGE, c)
    eng.set_statistic_weights(None)
    s = wr.matrix_gram(kind, c, wn)
    iu = np.triu_indices(len(c), 1)
    ref = np.zeros_like(s)
    ref[iu] = s[iu] if kind == wr.EUCLIDIAN else 1.0 - s[iu]
    ref = ref + ref.T
    _close(g["dist"], ref)
    # the merges are oracle/cluster.py's on these distances, bit for bit; on the restated matrix (which differs in the last
    # bits) the join heights agree
    merge, dmax, size = oc.hclust(g["dist"], oc.LINK_AVERAGE)
    assert np.array_equal(g["merge"], merge) and np.array_equal(g["size"], size) and np.array_equal(g["dmax"], dmax)
    assert np.allclose(np.sort(g["dmax"]), np.sort(oc.hclust(ref, oc.LINK_AVERAGE)[1]), rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ nulls
@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_COSINUS])
def test_null_intra_scores_supplied_alignments_with_the_weights(setup, kind):
    eng, case, wn = setup["eng"], setup["case"], setup["wn"]
    nrep, rr = 3, 40
    aln, _ = eng.simulate(5, 0, nrep * 2 * rr)
    sup = np.ascontiguousarray(aln.reshape(eng.T, nrep, 2, rr).transpose(1, 2, 0, 3))
    eng.set_statistic_weights(setup["w"])
    nl = eng.null_intra(kind, 5, 0, nrep, rr, supplied=sup)
    eng.set_statistic_weights(None)
    exp = []
    for r in range(nrep):
        a = eng.map_sites(sup[r, 0])["counts"]
        b = eng.map_sites(sup[r, 1])["counts"]
        exp.append(np.diag(wr.matrix_gram(kind, a, wn, b)))
    _close(nl["stat"], np.concatenate(exp))


def test_null_intra_replicate_ranges_concatenate(setup):
    eng = setup["eng"]
    eng.set_statistic_weights(setup["w"])
    one = eng.null_intra(engine.STAT_CORRELATION, 31, 0, 5, 30)
    a = eng.null_intra(engine.STAT_CORRELATION, 31, 0, 2, 30)
    b = eng.null_intra(engine.STAT_CORRELATION, 31, 2, 5, 30)
    eng.set_statistic_weights(None)
    for k in ("stat", "nmin", "prmin", "rcmin"):
        _check_same(one[k], np.concatenate([a[k], b[k]]))
    # the continuous-rate null runs through the same weighted path
    eng.set_statistic_weights(setup["w"])
    cont = eng.null_intra_continuous(engine.STAT_CORRELATION, 31, 0, 2, 30, 0.8)
    via = eng.null_intra_continuous_via_host(engine.STAT_CORRELATION, 31, 0, 2, 30, 0.8)
    eng.set_statistic_weights(None)
    _check_same(cont["stat"], via["stat"])


def test_null_inter_uses_the_first_contexts_weights(setup):
    case = setup["case"]
    e1, e2 = _engine(case), _engine(case)
    kind, w = engine.STAT_CORRELATION, setup["w"]
    plain = e1.null_inter(e2, kind, 9, 0, 2, 50)
    e1.set_statistic_weights(w)
    only1 = e1.null_inter(e2, kind, 9, 0, 2, 50)
    e2.set_statistic_weights(w)
    both = e1.null_inter(e2, kind, 9, 0, 2, 50)
    e1.set_statistic_weights(None)
    only2 = e1.null_inter(e2, kind, 9, 0, 2, 50)
    _check_same(only1["stat"], both["stat"])
    _check_same(only2["stat"], plain["stat"])
    assert not np.array_equal(only1["stat"], plain["stat"])
    # and it is the weighted statistic of the two sides' mapped replicates
    sup = [e1.simulate(9, ((r * 2 + h) * 50), 50)[0] for r in range(2) for h in range(2)]
    exp = np.concatenate([np.diag(wr.matrix_gram(kind, e1.map_sites(sup[2 * r])["counts"], setup["wn"],
                                                 e2.map_sites(sup[2 * r + 1])["counts"])) for r in range(2)])
    _close(only1["stat"], exp)


# ------------------------------------------------------------------------------------------------ unweighted unchanged
def test_every_entry_point_is_unchanged_after_set_then_clear(setup):
    case, c, m = setup["case"], setup["counts"], setup["m"]

    def run(eng):
        out = {}
        for kind in WEIGHTED + [engine.STAT_COSUBSTITUTION, engine.STAT_DISCRETE_MI]:
            out[f"pair{kind}"] = eng.pair_stats(kind, c, mean_vectors=_mv(kind, c))
            out[f"inter{kind}"] = eng.pair_stats(kind, c[:30], c[30:], mean_vectors=_mv(kind, c))
        for kind in (engine.STAT_CORRELATION, engine.STAT_COMPENSATION):
            nl = eng.null_intra(kind, 3, 0, 2, 40)
            out[f"null{kind}"] = nl["stat"]
            rows, _ = eng.intra_rows(kind, c, m["rate_class"], m["post_rate"], m["norm"], nl["stat"], nl["nmin"], nclasses=4)
            out[f"rows{kind}"] = rows.tobytes()
            out[f"group{kind}"] = eng.group_stats(kind, c, [[0, 1, 2], [4, 8, 9, 30]])
            out[f"irows{kind}"] = eng.inter_rows(kind, m, m)[0].tobytes()
        for dist in (oc.DIST_CORRELATION, oc.DIST_COMPENSATION, oc.DIST_EUCLIDIAN):
            g = eng.cluster_sites(dist, oc.LINK_COMPLETE, c)
            out[f"cl{dist}"] = (g["dist"], g["merge"], g["stat"])
        return out

    fresh = run(_engine(case))
    e = _engine(case)
    e.set_statistic_weights(setup["w"])
    e.set_statistic_weights(None)
    again = run(e)
    for k in fresh:
        a, b = fresh[k], again[k]
        if isinstance(a, tuple):
            for x, y in zip(a, b):
                _check_same(x, y)
        elif isinstance(a, bytes):
            assert a == b, k
        else:
            _check_same(a, b)


# ------------------------------------------------------------------------------------------------ errors
def test_bad_weights_fail_with_a_named_status_and_leave_the_context_usable(setup):
    eng, c = setup["eng"], setup["counts"][:20]
    eng.set_statistic_weights(setup["w"])
    before = eng.pair_stats(engine.STAT_CORRELATION, c)
    B = eng.B
    cases = [(np.ones(B + 1), -1, "branches"), (np.ones(B - 1), -1, "branches"),
             (np.where(np.arange(B) == 2, np.nan, 1.0), -1, "not finite"), (np.zeros(B), -1, "sum"),
             (np.where(np.arange(B) == 1, -0.5, 1.0), -2, "negative")]
    for w, status, words in cases:
        with pytest.raises(engine.CmxError) as e:
            eng.set_statistic_weights(w)
        assert e.value.status == status and words in str(e.value), str(e.value)
        assert np.array_equal(eng.statistic_weights(), setup["wn"])           # the previous weights are kept
    _check_same(eng.pair_stats(engine.STAT_CORRELATION, c), before)
    eng.set_statistic_weights(None)


def test_intra_analysis_passes_the_weights_through(setup):
    from comap_amd.pipeline import IntraAnalysis
    eng, case = setup["eng"], setup["case"]
    ana = IntraAnalysis(eng, torch.from_numpy(np.ascontiguousarray(case["aln"])).cuda(), "Correlation", weights=setup["w"])
    assert np.array_equal(eng.statistic_weights(), setup["wn"])
    ana.get_vectors()
    stat, _, _ = ana.compute_intra_stats()
    torch.cuda.synchronize()
    eng.set_statistic_weights(None)
    _close(stat.cpu().numpy(), wr.matrix_gram(wr.CORRELATION, setup["counts"], setup["wn"]))
