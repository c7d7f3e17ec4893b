"""The sliding-window conditional p-values on the device (cmx_window_*, cmx_intra_window_range_dev) against the
brute-force restatement of R/CoMapFunctions.R:168-215 in tests/window_reference.py.

count and nobs are integers and must be equal; p is one IEEE division of two exactly representable integers on either side and
must be equal too, NaN where the reference has NaN."""
import numpy as np
import pytest
import torch

from comap_amd import engine
from comap_amd.pipeline import IntraAnalysis, sum_pairs
from conftest import make_case
from window_reference import window_half_width, window_test

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return engine.Engine()      # the window calls need no tree and no model


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _build(eng, ns, nm, window):
    if len(ns) == 0:
        eng.window_null_dev(None, None, window)
    else:
        eng.window_null_dev(_dev(ns), _dev(nm), window)


def _query(eng, s, m, **kw):
    nq = len(s)
    pv = torch.full((nq,), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    nobs = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    eng.window_test_dev(_dev(s), _dev(m), pv, cnt, nobs, **kw)
    torch.cuda.synchronize()
    return pv.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), nobs.cpu().numpy().view(np.uint32)


def _same(got, ref, what=""):
    (pv, cnt, nobs), (rpv, rcnt, rnobs) = got, ref
    assert np.array_equal(nobs, rnobs), f"nobs {what}: {np.flatnonzero(nobs != rnobs)[:5]}"
    assert np.array_equal(cnt, rcnt), f"count {what}: {np.flatnonzero(cnt != rcnt)[:5]}"
    assert np.array_equal(np.isnan(pv), np.isnan(rpv)), f"NaN positions {what}"
    assert np.array_equal(pv, rpv, equal_nan=True), f"p {what}"


def _check(eng, ns, nm, s, m, window, what="", **kw):
    _build(eng, ns, nm, window)
    ref = window_test(ns, nm, s, m, window, **kw)
    _same(_query(eng, s, m, **kw), ref, what)
    return ref


@pytest.mark.parametrize("nnull", [1, 2, 31, 32, 33, 63, 64, 65, 1000, 4099])
def test_index_sizes_around_the_word_and_unit_edges(eng, nnull):
    rng = np.random.default_rng(nnull)
    ns, nm = rng.normal(size=nnull), rng.gamma(2.0, 1.5, size=nnull)
    pad = 0.1 * (nm.max() - nm.min())
    s, m = rng.normal(size=257), rng.uniform(nm.min() - pad, nm.max() + pad, size=257)
    s[:20], m[:20] = ns[rng.integers(0, nnull, 20)], nm[rng.integers(0, nnull, 20)]     # queries that are null values
    for window in (0.02, 0.2, 1.0, 2.5):
        _build(eng, ns, nm, window)
        info = eng.window_null_info()
        assert info["nkept"] == nnull and info["ws"] == window_half_width(ns, nm, window)[1]
        assert (info["nmin_min"], info["nmin_max"]) == (nm.min(), nm.max())
        for lower in (False, True):
            ref = window_test(ns, nm, s, m, window, min_nobs=2, lower=lower)
            _same(_query(eng, s, m, min_nobs=2, lower=lower), ref, f"window {window} lower {lower}")
        if window == 2.5:      # ws = 1.25 ranges: every query within a tenth of the range of its ends sees every entry
            assert (ref[2] == (nnull if nnull > 1 else 0)).all()


@pytest.mark.parametrize("lower", [False, True])
def test_ties_in_the_statistic(eng, lower):
    rng = np.random.default_rng(5)
    ns, nm = rng.integers(0, 4, size=700).astype(np.float64), rng.uniform(0, 3, size=700)      # as Cosubstitution yields
    s, m = rng.integers(-1, 6, size=257).astype(np.float64), rng.uniform(0, 3, size=257)
    _check(eng, ns, nm, s, m, 0.3, "four values", lower=lower)
    ref = _check(eng, np.full(100, 2.0), nm[:100], s, m, 0.5, "one value", lower=lower)
    hit = (s == 2.0) & (ref[2] > 0)
    assert hit.any() and (ref[1][hit] == ref[2][hit]).all()        # >= and <= both count every tied entry


def test_strict_window_edges_on_a_dyadic_grid(eng):
    """null nmins k / 8 over [0, 4], some twice; window 0.25: ws = 4 * 0.25 / 2 = 0.5 exactly, so m - ws and m + ws of a query on
    the grid are null values and neither may be counted"""
    rng = np.random.default_rng(8)
    nm = np.concatenate([np.arange(33) / 8.0, np.arange(0, 33, 3) / 8.0, [1.5, 1.5, 2.0]])
    ns = rng.normal(size=len(nm))
    assert window_half_width(ns, nm, 0.25)[1] == 0.5
    m = np.concatenate([np.arange(-8, 45) / 8.0, [1.0, 2.0, 2.5]])
    s = rng.normal(size=len(m))
    ref = _check(eng, ns, nm, s, m, 0.25, "grid")
    q = int(np.flatnonzero(m == 2.0)[0])       # (1.5, 2.5) strict: grid points 13 .. 19 once, the multiples of 3 (15, 18) and 2.0 again
    assert ref[2][q] == 7 + 2 + 1
    assert eng.window_null_info()["ws"] == 0.5


def test_empty_and_one_sided_windows(eng):
    rng = np.random.default_rng(2)
    ns, nm = rng.normal(size=300), rng.uniform(1.0, 2.0, size=300)
    m = np.array([-5.0, 0.5, 0.99, 1.0, 1.01, 1.99, 2.0, 2.01, 2.5, 9.0])
    ref = _check(eng, ns, nm, rng.normal(size=len(m)), m, 0.1, "outside the range", conserved_nmin=-10.0)
    assert ref[2][0] == 0 and ref[2][-1] == 0 and np.isnan(ref[0][0]) and ref[2][4] > 0
    for what, ens, enm in (("no entries", np.zeros(0), np.zeros(0)), ("all dropped", np.array([np.nan, 1.0, np.nan]), np.array([1.0, np.nan, np.nan]))):
        ref = _check(eng, ens, enm, np.array([0.1, 0.2, np.nan]), np.array([1.0, 0.001, 0.001]), 0.2, what)
        assert (ref[2] == 0).all() and np.isnan(ref[0][0]) and ref[0][1] == 1.0 and ref[0][2] == 1.0
        info = eng.window_null_info()
        assert info["nkept"] == 0 and info["ws"] == 0.0 and np.isnan(info["nmin_min"]) and np.isnan(info["nmin_max"])


def test_nan_in_the_null_and_in_the_queries(eng):
    rng = np.random.default_rng(3)
    ns, nm = rng.normal(size=500), rng.uniform(0, 4, size=500)
    ns[rng.integers(0, 500, 40)] = np.nan
    nm[rng.integers(0, 500, 40)] = np.nan
    nm[7], ns[7] = 100.0, np.nan            # a dropped entry must not stretch the range ws comes from
    s, m = rng.normal(size=257), rng.uniform(-0.5, 4.5, size=257)
    s[::9] = np.nan
    m[::7] = np.nan
    m[5], s[5] = 0.001, np.nan              # conserved and no statistic: the conserved rule comes first, p = 1
    m[9] = 2.0                              # no statistic alone: NaN
    ref = _check(eng, ns, nm, s, m, 0.2, "NaN")
    kept, ws = window_half_width(ns, nm, 0.2)
    info = eng.window_null_info()
    assert info["nkept"] == kept.sum() < 500 and info["ws"] == ws and info["nmin_max"] < 5.0
    assert ref[0][5] == 1.0 and np.isnan(ref[0][9]) and ref[2][0] == 0 and np.isnan(ref[0][0])


def test_min_nobs_boundary_and_the_conserved_rule(eng):
    rng = np.random.default_rng(4)
    ns, nm = rng.normal(size=400), rng.uniform(0, 2, size=400)
    s, m = np.array([0.1, 0.1, 0.1]), np.array([1.0, 1.0, 0.004])
    nobs = int(window_test(ns, nm, s, m, 0.1)[2][0])
    assert nobs > 3
    ref = _check(eng, ns, nm, s, m, 0.1, "nobs = min_nobs", min_nobs=nobs)
    assert not np.isnan(ref[0][0])
    ref = _check(eng, ns, nm, s, m, 0.1, "nobs = min_nobs - 1", min_nobs=nobs + 1)
    assert np.isnan(ref[0][0]) and ref[2][0] == nobs
    assert ref[0][2] == 1.0 and ref[2][2] < nobs + 1         # conserved with nobs < min_nobs: still 1
    ref = _check(eng, ns, nm, s, m, 0.1, "conserved_nmin", conserved_nmin=1.5)
    assert (ref[0] == 1.0).all()


def test_outputs_are_optional(eng):
    rng = np.random.default_rng(6)
    ns, nm, s, m = rng.normal(size=90), rng.uniform(0, 2, size=90), rng.normal(size=33), rng.uniform(0, 2, size=33)
    _build(eng, ns, nm, 0.4)
    ref = window_test(ns, nm, s, m, 0.4)
    nobs = torch.zeros(33, dtype=torch.int32, device="cuda")
    eng.window_test_dev(_dev(s), _dev(m), None, None, nobs)
    pv = torch.zeros(33, dtype=torch.float64, device="cuda")
    eng.window_test_dev(_dev(s), _dev(m), pv)
    torch.cuda.synchronize()
    assert np.array_equal(nobs.cpu().numpy().view(np.uint32), ref[2]) and np.array_equal(pv.cpu().numpy(), ref[0], equal_nan=True)


def test_errors_and_rebuilds():
    fresh = engine.Engine()
    one = _dev([1.0])
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    for call in (lambda: fresh.window_test_dev(one, one, out), fresh.window_null_info):
        with pytest.raises(engine.CmxError, match="no window index") as e:
            call()
        assert e.value.status == -1
    for bad in (0.0, -0.2, float("nan"), float("inf")):
        with pytest.raises(engine.CmxError, match="window") as e:
            fresh.window_null_dev(one, one, bad)
        assert e.value.status == -1
    with pytest.raises(engine.CmxError, match="no window index"):      # a refused build leaves no index behind
        fresh.window_test_dev(one, one, out)
    rng = np.random.default_rng(9)
    s, m = rng.normal(size=64), rng.uniform(0, 3, size=64)
    first = (rng.normal(size=2000), rng.uniform(0, 3, size=2000))
    second = (rng.normal(1.0, 1.0, size=150), rng.uniform(1, 2, size=150))
    a = _check(fresh, *first, s, m, 0.2, "first null")
    b = _check(fresh, *second, s, m, 0.5, "second null")        # smaller than the first: the buffers are the first one's
    assert not np.array_equal(a[2], b[2])
    fresh.close()


def test_host_entry_equals_the_device_sequence(eng):
    rng = np.random.default_rng(10)
    ns, nm = rng.normal(size=777), rng.uniform(0, 3, size=777)
    ns[3] = np.nan
    s, m = rng.normal(size=100), rng.uniform(-0.2, 3.2, size=100)
    for kw in (dict(window=0.2), dict(window=0.07, min_nobs=12, lower=True, conserved_nmin=0.3)):
        host = eng.window_test(ns, nm, s, m, **kw)
        _build(eng, ns, nm, kw["window"])
        q = {k: v for k, v in kw.items() if k != "window"}
        _same(host, _query(eng, s, m, **q), "host against device")
        _same(host, window_test(ns, nm, s, m, **kw), "host against the reference")
    pv, cnt, nobs = eng.window_test([], [], s, m)
    assert (nobs == 0).all() and (cnt == 0).all()
    assert len(eng.window_test(ns, nm, [], [])[0]) == 0


# ------------------------------------------------------------------------------------------------ the pair loop
N_SITES = 40


@pytest.fixture(scope="module")
def pair_case():
    case = make_case(8, N_SITES, 20, 77)
    e = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    return e, torch.from_numpy(case["aln"]).cuda()


@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COSUBSTITUTION])
def test_pair_loop_records(pair_case, kind):
    e, d_aln = pair_case
    n = N_SITES
    ana = IntraAnalysis(e, d_aln, kind)
    ana.get_vectors()
    nb = ana.null_distribution(11, 0, 3, 50)
    dense = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    e.pair_stats_dev(kind, ana.counts, dense)
    torch.cuda.synchronize()
    ns, nm, norm = nb["stat"].cpu().numpy().copy(), nb["nmin"].cpu().numpy().copy(), ana.norm.cpu().numpy()
    iu = np.triu_indices(n, 1)
    stat = dense.cpu().numpy()[iu]
    mmin = np.where(norm[iu[0]] < norm[iu[1]], norm[iu[0]], norm[iu[1]])
    assert len(ns) == 150

    def records(lower, window, rb=0, re_=n, prefetch=False):
        if prefetch:
            ana.prefetch_intra_gram(rb, re_)
        rec, npairs = ana.compute_intra_window(nb["stat"], nb["nmin"], window, lower, rb, re_)
        assert npairs == sum_pairs(n, rb, re_)
        return rec[:npairs * engine.PAIR_WINDOW.itemsize].cpu().numpy().view(engine.PAIR_WINDOW)

    for lower, window in ((False, 0.2), (True, 0.2), (False, 0.02), (False, 1.0)):
        rpv, rcnt, rnobs = window_test(ns, nm, stat, mmin, window, lower=lower)
        whole = records(lower, window)
        assert np.array_equal(whole["stat"], stat, equal_nan=True)
        assert np.array_equal(whole["nobs"], rnobs), (lower, window)
        assert np.array_equal(whole["count"], np.where(np.isnan(stat), 0xffffffff, rcnt)), (lower, window)
        for prefetch in (False, True):
            pieces = np.concatenate([records(lower, window, 0, 13, prefetch), records(lower, window, 13, n, prefetch)])
            assert pieces.tobytes() == whole.tobytes()
            assert records(lower, window, prefetch=prefetch).tobytes() == whole.tobytes()
        # the host-side p-values of the records == the array form's, for the reference's parameters and for others
        for kw in (dict(), dict(min_nobs=int(np.median(rnobs)) + 1, conserved_nmin=float(np.median(mmin)))):
            want = window_test(ns, nm, stat, mmin, window, lower=lower, **kw)[0]
            got = engine.window_pvalues_from_records(n, 0, n, norm, whole, **kw)
            assert np.array_equal(got, want, equal_nan=True)
            e.window_null_dev(nb["stat"], nb["nmin"], window)
            pv = torch.zeros(len(stat), dtype=torch.float64, device="cuda")
            e.window_test_dev(_dev(stat), _dev(mmin), pv, lower=lower, **kw)
            assert np.array_equal(pv.cpu().numpy(), got, equal_nan=True)
    part = engine.window_pvalues_from_records(n, 13, n, norm, whole[sum_pairs(n, 0, 13):])
    assert np.array_equal(part, engine.window_pvalues_from_records(n, 0, n, norm, whole)[sum_pairs(n, 0, 13):], equal_nan=True)
    with pytest.raises(engine.CmxError):
        engine.window_pvalues_from_records(n, 0, n, norm, whole[:-1])


def test_pair_loop_needs_an_index():
    case = make_case(8, 12, 20, 78)
    fresh = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    ana = IntraAnalysis(fresh, torch.from_numpy(case["aln"]).cuda(), engine.STAT_CORRELATION)
    ana.get_vectors()
    out = torch.zeros(sum_pairs(12, 0, 12) * 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(engine.CmxError, match="no window index") as err:
        fresh.intra_window_range_dev(engine.STAT_CORRELATION, ana.counts, ana.norm, out)
    assert err.value.status == -1
