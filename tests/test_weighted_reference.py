"""Per-branch weights of the statistics (weighted), CPU side: the pair-by-pair restatement in the reference's
order and the Gram form the device computes (tests/weighted_reference.py) agree, the uniform-weight identities hold,
and the library and the Python engine expose the weights entry points."""
import numpy as np
import pytest

import weighted_reference as wr
from comap_amd import engine

KINDS = {"cor": wr.CORRELATION, "comp": wr.COMPENSATION, "cos": wr.COSINUS, "cov": wr.COVARIANCE,
         "ccor": wr.CORRECTED_CORRELATION, "euclid": wr.EUCLIDIAN}


def _weights(rng, B, zeros=True):
    w = rng.uniform(0.1, 2.0, size=B)
    if zeros and B > 2:
        w[rng.choice(B, size=max(1, B // 4), replace=False)] = 0.0
    return wr.normalise(w)


def test_library_and_engine_expose_the_weights():
    lib = engine.load_library()
    assert hasattr(lib, "cmx_set_statistic_weights") and hasattr(lib, "cmx_get_statistic_weights")
    assert "cmx_set_statistic_weights" in engine.EXPORTS and "cmx_get_statistic_weights" in engine.EXPORTS
    assert callable(getattr(engine.Engine, "set_statistic_weights", None))
    assert callable(getattr(engine.Engine, "statistic_weights", None))


def test_header_documents_which_kinds_ignore_the_weights():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "comap_mi355x.h")).read()
    assert "cmx_set_statistic_weights(cmx_ctx* ctx, const double* w, size_t nbranches)" in hdr
    assert "cmx_get_statistic_weights(const cmx_ctx* ctx, double* w_out, int32_t* has_weights)" in hdr


@pytest.mark.parametrize("name", sorted(KINDS))
@pytest.mark.parametrize("B,K,n", [(1, 1, 6), (2, 1, 7), (3, 2, 8), (17, 1, 40), (17, 3, 25)])
def test_gram_form_equals_pair_by_pair(name, B, K, n):
    kind = KINDS[name]
    rng = np.random.default_rng(1000 * B + 10 * K + kind)
    c1 = wr.random_counts(rng, n, B, K, constant_sites=(1, 4))
    c2 = wr.random_counts(rng, n + 3, B, K, constant_sites=(0,))
    c1[2] = 0.0                                   # an all-zero site: cosinus / compensation NaN
    w = _weights(rng, B)
    mv = rng.uniform(0, 2, size=(2, B)) if kind == wr.CORRECTED_CORRELATION else None
    for other in (None, c2):
        brute = wr.matrix_brute(kind, c1, w, other, mv)
        gram = wr.matrix_gram(kind, c1, w, other, mv)
        ok, worst = wr.close(gram, brute, 1e-13, 1e-13)
        assert ok, (name, worst)


@pytest.mark.parametrize("name", ["cor", "cos", "comp", "cov", "euclid"])
def test_uniform_weights_identities(name):
    kind = KINDS[name]
    rng = np.random.default_rng(7 + kind)
    B = 13
    c = wr.random_counts(rng, 30, B, 2, constant_sites=(3,))
    w = wr.normalise(np.ones(B))
    got = wr.matrix_gram(kind, c, w)
    ref = wr.unweighted_brute(kind, c)
    if kind == wr.COVARIANCE:
        ref = ref * (B - 1) / B
    elif kind == wr.EUCLIDIAN:
        ref = ref / np.sqrt(B)
    ok, worst = wr.close(got, ref, 1e-12, 1e-13)
    assert ok, worst


def test_weights_are_scale_free_and_zero_weights_drop_branches():
    rng = np.random.default_rng(3)
    B = 9
    c = wr.random_counts(rng, 12, B, 1)
    w = rng.uniform(0.5, 1.5, size=B)
    w[[2, 5]] = 0.0
    keep = np.flatnonzero(w)
    for kind in (wr.CORRELATION, wr.COSINUS, wr.COMPENSATION):
        a = wr.matrix_brute(kind, c, wr.normalise(w))
        b = wr.matrix_brute(kind, c, wr.normalise(17.0 * w))
        d = wr.matrix_brute(kind, c[:, keep], wr.normalise(w[keep]))   # a zero weight == the branch left out
        assert wr.close(a, b, 1e-13, 1e-14)[0]
        assert wr.close(a, d, 1e-13, 1e-14)[0]


@pytest.mark.parametrize("name", ["cor", "comp", "cov", "cos"])
def test_group_restatement(name):
    kind = KINDS[name]
    rng = np.random.default_rng(11 + kind)
    B = 8
    c = wr.random_counts(rng, 20, B, 2, constant_sites=(5,))
    w = _weights(rng, B)
    for sites in ([0, 1], [2, 3, 4], [5, 6, 7, 8], [5, 9]):
        got = wr.group_brute(kind, c, sites, w)
        if kind == wr.COMPENSATION:
            # closed form: 1 - |sum of totals|_w / sum |totals|_w
            t = c[sites].sum(2)
            exp = 1 - np.sqrt((w * t.sum(0) ** 2).sum()) / np.sqrt((w * t ** 2).sum(1)).sum()
            if len(sites) == 2:   # the group of two is the pair
                assert abs(got - wr.pair_brute(kind, c[sites[0]], c[sites[1]], w)) < 1e-13
        else:
            vals = [wr.pair_brute(kind, c[i], c[j], w) for a, i in enumerate(sites) for j in sites[:a]]
            vals = [v for v in vals if not np.isnan(v)]
            exp = min(vals) if vals else np.inf
        assert abs(got - exp) <= 1e-13 * max(1.0, abs(exp)) or (np.isinf(got) and np.isinf(exp))
