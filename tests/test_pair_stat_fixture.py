"""The CPU restatements of the pair statistics (oracle.c, oracle/candidates.py, tests/weighted_reference.py) against the
definition-level fixture tests/golden/pair_stats.npz, within the bounds derived in tests/pair_stat_cases.py; and the
evidence that those bounds are neither too tight (headroom) nor so wide that they would hide a single-precision step
(sensitivity)."""
import importlib.util
import os
from functools import lru_cache

import numpy as np
import pytest

import oracle
import pair_stat_cases as pc
import weighted_reference as wr
from oracle import candidates

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "pair_stats.npz")


fixture = pc.fixture


def oracle_call(cs, key):
    """(oracle kind, params) of a statistic key"""
    if key in pc.MI_BOUNDS:
        b = pc.MI_BOUNDS[key]
        return oracle.ST_DISCRETE_MI, np.concatenate([[float(len(b))], b])
    if key == "k6":
        return oracle.ST_CORRECTED_CORRELATION, np.stack([cs.mv, cs.mv])
    return pc.kind_of(key), None


ORACLE_KEYS = [k for k in pc.UNWEIGHTED_KEYS if k != "sp"]


@lru_cache(maxsize=None)
def observed():
    """{(what, case, key): largest error / bound} over every CPU restatement"""
    fx, out = fixture(), {}
    for cs in pc.all_cases():
        ref, c = fx[cs.name], cs.counts
        big, idx = cs.expand(25, start=7)          # wraps the period: pairs (i, j) with i % 19 == j % 19 among them
        for key in ORACLE_KEYS:
            kind, params = oracle_call(cs, key)
            b = pc.pair_bounds(cs, key)
            got = np.array([[oracle.stat_pair(kind, c[i], c[j], params) for j in range(pc.NV)] for i in range(pc.NV)])
            out["stat_pair", cs.name, key] = pc.ratio(got, ref[key], b).max()
            got = oracle.pair_stats_intra(kind, big, params)
            assert np.isnan(got[np.tril_indices(25)]).all()
            iu = np.triu_indices(25, 1)
            out["intra", cs.name, key] = pc.ratio(got[iu], ref[key][np.ix_(idx, idx)][iu], pc.pair_bounds(cs, key, idx)[iu]).max()
            got = oracle.pair_stats_inter(kind, big[:9], big[9:], params)
            out["inter", cs.name, key] = pc.ratio(got, ref[key][np.ix_(idx[:9], idx[9:])], pc.pair_bounds(cs, key, idx[:9], idx[9:])).max()
            got = np.array([candidates.group_stat(kind, [c[s] for s in g], params) for g in pc.GROUPS])
            gb = np.array([pc.group_bound(cs, key, g, ref[key]) for g in pc.GROUPS])
            out["group_stat", cs.name, key] = pc.ratio(got, ref["g_" + key], gb).max()
        for key in pc.WEIGHTED_KEYS:
            kind = pc.kind_of(key)
            b = pc.pair_bounds(cs, key)
            got = np.array([[wr.pair_brute(kind, c[i], c[j], cs.w, cs.mv, cs.mv) for j in range(pc.NV)] for i in range(pc.NV)])
            out["pair_brute", cs.name, key] = pc.ratio(got, ref[key], b).max()
            if key != "w6":                        # group_brute carries no mean vector
                got = np.array([wr.group_brute(kind, c, g, cs.w) for g in pc.GROUPS])
                gb = np.array([pc.group_bound(cs, key, g, ref[key]) for g in pc.GROUPS])
                out["group_brute", cs.name, key] = pc.ratio(got, ref["g_" + key], gb).max()
    return out


def test_fixture_is_small_and_complete():
    assert os.path.getsize(FIXTURE) < 400 * 1024
    fx = fixture()
    assert sorted(fx) == sorted(pc.case_name(*c) for c in pc.CASES)
    for cs in pc.all_cases():
        assert cs.max_kappa() <= pc.KAPPA_MAX
        d = fx[cs.name]
        # the degenerate results the inputs were chosen for
        assert np.isnan(d["k0"][9]).all() and (d["k4"][9] == 0).all()            # constant vector
        assert np.isnan(d["k0"][8]).all() and np.isnan(d["k3"][8]).all() and np.isnan(d["k1"][8, 8])
        assert np.isnan(d["w0"][9]).all() and (d["w4"][9] == 0).all()            # its weighted mean is exact too
        assert np.isnan(d["k5"][14]).all() and np.isnan(d["k8a"][14]).all() and np.isfinite(d["k1"][14]).sum() == pc.NV
        assert abs(d["k0"][0, 10] - 1) < 1e-15 and abs(d["k3"][0, 10] - 1) < 1e-15 and abs(d["k1"][0, 10]) < 1e-15
        assert d["g_k0"][1] == np.inf and d["g_k3"][1] == np.inf and d["g_k0"][0] == np.inf
        if cs.signed:
            assert 0 < 1 - d["k1"][3, 18] < 1e-8                                 # the near anti-parallel pair


def test_restatements_are_within_the_bounds():
    bad = {k: v for k, v in observed().items() if not v <= 1.0}
    assert not bad, bad


def test_bounds_leave_headroom():
    """the largest error / bound over all CPU restatements is at most 0.5: the bounds are not tuned to what one
    implementation happens to give"""
    obs = observed()
    worst = max(obs, key=obs.get)
    assert obs[worst] <= 0.5, f"largest error / bound {obs[worst]:.3f} at {worst}"
    print(f"largest error / bound {obs[worst]:.3f} at {worst}")


def test_bounds_would_catch_a_single_precision_step():
    """the reference times (1 + 2^-40) is out of bound for every value that is inexact and at least an eighth of its
    natural scale (pair_stat_cases.natural_scale).  A value far below its scale is what is left of a cancellation -- a
    Correlation near 0, a Compensation 1 - q with q near 1 -- and no fp64 sum holds it to 2^-40 of itself, whatever the
    bound; every key has at least twenty values of the first kind in every case (the MI kinds, whose tables of 78 branches are close
    to independence, at least one)."""
    fx = fixture()
    for cs in pc.all_cases():
        for key in pc.KEYS:
            if key in pc.EXACT_KEYS:
                continue
            ref, b = fx[cs.name][key], pc.pair_bounds(cs, key)
            sized = np.isfinite(ref) & (b > 0) & (np.abs(ref) >= 0.125 * pc.natural_scale(cs, key)) & (ref != 0)
            inexact = np.isfinite(ref) & (b > 0)
            assert sized.sum() >= (1 if key in pc.MI_BOUNDS else min(20, inexact.sum() // 3)), (cs.name, key, int(sized.sum()))
            r = pc.ratio(ref * (1.0 + 2.0 ** -40), ref, b)
            assert (r[sized] > 1.0).all(), (cs.name, key, float(r[sized].min()))


VM_KINDS = {0: "k0", 3: "k3", 4: "k4", 9: "sp"}


@pytest.mark.parametrize("kind", sorted(VM_KINDS))
def test_vector_matrix_reference_agrees_with_the_fixture(kind):
    """the brute force the plain-vector matrices are held to on the device, at the dims it shares with the fixture"""
    fx = fixture()
    for cs in pc.all_cases():
        if cs.K != 1:
            continue
        X = np.ascontiguousarray(cs.counts[:, :, 0])
        ref, b = fx[cs.name][VM_KINDS[kind]], pc.pair_bounds(cs, VM_KINDS[kind])
        got = pc.vector_matrix_reference(kind, X, X)
        assert pc.check(got, ref, 0.25 * b, f"{cs.name} kind {kind}") <= 1.0
        assert np.allclose(pc.vector_matrix_bounds(kind, X), b, rtol=1e-9, atol=0)
        one = pc.vector_matrix_reference(kind, X)
        iu = np.triu_indices(pc.NV, 1)
        assert np.array_equal(one[iu], got[iu], equal_nan=True) and np.array_equal(one, one.T, equal_nan=True)
        assert (np.diag(one) == 1.0).all() if kind in (0, 3) else np.array_equal(np.diag(one), np.diag(got))


def test_generator_reproduces_the_committed_fixture():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_pair_stat_fixture", os.path.join(GOLDEN, "make_pair_stat_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = np.load(FIXTURE)
    for c in [(3, 1, False), (5, 2, True)]:
        for name, a in gen.case_arrays(pc.case(*c)).items():
            assert np.array_equal(a, z[name], equal_nan=True), name
