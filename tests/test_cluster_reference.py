"""The clustering tests' own reference, checked on the CPU: cluster_reference.hclust_fast is oracle.cluster.hclust bit for
bit; every designed case of tests/cluster_cases.py does what it was built for; deliberately wrong variants of the
reference are told apart by merge / dmax / size in every kernel shape class, while the sorted join distances -- all that
was checked at n >= 2000 before -- let some of them through; the group properties from their definitions."""
import numpy as np
import pytest

from oracle import cluster as oc
import cluster_cases as cc
import cluster_reference as cr


def _euclid(n, seed, dims=5):
    x = np.random.default_rng(seed).normal(size=(n, dims))
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    d = (d + d.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


def _uniform_ties(n, seed):
    d = np.random.default_rng(seed).integers(1, 4, size=(n, n)).astype(np.float64)
    d = np.maximum(d, d.T)
    np.fill_diagonal(d, 0.0)
    return d


@pytest.mark.parametrize("link", cc.LINKS)
@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 150, 300])
def test_fast_reference_equals_the_oracle(link, n):
    for d in (_euclid(n, 10 * n + link), _uniform_ties(n, n), cc.tie_matrix(n, n), cc.two_block_matrix(n, n)):
        assert cr.same_tree(cr.hclust_fast(d, link), oc.hclust(d, link))


@pytest.mark.parametrize("link", cc.LINKS)
def test_fast_reference_equals_the_oracle_on_nan_inf_and_constant_matrices(link):
    d = _euclid(40, 9)                               # the patterns of test_gpu_cluster.test_hclust_nan_and_inf
    d[7, :] = d[:, 7] = np.nan
    d[20, 3] = d[3, 20] = np.inf
    d[7, 7] = 0.0
    assert cr.same_tree(cr.hclust_fast(d, link), oc.hclust(d, link))
    for n in (2, 30, 40):
        d = np.full((n, n), np.nan)
        assert cr.same_tree(cr.hclust_fast(d, link), oc.hclust(d, link))
        d = np.ones((n, n))
        np.fill_diagonal(d, 0.0)
        assert cr.same_tree(cr.hclust_fast(d, link), oc.hclust(d, link))
    for kind in ("holes", "scatter"):                # the table's builders at a size the oracle can follow
        d = cc.BUILDERS[kind](600, 3)
        assert cr.same_tree(cr.hclust_fast(d, link), oc.hclust(d, link))


def test_case_table_covers_every_kernel_shape():
    per = lambda n: next(p for p, top in ((1, 512), (2, 1024), (4, 2048), (6, 3072), (10, 5000)) if n <= top)
    seen = {(per(n), link) for _, n, _, link in cc.CASES}
    assert seen == {(p, link) for p in (1, 2, 4, 6, 10) for link in cc.LINKS}
    for cls, (top, bottom) in cc.CLASSES.items():
        assert bottom == top + 1 and per(bottom) > per(top)
    assert cc.LIMIT == 5000 and len(set(cc.CASES)) == len(cc.CASES)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_designed_cases_meet_their_preconditions(case):
    d = cc.matrix(*case[1:3])
    assert d.shape == (case[1],) * 2
    if case[2] != "allnan":
        assert np.all(np.diag(d) == 0) and np.array_equal(d, d.T, equal_nan=True)
    if case[2] == "holes":
        nan_rows = np.flatnonzero(np.isnan(d).sum(1) > case[1] // 2)
        assert len(nan_rows) == cc.NAN_ROWS and nan_rows[0] == 0 and nan_rows[-1] >= 512 and np.isinf(d).sum() >= 10
    if case[2] == "scatter":
        assert np.isinf(d).sum() == 20 and not np.isnan(d).any()
    cc.check_preconditions(case)


def _applies(mutant, link):
    if mutant.startswith("avg_"):
        return link == oc.LINK_AVERAGE
    if mutant == "keep_cached":                      # under single linkage the new entry IS the cached minimum
        return link != oc.LINK_SINGLE
    return True


def _first_case_told_apart(mutant, cls):
    for case in sorted((c for c in cc.CASES if c[0] == cls and _applies(mutant, c[3])), key=lambda c: c[1]):
        n, kind, link = case[1:]
        if not cr.same_tree(cr.hclust_fast(cc.matrix(n, kind), link, mutant=mutant), cc.reference(n, kind, link)):
            return case
    return None


@pytest.mark.parametrize("cls", list(cc.CLASSES) + ["limit"])
@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_every_mutant_is_told_apart_in_every_shape_class(mutant, cls):
    assert _first_case_told_apart(mutant, cls) is not None


def test_sorted_join_distances_alone_miss_mutants():
    """the check test_hclust_full_size_against_scipy makes at n = 2000: sorted dmax at rtol 1e-12, monotone, root size,
    every node a son once.  Ties taken in the wrong order under single linkage (the sorted distances are the minimum
    spanning tree's, whatever the order) and a fused average (a few ulps) pass it; the exact comparison does not."""
    n = 2049
    missed = set()
    for kind, link in (("ties", oc.LINK_SINGLE), ("random", oc.LINK_AVERAGE)):
        ref = cc.reference(n, kind, link)
        for mutant in cr.MUTANTS:
            if not _applies(mutant, link):
                continue
            got = cr.hclust_fast(cc.matrix(n, kind), link, mutant=mutant)
            old_check = (np.allclose(np.sort(got[1]), np.sort(ref[1]), rtol=1e-12, atol=0) and np.all(np.diff(got[1]) >= -1e-12)
                         and got[2][-1] == n and np.array_equal(np.sort(got[0].ravel()), np.arange(2 * n - 2)))
            if old_check and not cr.same_tree(got, ref):
                missed.add(mutant)
    assert missed >= {"tie_last", "avg_fma"}, missed


@pytest.mark.parametrize("name", list(cc.WIDE_TREES))
def test_group_properties_of_the_oracle_against_their_definitions(name):
    counts = cc.wide_counts(name)
    B = counts.shape[1]
    assert (64 < B <= 256) if name == "B77" else B > 256
    for dist in (oc.DIST_CORRELATION, oc.DIST_COMPENSATION, oc.DIST_EUCLIDIAN):
        for link in cc.LINKS:
            merge, dmax, _ = cc.wide_tree_of(name, dist, link)
            stat, nmin = oc.group_properties(dist, merge, dmax, counts)
            stat_x, nmin_x = cr.group_properties_exact(dist, merge, dmax, counts)
            if dist == oc.DIST_COMPENSATION:
                assert np.abs(stat - stat_x).max() <= cc.stat_bound(name)
            else:
                assert np.array_equal(stat, stat_x)
            assert np.abs(nmin - nmin_x).max() <= cc.nmin_bound(name, counts)


@pytest.mark.parametrize("key", list(cc.WIDE_TREES) + list(cc.LARGE_SITES))
def test_tabled_errors_are_those_of_the_restated_form(key):
    """the tolerances of the GPU tests come from these figures: they must be what the restatement gives on the very inputs"""
    if key in cc.WIDE_TREES:
        counts = cc.wide_counts(key)
        for link in cc.LINKS:
            merge, dmax, _ = cc.wide_tree_of(key, oc.DIST_COMPENSATION, link)
            es, en = cc.measure_props_error(oc.DIST_COMPENSATION, merge, dmax, counts)
            assert es == cc.STAT_ERR[key] and en == cc.NORM_ERR[key]
    else:
        counts = cc.large_counts(key)
        assert float(np.abs(cr.host_norm(counts) - cr.exact_norm(counts)).max()) == cc.NORM_ERR[key]
