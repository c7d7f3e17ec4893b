"""The clustering stage at every kernel shape, against cluster_reference.hclust_fast (bit for bit) and the group properties'
definitions: every hclust_kernel<LINK, PER> instantiation at both sides of its size threshold, rescans over several
segments, the row-minimum kernel's grid stride, the device-pointer entries with a leading dimension and a stream, the
group-property kernel with more branches than a wave and than a workgroup, the null in more than one pass.  Cases,
preconditions and tolerances: tests/cluster_cases.py (checked on the CPU by tests/test_cluster_reference.py).
Every line printed is  case  quantity  largest device error  bound."""
import numpy as np
import pytest

import oracle
from oracle import cluster as oc
from comap_amd import engine, synthetic
import cluster_cases as cc
import cluster_reference as cr

pytestmark = pytest.mark.gpu

DISTS = {"cor": oc.DIST_CORRELATION, "comp": oc.DIST_COMPENSATION, "euclid": oc.DIST_EUCLIDIAN}
PAYLOAD = 0x7FF8C0DE0BADF00D        # a quiet NaN no arithmetic produces: padding must come back with these very bits


@pytest.fixture(scope="module")
def bare():
    return engine.Engine()


def _same_tree(g, ref):
    assert np.array_equal(g["merge"], ref[0])
    assert np.array_equal(g["dmax"], ref[1])
    assert np.array_equal(g["size"], ref[2])


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_exact_trees(bare, case):
    n, kind, link = case[1:]
    _same_tree(bare.hclust(cc.matrix(n, kind), link), cc.reference(n, kind, link))


@pytest.mark.parametrize("side_stream", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("n", [513, 1025])
def test_hclust_dev_leading_dimension_and_stream(bare, n, side_stream):
    """batch of three matrices with rows n + 7 apart: the trees are the reference's, and neither the linkage update's
    column addressing nor the NaN -> +inf rewrite touches the padding"""
    import torch
    kinds, pad = ("holes", "ties", "random"), 7
    host = torch.from_numpy(np.stack([cc.matrix(n, k) for k in kinds]))
    for link in cc.LINKS:
        buf = torch.empty((3, n, n + pad), dtype=torch.float64, device="cuda")
        buf.view(torch.int64).fill_(PAYLOAD)
        buf[:, :, :n] = host.cuda()
        merge = torch.zeros((3, n - 1, 2), dtype=torch.int32, device="cuda")
        dmax = torch.zeros((3, n - 1), dtype=torch.float64, device="cuda")
        size = torch.zeros((3, n - 1), dtype=torch.int32, device="cuda")
        dist = buf[:, :, :n]
        assert dist.stride(1) == n + pad and dist.stride(0) == n * (n + pad)
        torch.cuda.synchronize()
        if side_stream:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                assert torch.cuda.current_stream() != torch.cuda.default_stream()
                bare.hclust_dev(link, dist, merge, dmax, size)
            s.synchronize()
        else:
            bare.hclust_dev(link, dist, merge, dmax, size)
        torch.cuda.synchronize()
        for b, kind in enumerate(kinds):
            _same_tree(dict(merge=merge[b].cpu().numpy(), dmax=dmax[b].cpu().numpy(), size=size[b].cpu().numpy()),
                       cc.reference(n, kind, link))
        assert bool((buf.view(torch.int64)[:, :, n:] == PAYLOAD).all())
        assert not bool(torch.isnan(dist).any())             # inside the n columns the rewrite did happen


def test_row_minimum_grid_stride(bare):
    """more (matrix, row) pairs than the row-minimum kernel's grid has waves: its stride loop takes a second trip"""
    batch, n = 1100, 30
    assert batch * n > 8192 * 4
    rng = np.random.default_rng(30)
    ds = rng.random((batch, n, n))
    ds = np.triu(ds, 1) + np.triu(ds, 1).transpose(0, 2, 1)
    g = bare.hclust(ds, oc.LINK_AVERAGE)
    for b in range(batch):
        merge, dmax, size = oc.hclust(ds[b], oc.LINK_AVERAGE)
        assert np.array_equal(g["merge"][b], merge) and np.array_equal(g["dmax"][b], dmax) and np.array_equal(g["size"][b], size), b


@pytest.fixture(scope="module")
def small_engine():
    parent, blen, lot = synthetic.random_tree(cc.LARGE_TAXA, cc.LARGE_TREE_SEED)
    mdl = synthetic.dna_model(1.0, 1)
    return engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])


@pytest.mark.parametrize("dname,link", [("euclid", oc.LINK_AVERAGE), ("cor", oc.LINK_COMPLETE)])
@pytest.mark.parametrize("n", cc.LARGE_SITES)
def test_cluster_sites_trees_from_the_device_distances(small_engine, n, dname, link):
    dist = DISTS[dname]
    counts = cc.large_counts(n)
    assert counts.shape == (n, small_engine.B, 1)
    g = small_engine.cluster_sites(dist, link, counts)
    assert np.array_equal(g["dist"], g["dist"].T) and np.all(np.diag(g["dist"]) == 0)
    _same_tree(g, cr.hclust_fast(g["dist"], link))
    assert np.array_equal(g["stat"], g["dmax"] if dist == oc.DIST_EUCLIDIAN else 1.0 - g["dmax"])
    _, nmin = cr.group_properties_exact(dist, g["merge"], g["dmax"], counts)
    err, bound = float(np.abs(g["nmin"] - nmin).max()), cc.nmin_bound(n, counts)
    print(f"sites-{n}-{dname}  nmin  {err:.3e}  {bound:.3e}")
    assert err <= bound


@pytest.fixture(scope="module", params=list(cc.WIDE_TREES))
def wide(request):
    """DNA model with two signed registers on a tree of more branches than a wave (B77) / than a workgroup (B277) has lanes"""
    name = request.param
    parent, blen, lot = cc.wide_tree(name)
    mdl = synthetic.dna_model(5.0, 4)
    rng = np.random.default_rng(len(parent))
    Bk = np.stack([synthetic.weighted_register(mdl["Q"], rng.uniform(-1, 1, size=(4, 4))) for _ in range(cc.WIDE_K)])
    eng = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], clamp_negative=False, Bk=Bk)
    assert eng.K == cc.WIDE_K == 2
    assert (64 < eng.B <= 256) if name == "B77" else eng.B > 256
    return name, eng


@pytest.mark.parametrize("dname", list(DISTS))
def test_group_properties_on_wide_trees(wide, dname):
    import torch
    name, eng = wide
    dist, counts, n = DISTS[dname], cc.wide_counts(name), cc.WIDE_SITES
    assert counts.shape == (n, eng.B, eng.K)
    worst_stat = worst_nmin = 0.0
    for link in cc.LINKS:
        g = eng.cluster_sites(dist, link, counts)
        _same_tree(g, cr.hclust_fast(g["dist"], link))
        assert np.array_equal(g["merge"], cc.wide_tree_of(name, dist, link)[0])    # the tree the tabled errors were measured on
        stat, nmin = cr.group_properties_exact(dist, g["merge"], g["dmax"], counts)
        if dist == oc.DIST_COMPENSATION:
            worst_stat = max(worst_stat, float(np.abs(g["stat"] - stat).max()))
            assert np.abs(g["stat"] - stat).max() <= cc.stat_bound(name)
        else:
            assert np.array_equal(g["stat"], g["dmax"] if dist == oc.DIST_EUCLIDIAN else 1.0 - g["dmax"])
            assert np.array_equal(g["stat"], stat)
        worst_nmin = max(worst_nmin, float(np.abs(g["nmin"] - nmin).max()))
        assert np.abs(g["nmin"] - nmin).max() <= cc.nmin_bound(name, counts)
        # the device-pointer entry with the count rows n + 5 apart: the same bytes
        ldc = n + 5
        d_counts = torch.full((eng.B * eng.K, ldc), float("nan"), dtype=torch.float64, device="cuda")
        d_counts[:, :n] = torch.from_numpy(np.ascontiguousarray(counts.reshape(n, -1).T)).cuda()
        d_norm = torch.from_numpy(cr.host_norm(counts)).cuda()
        out = dict(dist=torch.zeros((n, n), dtype=torch.float64, device="cuda"),
                   merge=torch.zeros((n - 1, 2), dtype=torch.int32, device="cuda"),
                   size=torch.zeros(n - 1, dtype=torch.int32, device="cuda"),
                   **{k: torch.zeros(n - 1, dtype=torch.float64, device="cuda") for k in ("dmax", "stat", "nmin")})
        eng.cluster_sites_dev(dist, link, d_counts[:, :n], d_norm, out["merge"], out["dmax"], out["size"], out["stat"],
                              out["nmin"], dist=out["dist"])
        torch.cuda.synchronize()
        for k, v in out.items():
            assert np.array_equal(v.cpu().numpy(), g[k]), (k, link)
        assert bool(torch.isnan(d_counts[:, n:]).all())
    if dist == oc.DIST_COMPENSATION:
        print(f"{name}-{dname}  stat  {worst_stat:.3e}  {cc.stat_bound(name):.3e}")
    print(f"{name}-{dname}  nmin  {worst_nmin:.3e}  {cc.nmin_bound(name, counts):.3e}")


def test_cluster_null_in_more_than_one_pass():
    """1030 replicates: the null's pass loop (1024 replicates a pass at the most) runs twice, the second pass from a
    non-zero replicate and output offset"""
    from test_gpu_cluster import _setup, _no_duplicate_columns
    om, eng = _setup(4, 18, 8)
    dist, link, seed, nsites, nrep = oc.DIST_EUCLIDIAN, oc.LINK_AVERAGE, 123, 5, 1030
    assert nrep > 1024
    g = eng.cluster_null(dist, link, seed, 0, nrep, nsites)
    a = eng.cluster_null(dist, link, seed, 0, 1024, nsites)
    b = eng.cluster_null(dist, link, seed, 1024, nrep, nsites)
    for k in g:
        assert np.array_equal(g[k], np.concatenate([a[k], b[k]])), k
    for r in range(1020, nrep):
        _no_duplicate_columns(oracle.simulate(om, seed, r * nsites, nsites)[0])
    o = oc.cluster_null(om, dist, link, seed, 1020, nrep, nsites)
    for q, r in enumerate(range(1020, nrep)):
        assert np.array_equal(g["merge"][r], o[q]["merge"]) and np.array_equal(g["size"][r], o[q]["size"])
        assert np.allclose(g["dmax"][r], o[q]["dmax"], rtol=1e-6, atol=1e-12)
        assert np.allclose(g["stat"][r], o[q]["stat"], rtol=1e-6, atol=1e-9)
        assert np.allclose(g["nmin"][r], o[q]["nmin"], rtol=1e-6, atol=0)
