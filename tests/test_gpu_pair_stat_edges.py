"""Every device implementation of the pair statistics against the definition-level fixture tests/golden/pair_stats.npz,
within the bounds of tests/pair_stat_cases.py, at the edges of each: the Gram kernel's padding, clamps and row offsets,
the per-lane code behind groups and diagonal pairs, the hash-table MI kernels, the weighted operands, the plain-vector
matrices and the clustering distances.

Site i of an n-site input is fixture vector (start + i) % 19, so the reference of pair (i, j) is the fixture's entry for
those two residues: a wrong clamp or a tile shifted by 16, 64 or 256 columns lands on another residue."""
import numpy as np
import pytest
import torch

import pair_stat_cases as pc
import tree_shapes as ts
from comap_amd import engine, synthetic
from oracle import cluster as oc

pytestmark = pytest.mark.gpu
fixture = pc.fixture

CASE_BY_NAME = {pc.case_name(*c): c for c in pc.CASES}
DENSE_N = [1, 2, 19, 63, 64, 65, 255, 256, 257]
EDGE_CASES = ["B5K1", "B5K2s", "B78K1"]          # B % 4 = 1 and a single padded k-step pair; signed K = 2; B > 64, B % 4 = 2
_ENGINES = {}


def _tree(B):
    """a DNA tree with B branches: unrooted with (B + 3) / 2 taxa for odd B, rooted for even B"""
    if B % 2:
        return synthetic.random_tree((B + 3) // 2, 11 + B)
    parent, lot = ts._caterpillar((B + 2) // 2) if B < 10 else ts._balanced((B + 2) // 2)
    blen = np.full(len(parent), 0.1)
    blen[-1] = 0.0
    return parent, blen, lot


def eng_of(name):
    if name not in _ENGINES:
        B, K, signed = CASE_BY_NAME[name]
        parent, blen, lot = _tree(B)
        mdl = synthetic.dna_model(0.5, 4)
        kw = {}
        if K == 2:
            W = synthetic.compensation_weights_dna()
            second = W if signed else np.abs(W)
            kw = dict(Bk=np.stack([synthetic.weighted_register(mdl["Q"]), synthetic.weighted_register(mdl["Q"], second)]),
                      clamp_negative=not signed)
        e = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], **kw)
        assert (e.B, e.K) == (B, K)
        _ENGINES[name] = e
    return _ENGINES[name]


def call(cs, key):
    """(engine kind, keyword arguments) of a statistic key"""
    if key in ("k8a", "k8l"):
        return engine.STAT_DISCRETE_MI_BOUNDS, dict(threshold=pc.MI_BOUNDS[key])
    if key in ("k6", "w6"):
        return engine.STAT_CORRECTED_CORRELATION, dict(mean_vectors=cs.mv)
    return pc.kind_of(key), {}


def ref_of(cs, key, idx1, idx2=None):
    r = fixture()[cs.name][key]
    return r[np.ix_(idx1, idx1 if idx2 is None else idx2)], pc.pair_bounds(cs, key, idx1, idx2)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ dense pair_stats
@pytest.mark.parametrize("name,n", [(c, n) for c in ("B5K1", "B78K1") for n in DENSE_N] +
                         [(c, 65) for c in CASE_BY_NAME if c not in ("B5K1", "B78K1")])
def test_dense_one_set(name, n):
    cs, eng = pc.case(*CASE_BY_NAME[name]), eng_of(name)
    counts, idx = cs.expand(n, start=3)
    iu, il = np.triu_indices(n, 1), np.tril_indices(n)
    for key in pc.UNWEIGHTED_KEYS:
        kind, kw = call(cs, key)
        got = eng.pair_stats(kind, counts, **kw)
        assert np.isnan(got[il]).all(), (key, "j <= i is NaN")
        ref, b = ref_of(cs, key, idx)
        pc.check(got[iu], ref[iu], b[iu], f"{name} {key} n={n}")


@pytest.mark.parametrize("name", EDGE_CASES)
@pytest.mark.parametrize("n1,n2", [(1, 257), (257, 1), (65, 19), (64, 256), (33, 300)])
def test_dense_two_sets(name, n1, n2):
    cs, eng = pc.case(*CASE_BY_NAME[name]), eng_of(name)
    (c1, i1), (c2, i2) = cs.expand(n1, start=3), cs.expand(n2, start=8)
    for key in pc.UNWEIGHTED_KEYS:
        kind, kw = call(cs, key)
        got = eng.pair_stats(kind, c1, c2, **kw)
        ref, b = ref_of(cs, key, i1, i2)
        pc.check(got, ref, b, f"{name} {key} {n1}x{n2}")          # (NaN only where the reference has it: no NaN triangle)


def test_compensation_of_a_rectangle_of_cancelling_pairs():
    """every pair of a 300 x 333 rectangle is the near anti-parallel pair: whole tiles and ragged ones take the direct sum,
    and all get the one value"""
    cs, eng = pc.case(5, 2, True), eng_of("B5K2s")
    c1, c2 = np.repeat(cs.counts[3:4], 300, axis=0), np.repeat(cs.counts[18:19], 333, axis=0)
    got = eng.pair_stats(engine.STAT_COMPENSATION, c1, c2)
    assert (got == got[0, 0]).all()
    pc.check(got[:1, :1], fixture()[cs.name]["k1"][3:4, 18:19], pc.pair_bounds(cs, "k1")[3:4, 18:19], "anti-parallel rectangle")


# ------------------------------------------------------------------------------------------------ row blocks
def _dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)


def _pairs_of_rows(n, r0, r1):
    return sum(n - 1 - i for i in range(r0, r1))


@pytest.mark.parametrize("name", EDGE_CASES)
def test_row_blocks_without_a_null(name):
    cs, eng = pc.case(*CASE_BY_NAME[name]), eng_of(name)
    n = 257
    counts, idx = cs.expand(n, start=3)
    d_counts, d_norm = _dev(counts.reshape(n, -1).T), _dev(1.0 + np.arange(n) % 7)
    iu = np.triu_indices(n, 1)

    def run(key, r0, r1):
        kind, kw = call(cs, key)
        out = torch.zeros(_pairs_of_rows(n, r0, r1) * engine.PAIR_COMPACT.itemsize, dtype=torch.uint8, device="cuda")
        eng.intra_compact_range_dev(kind, d_counts, d_norm, None, None, 4, out, r0, r1, **kw)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    for key in [k for k in pc.UNWEIGHTED_KEYS if k not in ("k7", "sp")]:
        whole = run(key, 0, n)
        pieces = np.concatenate([run(key, 0, 37), run(key, 37, 100), run(key, 100, n)])     # irow0 = 37, 100: no multiple of 64
        assert same_bytes(whole, pieces), key
        ref, b = ref_of(cs, key, idx)
        pc.check(whole.view(engine.PAIR_COMPACT)["stat"], ref[iu], b[iu], f"{name} {key} rows")
    with pytest.raises(engine.CmxError) as err:
        run("k7", 0, n)
    assert err.value.status == -2                     # CMX_ERR_UNSUPPORTED: a distance, not a statistic


# ------------------------------------------------------------------------------------------------ per-lane code
PAIR_GROUPS = [[i, j] for i in range(pc.NV) for j in range(pc.NV) if i != j]


def _group_refs(cs, key):
    """reference and bound of PAIR_GROUPS + pc.GROUPS"""
    d = fixture()[cs.name]
    R = d[key]
    if pc.kind_of(key) == 1:       # the closed form of two members is the pair's formula (NaN stays NaN)
        ref = [R[g[1], g[0]] for g in PAIR_GROUPS]
    else:                          # a minimum: a NaN pair never wins
        ref = [R[g[1], g[0]] if np.isfinite(R[g[1], g[0]]) else np.inf for g in PAIR_GROUPS]
    groups = PAIR_GROUPS + pc.GROUPS
    ref = np.concatenate([ref, d["g_" + key]])
    return ref, np.array([pc.group_bound(cs, key, g, R) for g in groups])


@pytest.mark.parametrize("name", list(CASE_BY_NAME))
def test_groups_on_the_per_lane_code(name):
    cs, eng = pc.case(*CASE_BY_NAME[name]), eng_of(name)
    groups = PAIR_GROUPS + pc.GROUPS
    iu = np.triu_indices(pc.NV, 1)
    for key in [k for k in pc.UNWEIGHTED_KEYS if k != "sp"]:
        kind, kw = call(cs, key)
        got = eng.group_stats(kind, cs.counts, groups, **kw)
        ref, b = _group_refs(cs, key)
        pc.check(got, ref, b, f"{name} {key} groups")
        if key in ("k2", "k5", "k8a", "k8l"):
            # integer tables tie with null values and the p-value rule is strict: the dense path and the per-lane /
            # per-wave path give the same bytes for the same pair
            dense = eng.pair_stats(kind, cs.counts, **kw)[iu]
            lanes = np.array([got[PAIR_GROUPS.index([j, i])] for i, j in zip(*iu)])
            assert same_bytes(np.where(np.isnan(dense), np.inf, dense), lanes), key


VM_KEYS = {engine.STAT_CORRELATION: "k0", engine.STAT_COSINUS: "k3", engine.STAT_COVARIANCE: "k4", engine.STAT_SCALAR_PRODUCT: "sp"}


@pytest.mark.parametrize("name", list(CASE_BY_NAME))
def test_vector_matrix_independent_diagonal(name):
    cs, eng = pc.case(*CASE_BY_NAME[name]), eng_of(name)
    idx2 = (np.arange(pc.NV) + 3) % pc.NV
    X1 = np.ascontiguousarray(cs.counts[:, :, 0])
    X2 = np.ascontiguousarray(X1[idx2])
    off = ~np.eye(pc.NV, dtype=bool)
    for kind, key in VM_KEYS.items():
        got = eng.vector_matrix(kind, X1, X2, independent=True)
        assert (got[off] == 0).all()
        R = fixture()[cs.name][key]
        pc.check(np.diag(got), R[np.arange(pc.NV), idx2], pc.pair_bounds(cs, key)[np.arange(pc.NV), idx2], f"{name} {key} diagonal")


def _plain_vectors(dim, n, seed):
    """fixture type-0 columns where a K = 1 case has this length, otherwise fresh draws with the same special vectors"""
    for c in pc.CASES:
        if c[0] == dim and c[1] == 1 and n == pc.NV:
            return np.ascontiguousarray(pc.case(*c).counts[:, :, 0]), pc.case(*c)
    rng = np.random.default_rng([dim, n, seed])
    X = rng.gamma(0.3, 3.0, size=(n, dim))
    X[3] = 0.0
    X[4] = 0.5
    X[5] = X[0] / 8
    X[6] = X[1] * (1 + 1e-9 * rng.standard_normal(dim))
    X[7] = X[2] + 64
    return X, None


@pytest.mark.parametrize("dim", [2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130])
def test_vector_matrix_dims(dim):
    eng = eng_of("B5K1")
    X, cs = _plain_vectors(dim, pc.NV, 1)
    Y, _ = _plain_vectors(dim, 23, 2)
    iu = np.triu_indices(pc.NV, 1)
    for kind, key in VM_KEYS.items():
        if dim < 2 and kind in (engine.STAT_CORRELATION, engine.STAT_COVARIANCE):
            continue
        one = eng.vector_matrix(kind, X)
        pc.check(one, pc.vector_matrix_reference(kind, X), pc.vector_matrix_bounds(kind, X), f"dim {dim} kind {kind} one set")
        assert same_bytes(one, one.T)                                  # the lower triangle mirrors the upper one
        if kind in (engine.STAT_CORRELATION, engine.STAT_COSINUS):
            assert (np.diag(one) == 1.0).all()                         # AnalysisTools.cpp:178, 236: not f(v, v)
        two = eng.vector_matrix(kind, X, Y)
        pc.check(two, pc.vector_matrix_reference(kind, X, Y), pc.vector_matrix_bounds(kind, X, Y), f"dim {dim} kind {kind} two sets")
        same = eng.vector_matrix(kind, X, X)                           # two sets: the diagonal is f(v, v)
        assert same_bytes(same[iu], one[iu])
        if cs is not None:
            pc.check(same, fixture()[cs.name][key], pc.pair_bounds(cs, key), f"dim {dim} kind {kind} fixture")


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("name", list(CASE_BY_NAME))
def test_weighted_kinds_and_the_kinds_that_ignore_weights(name):
    cs, eng = pc.case(*CASE_BY_NAME[name]), eng_of(name)
    n = 65
    counts, idx = cs.expand(n, start=3)
    iu = np.triu_indices(n, 1)
    groups = PAIR_GROUPS + pc.GROUPS
    ignoring = ["k2", "k5", "k8a", "k8l", "sp"]
    plain = {}
    for key in ignoring:
        kind, kw = call(cs, key)
        plain[key] = (eng.pair_stats(kind, counts, **kw), None if key == "sp" else eng.group_stats(kind, cs.counts, groups, **kw))
    eng.set_statistic_weights(cs.w_raw)
    try:
        assert np.array_equal(eng.statistic_weights(), cs.w)
        for key in pc.WEIGHTED_KEYS:
            kind, kw = call(cs, key)
            got = eng.pair_stats(kind, counts, **kw)
            assert np.isnan(got[np.tril_indices(n)]).all()
            ref, b = ref_of(cs, key, idx)
            pc.check(got[iu], ref[iu], b[iu], f"{name} {key} n={n}")
            ref, b = _group_refs(cs, key)
            pc.check(eng.group_stats(kind, cs.counts, groups, **kw), ref, b, f"{name} {key} groups")
        for key in ignoring:
            kind, kw = call(cs, key)
            assert same_bytes(eng.pair_stats(kind, counts, **kw), plain[key][0]), key
            if key != "sp":
                assert same_bytes(eng.group_stats(kind, cs.counts, groups, **kw), plain[key][1]), key
    finally:
        eng.set_statistic_weights(None)


# ------------------------------------------------------------------------------------------------ clustering distances
@pytest.mark.parametrize("name", EDGE_CASES)
@pytest.mark.parametrize("dist_kind,key", [(engine.DIST_CORRELATION, "k0"), (engine.DIST_COMPENSATION, "k1"),
                                           (engine.DIST_EUCLIDIAN, "k7")])
def test_clustering_distances(name, dist_kind, key):
    cs, eng = pc.case(*CASE_BY_NAME[name]), eng_of(name)
    n = 65
    counts, idx = cs.expand(n, start=3)
    d = eng.cluster_sites(dist_kind, engine.LINK_AVERAGE, counts, want_dist=True)["dist"]
    assert same_bytes(d, d.T) and (np.diag(d) == 0).all()
    R, b = ref_of(cs, key, idx)
    # oracle/cluster.py distance_matrix: the statistic itself for EuclidianDistance, 1 - statistic otherwise (one more rounding)
    ref = R if dist_kind == oc.DIST_EUCLIDIAN else 1.0 - R
    iu = np.triu_indices(n, 1)
    pc.check(d[iu], ref[iu], (b + (0 if dist_kind == oc.DIST_EUCLIDIAN else 2 * pc.U))[iu], f"{name} {key} distances")
