"""Mica's column mutual information for alphabets other than 4 / 20 states (2 .. 64: codon models), cmx_mica_wide.hip: the
matrix-core kernel (one or two row tiles, both epilogues), the plain kernel (listed pairs, more than 2 047 taxa, the debug
switch), the entropies, the parametric null on a codon-sized model, the output table, the refusals, the scratch guard.
The yardstick is the numpy restatement of tests/mica_wide_reference.py (pinned to the oracle by
tests/test_mica_wide_reference.py), and the oracle itself up to 31 states.  Tolerances are this stage's own
(test_mi_columns_mfma_path_resolved_and_mixed_columns)."""
import numpy as np
import pytest

import oracle
import mica_wide_reference as ref
from comap_amd import engine, formats, mica, protein_models as pm
from conftest import make_case, rel_close

pytestmark = pytest.mark.gpu

SHAPES = [(2, 33, 9, 7), (21, 65, 9, 7), (31, 256, 12, 10), (32, 40, 9, 7), (33, 31, 5, 9), (61, 64, 10, 9), (63, 97, 9, 7),
          (64, 256, 9, 10), (64, 1, 3, 3), (61, 40, 1, 1)]


@pytest.fixture(scope="module")
def eng():
    return engine.Engine()


def _inputs(A, T, n1, n2, seed=0):
    return ref.columns(A, T, n1, 1000 * A + T + seed), ref.columns(A, T, n2, 1000 * A + T + seed + 1)


def _check(r, o, intra=False):
    n1, n2 = o["mi"].shape
    keep = np.triu(np.ones((n1, n2), dtype=bool), 1) if intra else np.ones((n1, n2), dtype=bool)
    for k in ("mi", "hjoint"):
        assert np.isnan(r[k][~keep]).all(), k + ": NaN on and below the diagonal"
        rel_close(r[k][keep], o[k][keep], 1e-6, 1e-12)
    rel_close(r["h1"], o["h1"], 1e-9, 1e-12)
    rel_close(r["h2"], o["h2"], 1e-9, 1e-12)


@pytest.mark.parametrize("A,T,n1,n2", SHAPES)
def test_columns_match_the_restatement(eng, A, T, n1, n2):
    a1, a2 = _inputs(A, T, n1, n2)
    r = eng.mi_columns(a1, a2, nalpha=A)
    o = ref.mi_columns(a1, a2, A)
    _check(r, o)
    ri = eng.mi_columns(a1, None, nalpha=A)
    oi = ref.mi_columns(a1, None, A)
    _check(ri, oi, intra=True)
    assert np.array_equal(ri["h1"], r["h1"]) and np.array_equal(ri["h2"], ri["h1"])
    if A <= 31:
        _check(r, oracle.mi_columns(a1, a2, A))
        _check(ri, oracle.mi_columns(a1, a1, A), intra=True)
    if n1 >= 3 and n2 >= 3:
        if T > 1 and n1 >= 5:
            assert (a1[:, : n1 // 2] >= A).any() and not (a1[:, n1 // 2:-1] >= A).any()   # both epilogues in one call
        assert abs(r["h1"][1] - np.log(A)) <= 1e-9 * np.log(A) + 1e-12 and abs(r["h1"][-1]) <= 1e-12
        assert abs(r["h2"][1] - np.log(A)) <= 1e-9 * np.log(A) + 1e-12 and abs(r["h2"][-1]) <= 1e-12
        for k in (1, -1):                                    # the all-unknown and the constant column
            assert np.abs(r["mi"][k, :]).max() <= 1e-12 and np.abs(r["mi"][:, k]).max() <= 1e-12


def test_same_call_twice_and_permuted_columns_give_the_same_bytes(eng):
    A, T, n1, n2 = 61, 64, 13, 11
    a1, a2 = _inputs(A, T, n1, n2)
    rng = np.random.default_rng(3)
    p1, p2 = rng.permutation(n1), rng.permutation(n2)
    was = engine.mica_wide_plain(None)
    try:
        for plain in (False, True):
            engine.mica_wide_plain(plain)
            r, again = eng.mi_columns(a1, a2, nalpha=A), eng.mi_columns(a1, a2, nalpha=A)
            rp = eng.mi_columns(a1[:, p1], a2[:, p2], nalpha=A)
            for k in ("mi", "hjoint"):
                assert r[k].tobytes() == again[k].tobytes(), (plain, k)
                assert rp[k].tobytes() == np.ascontiguousarray(r[k][p1][:, p2]).tobytes(), (plain, k)
            assert rp["h1"].tobytes() == r["h1"][p1].tobytes() and rp["h2"].tobytes() == r["h2"][p2].tobytes()
    finally:
        engine.mica_wide_plain(was)


def test_device_entry_with_padded_leading_dimensions(eng):
    import torch
    A, T, n1, n2 = 61, 64, 13, 11
    a1, a2 = _inputs(A, T, n1, n2)
    r = eng.mi_columns(a1, a2, nalpha=A)
    dev = torch.device("cuda", eng.device)
    d1 = torch.full((T, n1 + 3), 9, dtype=torch.uint8, device=dev)
    d2 = torch.full((T, n2 + 6), 9, dtype=torch.uint8, device=dev)
    d1[:, :n1] = torch.from_numpy(a1).to(dev)
    d2[:, :n2] = torch.from_numpy(a2).to(dev)
    mi = torch.full((n1, n2 + 5), -7.0, dtype=torch.float64, device=dev)
    hj = torch.full((n1, n2 + 5), -7.0, dtype=torch.float64, device=dev)
    h1 = torch.full((n1 + 2,), -7.0, dtype=torch.float64, device=dev)
    h2 = torch.full((n2 + 2,), -7.0, dtype=torch.float64, device=dev)
    eng.mi_columns_dev(d1[:, :n1], mi[:, :n2], hj[:, :n2], d2[:, :n2], nalpha=A, h1=h1, h2=h2)
    torch.cuda.synchronize()
    mi, hj, h1, h2 = mi.cpu().numpy(), hj.cpu().numpy(), h1.cpu().numpy(), h2.cpu().numpy()
    assert np.ascontiguousarray(mi[:, :n2]).tobytes() == r["mi"].tobytes()
    assert np.ascontiguousarray(hj[:, :n2]).tobytes() == r["hjoint"].tobytes()
    assert h1[:n1].tobytes() == r["h1"].tobytes() and h2[:n2].tobytes() == r["h2"].tobytes()
    assert (mi[:, n2:] == -7.0).all() and (hj[:, n2:] == -7.0).all() and (h1[n1:] == -7.0).all() and (h2[n2:] == -7.0).all()
    # the intra form: j > i filled, NaN elsewhere inside, the sentinel outside
    mi = torch.full((n1, n1 + 5), -7.0, dtype=torch.float64, device=dev)
    hj = torch.full((n1, n1 + 5), -7.0, dtype=torch.float64, device=dev)
    eng.mi_columns_dev(d1[:, :n1], mi[:, :n1], hj[:, :n1], None, nalpha=A)
    torch.cuda.synchronize()
    ri = eng.mi_columns(a1, None, nalpha=A)
    assert np.array_equal(mi.cpu().numpy()[:, :n1], ri["mi"], equal_nan=True) and (mi.cpu().numpy()[:, n1:] == -7.0).all()
    assert np.array_equal(hj.cpu().numpy()[:, :n1], ri["hjoint"], equal_nan=True) and (hj.cpu().numpy()[:, n1:] == -7.0).all()


@pytest.mark.parametrize("A,T,n1,n2", [(64, 256, 9, 10), (21, 65, 9, 7)])
def test_two_paths_one_answer(eng, A, T, n1, n2):
    a1, a2 = _inputs(A, T, n1, n2)
    was = engine.mica_wide_plain(None)
    try:
        engine.mica_wide_plain(True)
        assert engine.mica_wide_plain(None) is True
        p, pi = eng.mi_columns(a1, a2, nalpha=A), eng.mi_columns(a1, None, nalpha=A)
        engine.mica_wide_plain(False)
        m, mi_ = eng.mi_columns(a1, a2, nalpha=A), eng.mi_columns(a1, None, nalpha=A)
    finally:
        engine.mica_wide_plain(was)
    iu = np.triu_indices(n1, 1)
    for k in ("mi", "hjoint"):
        assert np.abs(p[k] - m[k]).max() <= 1e-12, k
        assert np.abs(pi[k][iu] - mi_[k][iu]).max() <= 1e-12 and np.array_equal(np.isnan(pi[k]), np.isnan(mi_[k])), k
    for k in ("h1", "h2"):
        assert p[k].tobytes() == m[k].tobytes() and pi[k].tobytes() == mi_[k].tobytes(), k


def test_past_the_matrix_core_range(eng):
    """2 047 taxa is the matrix-core kernel's last size, 2 048 the plain kernel's first; the first 2 047 taxa are shared,
    so a wrong T in either shows"""
    A, n1, n2 = 64, 5, 4
    a1, a2 = _inputs(A, 2048, n1, n2)
    for T in (2047, 2048):
        r = eng.mi_columns(a1[:T], a2[:T], nalpha=A)
        _check(r, ref.mi_columns(a1[:T], a2[:T], A))
        _check(eng.mi_columns(a1[:T], None, nalpha=A), ref.mi_columns(a1[:T], None, A), intra=True)


def test_listed_pairs(eng):
    A, T, n, npairs = 61, 48, 60, 37
    a1, a2 = _inputs(A, T, n, n)
    a1[:, 7] = A                                              # a second all-unknown column (column 1 is one already)
    rng = np.random.default_rng(8)
    i1, i2 = rng.integers(0, n, size=npairs), rng.integers(0, n, size=npairs)
    i1[0], i2[0] = 5, 5                                       # i = j
    i1[3], i2[3] = i1[2], i2[2]                               # a repeated pair
    i1[4], i2[4] = 1, 7                                       # two all-unknown columns
    i1[5], i2[5] = n - 1, 0
    for second in (None, a2):
        r = eng.mi_pairs(a1, i1, i2, second, nalpha=A)
        o = ref.mi_pairs(a1, i1, i2, A, second)
        rel_close(r["mi"], o["mi"], 1e-6, 1e-12)
        rel_close(r["hjoint"], o["hjoint"], 1e-6, 1e-12)
        full = eng.mi_columns(a1, a1 if second is None else second, nalpha=A)
        assert np.abs(r["mi"] - full["mi"][i1, i2]).max() <= 1e-12 and np.abs(r["hjoint"] - full["hjoint"][i1, i2]).max() <= 1e-12
        again = eng.mi_pairs(a1, i1, i2, second, nalpha=A)
        assert again["mi"].tobytes() == r["mi"].tobytes() and again["hjoint"].tobytes() == r["hjoint"].tobytes()
        assert r["mi"][2] == r["mi"][3]
        if second is None:
            assert abs(r["mi"][4]) <= 1e-12 and abs(r["hjoint"][4] - 2 * np.log(A)) <= 1e-9


def _codon_case(S, ntaxa=9, nsites=70, seed=5):
    """_case of tests/test_gpu_codon_alphabets.py"""
    case = make_case(ntaxa, nsites, 20, seed)
    Q, pi = pm.synthetic_reversible(S, seed + 100)
    rng = np.random.default_rng(seed)
    aln = rng.integers(0, S, size=case["aln"].shape).astype(np.uint8)
    base = rng.integers(0, S, size=(1, nsites))
    aln = np.where(rng.random(aln.shape) < 0.6, base, aln).astype(np.uint8)
    aln[2, ::7] = S
    aln[5, 3::11] = 200
    case.update(Q=Q, pi=pi, aln=aln)
    return case


def test_parametric_null_on_a_codon_sized_model():
    case = _codon_case(61, ntaxa=8)
    args = (case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    em, om = engine.Engine(*args), oracle.Model(*args)
    seed, nrep, ram = 77, 2, 50
    r = em.mica_parametric_null(seed, nrep, ram)
    sims = [[oracle.simulate(om, seed, (rep * 2 + h) * ram, ram)[0] for h in range(2)] for rep in range(nrep)]
    j = np.arange(ram)
    o = [ref.mi_pairs(s[0], j, j, 61, s[1]) for s in sims]
    rel_close(r["mi"], np.concatenate([x["mi"] for x in o]), 1e-6, 1e-12)
    rel_close(r["hjoint"], np.concatenate([x["hjoint"] for x in o]), 1e-6, 1e-12)
    d, h = mica.parametric_null(em, seed, nrep, ram, nalpha=61), mica.parametric_null_via_host(em, seed, nrep, ram, nalpha=61)
    assert d["mi"].tobytes() == h["mi"].tobytes() and d["hjoint"].tobytes() == h["hjoint"].tobytes()
    assert d["mi"].tobytes() == r["mi"].tobytes()
    rn = em.mica_parametric_null(seed, nrep, ram, with_norms=True)
    assert rn["mi"].tobytes() == r["mi"].tobytes()
    nmin = np.concatenate([np.minimum(oracle.map_sites(om, s[0])["norm"], oracle.map_sites(om, s[1])["norm"]) for s in sims])
    rel_close(rn["nmin"], nmin, 1e-6)


def test_the_output_table(eng):
    A, T, n, ncls = 61, 40, 37, 4
    aln = ref.columns(A, T, n, 21)
    o = ref.mi_columns(aln, None, A)
    r0 = mica.analysis(eng, aln, nalpha=A)
    avg, full = oracle.mica_average_mi(o["mi"])
    rel_close(r0["average_mi"], avg, 1e-6, 1e-12)
    assert abs(r0["full_average_mi"] - full) <= 1e-6 * full
    rel_close(r0["entropy"], o["h1"], 1e-9, 1e-12)
    ns, nk = mica.zscore_null(eng, r0["mi"], r0["entropy"], "MI")
    res = mica.analysis(eng, aln, nalpha=A, null=(ns, nk), nclasses=ncls)
    lines = formats.to_text(formats.write_mica, np.arange(1, n + 1), res).split("\n")
    assert lines[0] == "Group\tMI\tAPC\tRCW\tHjoint\tHmin\tBs.p.value\tBs.nb"
    assert len(lines) == n * (n - 1) // 2 + 2 and lines[1].startswith("[1;2]\t")


def test_refusals_and_the_untouched_paths(eng):
    a1, a2 = _inputs(61, 40, 9, 7)
    masks = np.full(64, 0xFFFFFFFF, dtype=np.uint32)
    for call in (lambda: eng.mi_columns(a1, a2, nalpha=61, masks=masks),
                 lambda: eng.mi_pairs(a1, [0, 1], [2, 3], None, nalpha=61, masks=masks)):
        with pytest.raises(engine.CmxError) as e:
            call()
        assert e.value.status == -2 and "ambiguity table" in str(e.value)           # CMX_ERR_UNSUPPORTED
    for bad in (1, 65):
        for call in (lambda: eng.mi_columns(a1, a2, nalpha=bad), lambda: eng.mi_pairs(a1, [0, 1], [2, 3], None, nalpha=bad)):
            with pytest.raises(engine.CmxError) as e:
                call()
            assert e.value.status == -1                                            # CMX_ERR_INVALID
    with pytest.raises(engine.CmxError) as e:
        eng.mica_permutation_test(a1, 10, 1, nalpha=61)
    assert e.value.status == -2
    # a wide call, a 20-state call, a wide call of another size, the 20-state call again: no scratch shared by name
    rng = np.random.default_rng(4)
    p1 = rng.integers(0, 20, size=(40, 33)).astype(np.uint8)
    p2 = rng.integers(0, 20, size=(40, 17)).astype(np.uint8)
    p1[3, ::5] = 20
    p2[7, ::3] = 25
    w = eng.mi_columns(a1, a2, nalpha=61)
    first = eng.mi_columns(p1, p2, nalpha=20)
    b1, b2 = _inputs(64, 65, 41, 23)
    w2 = eng.mi_columns(b1, b2, nalpha=64)
    second = eng.mi_columns(p1, p2, nalpha=20)
    for k in ("mi", "hjoint", "h1", "h2"):
        assert first[k].tobytes() == second[k].tobytes(), k
    _check(first, oracle.mi_columns(p1, p2, 20))
    _check(w, ref.mi_columns(a1, a2, 61))
    _check(w2, ref.mi_columns(b1, b2, 64))
    assert eng.mi_columns(a1, a2, nalpha=61)["mi"].tobytes() == w["mi"].tobytes()


@pytest.fixture(scope="module")
def guard():
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    engine.scratch_shrink(None, 0)
    yield
    engine.scratch_shrink(None, 0)
    engine.scratch_guard(was)


def test_under_the_scratch_guard(guard):
    g = engine.Engine()                                       # created under the guard: every buffer carries a canary
    a1, a2 = _inputs(61, 40, 31, 33)
    _check(g.mi_columns(a1, a2, nalpha=61), ref.mi_columns(a1, a2, 61))
    b = ref.columns(64, 40, 64, 5)
    _check(g.mi_columns(b, None, nalpha=64), ref.mi_columns(b, None, 64), intra=True)
    s1, s2 = _inputs(33, 40, 5, 3)                            # a smaller call after a larger one
    _check(g.mi_columns(s1, s2, nalpha=33), ref.mi_columns(s1, s2, 33))
    was = engine.mica_wide_plain(True)
    try:
        _check(g.mi_columns(a1, a2, nalpha=61), ref.mi_columns(a1, a2, 61))
    finally:
        engine.mica_wide_plain(was)
    rng = np.random.default_rng(6)
    i1, i2 = rng.integers(0, 31, size=37), rng.integers(0, 33, size=37)
    rel_close(g.mi_pairs(a1, i1, i2, a2, nalpha=61)["mi"], ref.mi_pairs(a1, i1, i2, 61, a2)["mi"], 1e-6, 1e-12)
    g.synchronize()
    g.scratch_check()
    assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
