"""Mica's permutation test (null.method = permutations, miTest CoMap/Mica.cpp:93-118) for alphabets of 2 .. 64 states,
cmx_mica_perm_wide.hip behind cmx_mica_permutation_test_states: both paths (resolved pairs, pairs with unknowns), every
stopping class, the pair range, 4 / 20 states through the new entry, the refusals, the call history, the scratch guard, the
output table.  Comparisons are exact (bytes): the yardstick is the restatement of tests/mica_perm_reference.py (pinned to the
oracle by tests/test_mica_perm_reference.py), and the oracle itself up to 31 states."""
import functools

import numpy as np
import pytest

import oracle
import mica_perm_reference as ref
from comap_amd import engine, formats, mica

pytestmark = pytest.mark.gpu

SEED = 41
# (A, T, n, max_perm).  (63, 97): sh = 39; (64, 256): sh = 38; (64, 2): the smallest T, 63 is a state; (61, 41, 4, 1): one
# shuffle, T no multiple of 4; (64, 2047): the taxon limit, sh = 35, one resolved pair and two with unknowns
SHAPES = [(2, 33, 12, 130), (7, 30, 14, 200), (31, 40, 12, 130), (32, 40, 12, 130), (33, 65, 12, 130), (61, 40, 14, 130),
          (63, 97, 7, 70), (64, 256, 7, 70), (64, 2, 4, 20), (61, 41, 4, 1), (64, 2047, 3, 70)]
# input seeds are 1000 A + T, but for: with that seed no resolved pair of the shapes with A >= 32 stopped between 64 shuffles
# and the maximum (found with the restatement, on the CPU)
SEEDS = {(32, 40): 1000 * 32 + 40 + 5, (33, 65): 1000 * 33 + 65 + 9, (61, 40): 1000 * 61 + 40 + 11}


def _aln(A, T, n):
    return ref.columns(A, T, n, SEEDS.get((A, T), 1000 * A + T))


@functools.lru_cache(maxsize=None)
def _expected(A, T, n, max_perm):
    """the restatement's answer, computed once and shared (read only)"""
    pv, nb, gen = ref.permutation_test(_aln(A, T, n), A, max_perm, SEED)
    for x in (pv, nb, gen):
        x.setflags(write=False)
    return pv, nb, gen


@pytest.fixture(scope="module")
def eng():
    return engine.Engine()


def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes(), (got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes()


@pytest.mark.parametrize("A,T,n,max_perm", SHAPES)
def test_parity_with_the_restatement(eng, A, T, n, max_perm):
    aln = _aln(A, T, n)
    want = _expected(A, T, n, max_perm)
    _same(eng.mica_permutation_test_states(aln, max_perm, SEED, A), want)
    if A <= 31:
        _same(oracle.mica_permutation_test(aln, A, max_perm, SEED), want)
    if A == 64 and T == 2047:
        assert want[2].tolist() == [True, True, False] and (want[1] > 0).all()


def _classes(nb, gen, max_perm):
    """pairs per path (resolved, with unknowns) and stopping class: constant, < 16, 16 .. 63, 64 .. max - 1, = max"""
    out = np.zeros((2, 5), dtype=int)
    for g in (0, 1):
        x = nb[gen == bool(g)]
        full = x == max_perm
        out[g] = [(x == 0).sum(), ((x > 0) & (x < 16) & ~full).sum(), ((x >= 16) & (x < 64) & ~full).sum(), ((x >= 64) & ~full).sum(),
                  full.sum()]
    return out


def test_the_inputs_reach_every_path_and_stopping_class():
    total, wide = np.zeros((2, 5), dtype=int), np.zeros((2, 5), dtype=int)
    for A, T, n, max_perm in SHAPES:
        _, nb, gen = _expected(A, T, n, max_perm)
        c = _classes(nb, gen, max_perm)
        total += c
        if A >= 32:
            wide += c
    assert (total >= 3).all(), total
    assert (wide >= 1).all(), wide


def test_pair_ranges_concatenate_to_the_full_call(eng):
    A, T, n, max_perm = 61, 40, 14, 130
    aln = _aln(A, T, n)
    full = eng.mica_permutation_test_states(aln, max_perm, SEED, A)
    _same(full, _expected(A, T, n, max_perm))
    npairs = n * (n - 1) // 2
    parts = [eng.mica_permutation_test_states(aln, max_perm, SEED, A, b, e) for b, e in ((0, 17), (17, 18), (18, npairs))]
    assert [len(p[0]) for p in parts] == [17, 1, npairs - 18]
    _same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), full)
    _same(eng.mica_permutation_test_states(aln, max_perm, SEED, A, 18, None), (full[0][18:], full[1][18:]))


def test_device_entry_with_a_padded_leading_dimension(eng):
    import ctypes
    import torch
    A, T, n, max_perm = 61, 40, 14, 130
    want = _expected(A, T, n, max_perm)
    dev = torch.device("cuda", eng.device)
    d = torch.full((T, n + 3), 9, dtype=torch.uint8, device=dev)
    d[:, :n] = torch.from_numpy(_aln(A, T, n)).to(dev)
    b, e = 5, 40
    pv = torch.full((e - b + 2,), -7.0, dtype=torch.float64, device=dev)
    nb = torch.full((e - b + 2,), -7, dtype=torch.int32, device=dev)
    eng._check(eng._lib.cmx_mica_permutation_test_states_dev(eng._ctx, A, T, engine._vp(d), engine._sz(n), engine._sz(n + 3),
                                                             ctypes.c_uint32(max_perm), ctypes.c_uint64(SEED), engine._sz(b), engine._sz(e),
                                                             engine._vp(pv), engine._vp(nb), eng._stream()))
    torch.cuda.synchronize()
    pv, nb = pv.cpu().numpy(), nb.cpu().numpy()
    _same((pv[:e - b], nb[:e - b]), (want[0][b:e], want[1][b:e]))
    assert (pv[e - b:] == -7.0).all() and (nb[e - b:] == -7).all()


@pytest.mark.parametrize("A", [20, 4])
def test_four_and_twenty_states_through_the_new_entry(eng, A):
    aln = ref.columns(A, 40, 9, 1000 * A + 40)
    assert (aln[:, :3] >= A).any()
    old = eng.mica_permutation_test(aln, 130, SEED, nalpha=A, masks=None)
    _same(eng.mica_permutation_test_states(aln, 130, SEED, A), old)
    _same(eng.mica_permutation_test_states(aln, 130, SEED, A, 7, 31), (old[0][7:31], old[1][7:31]))
    _same(ref.permutation_test(aln, A, 130, SEED)[:2], old)


def test_refusals(eng):
    aln = _aln(61, 40, 14)

    def status(call):
        with pytest.raises(engine.CmxError) as e:
            call()
        return e.value.status

    for bad in (1, 65):
        assert status(lambda: eng.mica_permutation_test_states(aln, 10, 1, bad)) == -1         # CMX_ERR_INVALID
    assert status(lambda: eng.mica_permutation_test_states(np.zeros((2048, 3), dtype=np.uint8), 10, 1, 61)) == -2   # CMX_ERR_UNSUPPORTED
    assert status(lambda: eng.mica_permutation_test_states(aln[:1], 10, 1, 61)) == -2
    assert status(lambda: eng.mica_permutation_test_states(aln, 0, 1, 61)) == -1
    assert status(lambda: eng.mica_permutation_test_states(aln, 10, 1, 61, 5, 5)) == -1          # an empty pair range
    assert status(lambda: eng.mica_permutation_test_states(aln, 10, 1, 61, 0, 92)) == -1         # one pair past the end
    with pytest.raises(engine.CmxError) as e:
        eng.mica_permutation_test(aln, 10, 1, nalpha=61)                                       # the old entry is as it was
    assert e.value.status == -2 and "cmx_mica_permutation_test_states" in str(e.value)


def test_call_history(eng):
    """a 61-state call, a 20-state call with partial ambiguity codes, a 64-state call of another length, then the first two
    again: no scratch buffer or table key is shared by name"""
    A, T, n, max_perm = 61, 40, 14, 130
    a61 = _aln(A, T, n)
    rng = np.random.default_rng(12)
    a20 = rng.integers(0, 20, size=(40, 11)).astype(np.uint8)
    a20[:, 1] = np.where(rng.random(40) < 0.5, a20[:, 0], a20[:, 1])
    a20[rng.random((40, 11)) < 0.06] = 20                   # B-like: two states
    a20[rng.random((40, 11)) < 0.04] = 21                   # three states
    a20[rng.random((40, 11)) < 0.04] = 22                   # X
    masks = oracle.default_masks(20)[:23].copy()
    masks[20], masks[21] = (1 << 2) | (1 << 11), (1 << 5) | (1 << 6) | (1 << 13)
    first61 = eng.mica_permutation_test_states(a61, max_perm, SEED, A)
    first20 = eng.mica_permutation_test(a20, 130, 7, nalpha=20, masks=masks)
    other = eng.mica_permutation_test_states(_aln(64, 256, 7), 70, SEED, 64)
    _same(eng.mica_permutation_test_states(a61, max_perm, SEED, A), first61)
    _same(eng.mica_permutation_test(a20, 130, 7, nalpha=20, masks=masks), first20)
    _same(first61, _expected(A, T, n, max_perm))
    _same(other, _expected(64, 256, 7, 70))
    _same(first20, oracle.mica_permutation_test(a20, 20, 130, 7, masks=masks))


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
    big = ref.columns(61, 40, 31, 61040)
    _same(g.mica_permutation_test_states(big, 130, SEED, 61), ref.permutation_test(big, 61, 130, SEED)[:2])
    small = ref.columns(33, 40, 5, 33040)                     # a smaller call after a larger one
    _same(g.mica_permutation_test_states(small, 130, SEED, 33), ref.permutation_test(small, 33, 130, SEED)[:2])
    g.synchronize()
    g.scratch_check()
    assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()


def test_the_output_table(eng):
    A, T, n, max_perm = 61, 40, 14, 130
    aln = _aln(A, T, n)
    res = mica.analysis(eng, aln, nalpha=A, permutations=(max_perm, SEED))
    pv, nb, _ = _expected(A, T, n, max_perm)
    iu = np.triu_indices(n, 1)
    assert res["perm_pvalue"][iu].tobytes() == pv.tobytes() and res["perm_nb"][iu].tobytes() == nb.tobytes()
    lines = formats.to_text(formats.write_mica, np.arange(1, n + 1), res).split("\n")
    assert lines[0].endswith("Perm.p.value\tPerm.nb")
    assert len(lines) == n * (n - 1) // 2 + 2 and lines[1].startswith("[1;2]\t")
