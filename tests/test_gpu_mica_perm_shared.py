"""What the two families of Mica's permutation test share (cmx_mica_perm.h, the table cache and the launch order of
cmx_api_mica.cpp): the fixed-point table after its scratch buffer was re-created, 20 states at the taxon limit (no opening
pass: nperm is preset before either kernel), the shared device pieces at 4 states.  Comparisons are exact (bytes), against
the oracle; against the restatement of tests/mica_perm_reference.py where the oracle stops (it takes up to 31 states)."""
import numpy as np
import pytest

import oracle
import mica_perm_reference as ref
from comap_amd import engine

pytestmark = pytest.mark.gpu

SEED = 41


def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes(), (got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes()


def _with_unknowns(A, T, n, cols, seed):
    """independent columns, code A in a tenth of the cells of `cols`"""
    rng = np.random.default_rng(seed)
    aln = rng.integers(0, A, size=(T, n))
    hit = rng.random((T, n)) < 0.1
    hit[:, [c for c in range(n) if c not in cols]] = False
    aln[hit] = A
    assert all((aln[:, c] == A).any() for c in cols)
    return aln.astype(np.uint8)


def test_the_table_survives_a_recreated_buffer():
    """switching the scratch guard on after the first call re-creates every scratch buffer, perm_F / permw_F among them:
    the table has to be uploaded again although its key (entries, shift) still matches"""
    was = engine.scratch_guard(False)
    try:
        engine.scratch_guard_failures(clear=True)
        eng = engine.Engine()
        a20 = _with_unknowns(20, 30, 6, (3, 4, 5), 2030)
        a33 = _with_unknowns(33, 30, 6, (3, 4, 5), 3330)
        first20 = eng.mica_permutation_test(a20, 130, SEED, nalpha=20)
        first33 = eng.mica_permutation_test_states(a33, 130, SEED, 33)
        _same(first20, oracle.mica_permutation_test(a20, 20, 130, SEED))
        _same(first33, ref.permutation_test(a33, 33, 130, SEED)[:2])
        engine.scratch_guard(True)
        _same(eng.mica_permutation_test(a20, 130, SEED, nalpha=20), first20)
        _same(eng.mica_permutation_test_states(a33, 130, SEED, 33), first33)
        eng.synchronize()
        eng.scratch_check()
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
    finally:
        engine.scratch_guard(was)


@pytest.fixture(scope="module")
def eng():
    return engine.Engine()


def _at_the_limit(unknowns):
    T = 2047
    rng = np.random.default_rng(2047 + unknowns)
    aln = rng.integers(0, 20, size=(T, 4))
    aln[:, 1] = np.where(rng.random(T) < 0.9, aln[:, 0], aln[:, 1])
    if unknowns:
        aln[:, 2:][rng.random((T, 2)) < 0.1] = 20
    return aln.astype(np.uint8)


@pytest.mark.parametrize("unknowns", [0, 1])
def test_twenty_states_at_the_taxon_limit(eng, unknowns):
    """2 047 taxa: the opening pass does not fit the LDS at 20 states, every resolved pair starts at shuffle 0 from a
    preset nperm.  With unknowns in columns 2 and 3: one resolved pair and five of the general kernel, which runs between
    the preset and the resolved kernel -- neither may overwrite the other's pairs"""
    aln = _at_the_limit(unknowns)
    assert (aln == 20).any(axis=0).tolist() == [False, False, bool(unknowns), bool(unknowns)]
    want = oracle.mica_permutation_test(aln, 20, 70, SEED)
    assert (want[1] > 0).all()
    got = eng.mica_permutation_test(aln, 70, SEED, nalpha=20)
    _same(got, want)
    if unknowns:
        _same(eng.mica_permutation_test_states(aln, 70, SEED, 20, 1, 4), (got[0][1:4], got[1][1:4]))


def test_four_resolved_states_against_the_restatement(eng):
    """generator, pair numbering, stopping rule and final write are one copy for both families: the 4-state kernels
    against the restatement that the other alphabets are tested with"""
    aln = np.random.default_rng(433).integers(0, 4, size=(33, 8)).astype(np.uint8)
    _same(eng.mica_permutation_test(aln, 130, SEED, nalpha=4), ref.permutation_test(aln, 4, 130, SEED)[:2])
