"""The fused null's pattern table is tile-major: a mapping wave writes the counts of its patterns as one
[B*K][row] block, the pairs are scored from those blocks, and Correlation / Covariance are scored in one pass from
per-pattern moments.  The pattern path must still give the same bytes as mapping every site of every pair.  What
test_gpu_null_patterns.py does not pin: pattern counts at the edges of a tile, every statistic the fused null accepts, a
class-fused DNA model forced onto the pattern path, and a pass whose patterns fill less than one tile.  Every case once
more with a canary behind every scratch buffer."""
import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np
import pytest

from comap_amd import engine
from large_tree_cases import with_patterns
from test_gpu_null_patterns import KEYS, _both, _clean, _columns, _distinct, _dna, _protein, _supplied

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=[False, True], ids=["plain", "guard"])
def guard(request):
    if not request.param:
        yield False
        return
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    yield True
    engine.scratch_guard(was)


def _with_patterns(eng, npat, nrep, ram, seed):
    """[nrep][2][T][ram] alignments with exactly npat distinct columns (large_tree_cases.with_patterns, for this engine's
    taxa and states)"""
    return with_patterns(eng.T, eng.S, npat, nrep, ram, seed)


@pytest.mark.parametrize("npat", [1, 63, 64, 65, 150])
def test_pattern_counts_at_the_edges_of_a_tile(npat, guard):
    """a tile holds one mapping wave's patterns (64 for proteins): one pattern, one short of a tile, a whole tile, one over,
    and two tiles and a part"""
    eng = _protein()
    sup = _with_patterns(eng, npat, 2, 48, 100 + npat)
    assert _distinct(_columns(sup)) == npat
    for kind in (engine.STAT_CORRELATION, engine.STAT_COMPENSATION):     # the one-pass scoring and the generic one
        _, _, n = _both(eng, kind, 0, 0, 2, 48, supplied=sup)
        assert n == npat
    _clean(eng, guard)


KINDS = [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_COSUBSTITUTION, engine.STAT_COSINUS,
         engine.STAT_COVARIANCE, engine.STAT_DISCRETE_MI, engine.STAT_CORRECTED_CORRELATION, engine.STAT_EUCLIDIAN_DISTANCE,
         engine.STAT_SCALAR_PRODUCT]


@pytest.mark.parametrize("kind", KINDS)
def test_every_statistic_of_the_fused_null(kind, guard):
    """kinds 0 and 4 are scored from the per-pattern moments, the others by pair_stat_strided on the tiles"""
    eng = _protein()
    kw = {}
    if kind == engine.STAT_CORRECTED_CORRELATION:
        kw["mean_vectors"] = np.random.default_rng(2).uniform(0, 0.2, size=(2, eng.B))
    _, on, n = _both(eng, kind, 23, 1, 4, 101, **kw)                      # simulated: duplicates, 606 sites
    aln, _ = eng.simulate(23, 1 * 2 * 101, 3 * 2 * 101)
    assert n == _distinct(aln.T)
    assert np.isfinite(on["stat"]).any()
    sup = _with_patterns(eng, 171, 3, 37, 7)                              # supplied: 222 sites, two tiles and 43 patterns
    _, _, n = _both(eng, kind, 0, 0, 3, 37, supplied=sup, **kw)
    assert n == 171
    _clean(eng, guard)


@pytest.mark.parametrize("ncat", [4, 5])
def test_forced_on_fused_dna(ncat, guard):
    """class-fused nucleotide models (16 / 20 device states, cherry tables) take the per-site path unless told otherwise"""
    eng = _dna(16, ncat)
    assert eng.info()["device_states"] == 4 * ncat
    sup = _supplied(eng, 41, 3, 77)
    want = _distinct(_columns(sup))
    for kind in (engine.STAT_COVARIANCE, engine.STAT_EUCLIDIAN_DISTANCE, engine.STAT_CORRELATION):
        _, _, n = _both(eng, kind, 0, 0, 3, 77, supplied=sup)
        assert n == want
    few = _with_patterns(eng, 65, 2, 40, 3)
    _, _, n = _both(eng, engine.STAT_CORRELATION, 0, 0, 2, 40, supplied=few)
    assert n == 65
    _clean(eng, guard)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guard"])
def test_last_pass_smaller_than_a_tile(guarded):
    """CMX_NULL_PASS_BYTES for two replicates a pass: three replicates of 2 x 20 sites run as passes of 80 and 40 sites, the
    second under one tile; the same bytes as one pass (which _both compares with mapping every site)"""
    eng = _protein()
    nrep, ram = 3, 20
    sup = _supplied(eng, 29, nrep, ram)
    one = {kind: _both(eng, kind, 0, 0, nrep, ram, supplied=sup)[1] for kind in (engine.STAT_CORRELATION, engine.STAT_COSINUS)}
    # at least what the pattern path holds per site (counts, packed column, keys / indices / per-pattern scalars)
    per_rep = 2 * ram * (eng.B * eng.K * 8 + (eng.T + 15) // 16 * 16 + 84)
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        import torch
        sys.path.insert(0, %r + '/tests')
        from comap_amd import engine
        from test_gpu_null_patterns import _protein, _both, KEYS
        guarded = bool(int(sys.argv[3]))
        if guarded:
            engine.scratch_guard(True)
            engine.scratch_guard_failures(clear=True)
        eng = _protein()
        sup = np.load(sys.argv[1])
        out = {}
        for kind in (0, 3):
            r = _both(eng, kind, 0, 0, %d, %d, supplied=sup)
            out.update({"k%%d_%%s" %% (kind, k): r[1][k] for k in KEYS})
            out["n%%d" %% kind] = np.array(r[2])
        if guarded:
            eng.synchronize()
            eng.scratch_check()
            assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
        np.savez(sys.argv[2], **out)
    """ % (ROOT, ROOT, nrep, ram))
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "sup.npy"), sup)
        env = dict(os.environ, CMX_NULL_PASS_BYTES=str(2 * per_rep + per_rep // 2))
        subprocess.check_call([sys.executable, "-c", code, os.path.join(d, "sup.npy"), os.path.join(d, "out.npz"), str(int(guarded))],
                              env=env, cwd=ROOT)
        out = dict(np.load(os.path.join(d, "out.npz")))
    cols = _columns(sup)
    # the split shows in the count: deduplication stops at the pass boundary (replicates 0-1 | replicate 2), and columns
    # repeat across it; the last pass is 2 * ram = 40 sites, under one tile of 64
    per_pass = _distinct(cols[:2 * 2 * ram]) + _distinct(cols[2 * 2 * ram:])
    assert 2 * ram < 64 and per_pass > _distinct(cols)
    assert per_pass != _distinct(cols[:2 * ram]) + _distinct(cols[2 * ram:2 * 2 * ram]) + _distinct(cols[2 * 2 * ram:])   # not 1 + 1 + 1
    for kind in (0, 3):
        for k in KEYS:
            assert out["k%d_%s" % (kind, k)].tobytes() == one[kind][k].tobytes(), (kind, k)
        assert out["n%d" % kind] == per_pass
