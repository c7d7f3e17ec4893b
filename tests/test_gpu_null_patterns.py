"""The fused null maps each distinct simulated column once (cmx_set_null_patterns): a column's counts, norm,
posterior rate and rate class depend on the column alone, so a duplicate takes its first occurrence's results and the pairs
are scored from a table of patterns.  The pattern path must give the same bytes as mapping every site of every pair.

Everything rests on per-site results not depending on the lane and wave a site lands on: the first tests map one null and
the same null with its columns rotated by 1 .. 63 and compare the bytes."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from comap_amd import engine, synthetic
from tree_shapes import _balanced

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("stat", "rcmin", "prmin", "nmin")


def _protein(ntaxa=24, seed=20260101):
    parent, blen, lot = synthetic.random_tree(ntaxa, seed)
    mdl = synthetic.protein_model(0.5, 4)
    return engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])


def _dna(ntaxa=16, ncat=4):
    parent, lot = _balanced(ntaxa)
    blen = np.maximum(np.random.default_rng(ntaxa).exponential(0.1, size=len(parent)), 1e-6)
    blen[-1] = 0.0
    mdl = synthetic.dna_model(0.7, ncat)
    return engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])


def _supplied(eng, seed, nrep, ram):
    """[nrep][2][T][ram] alignments from the engine's own simulator (the null's draws, g = (rep * 2 + h) * ram + j)"""
    aln, _ = eng.simulate(seed, 0, nrep * 2 * ram)
    return np.ascontiguousarray(aln.reshape(eng.T, nrep, 2, ram).transpose(1, 2, 0, 3))


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("model", ["protein", "dna"])
def test_per_site_results_do_not_depend_on_the_lane(model):
    eng = _protein() if model == "protein" else _dna()
    ram = 192
    sup = _supplied(eng, 11, 1, ram)
    base = eng.null_intra(engine.STAT_CORRELATION, 0, 0, 1, ram, supplied=sup)
    for k in range(1, 64):
        got = eng.null_intra(engine.STAT_CORRELATION, 0, 0, 1, ram, supplied=np.ascontiguousarray(np.roll(sup, k, axis=-1)))
        for key in KEYS:
            assert np.array_equal(got[key], np.roll(base[key], k), equal_nan=True), (k, key)


@pytest.fixture(params=[False, True], ids=["plain", "guard"])
def guard(request):
    """every case once more with a canary behind every scratch buffer (contexts created inside the test)"""
    if not request.param:
        yield False
        return
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    yield True
    engine.scratch_guard(was)


def _clean(eng, guard):
    if guard:
        eng.synchronize()
        eng.scratch_check()
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()


def _distinct(cols):
    """distinct columns of [n][T] uint8 rows"""
    return len(np.unique(np.ascontiguousarray(cols), axis=0))


def _columns(sup):
    """[nrep][2][T][ram] -> the columns of sites g = (rep * 2 + h) * ram + j, one row each"""
    return sup.transpose(0, 1, 3, 2).reshape(-1, sup.shape[2])


def _both(eng, *args, **kw):
    """the null with patterns off and on: (off, on, patterns mapped with them on)"""
    eng.set_null_patterns(False)
    off = eng.null_intra(*args, **kw)
    assert eng.null_pattern_count() == 2 * len(off["stat"])
    eng.set_null_patterns(True)
    on = eng.null_intra(*args, **kw)
    n = eng.null_pattern_count()
    eng.set_null_patterns(None)
    for k in KEYS:
        assert off[k].tobytes() == on[k].tobytes(), k
    return off, on, n


@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_DISCRETE_MI,
                                  engine.STAT_CORRECTED_CORRELATION, engine.STAT_EUCLIDIAN_DISTANCE])
def test_protein_null_patterns_give_the_same_bytes(kind, guard):
    eng = _protein()
    kw = {}
    if kind == engine.STAT_CORRECTED_CORRELATION:
        kw["mean_vectors"] = np.random.default_rng(1).uniform(0, 0.2, size=(2, eng.B))
    rb, re, ram = 3, 8, 150
    _, _, n = _both(eng, kind, 7, rb, re, ram, **kw)                      # the null simulates for itself
    aln, _ = eng.simulate(7, rb * 2 * ram, (re - rb) * 2 * ram)
    assert n == _distinct(aln.T) < 2 * (re - rb) * ram
    sup = _supplied(eng, 9, 4, 96)
    _, _, n = _both(eng, kind, 0, 0, 4, 96, supplied=sup, **kw)          # supplied alignments
    assert n == _distinct(_columns(sup))
    _clean(eng, guard)


@pytest.mark.parametrize("ncat", [4, 5])
def test_fused_dna_with_cherry_tables(ncat, guard):
    eng = _dna(16, ncat)
    info = eng.info()
    assert info["device_states"] == 4 * ncat and info["cherry_tables"] > 0
    sup = _supplied(eng, 5, 3, 53)
    _, _, n = _both(eng, engine.STAT_CORRELATION, 0, 0, 3, 53, supplied=sup)
    assert n == _distinct(_columns(sup))
    _, _, n = _both(eng, engine.STAT_COMPENSATION, 11, 1, 4, 70)
    aln, _ = eng.simulate(11, 1 * 2 * 70, 3 * 2 * 70)
    assert n == _distinct(aln.T)
    _clean(eng, guard)


@pytest.mark.parametrize("case", ["identical", "distinct", "one_replicate", "ragged"])
def test_supplied_alignments(case, guard):
    eng = _protein()
    rng = np.random.default_rng(3)
    nrep, ram = {"identical": (3, 64), "distinct": (3, 80), "one_replicate": (1, 77), "ragged": (5, 101)}[case]
    if case == "identical":
        col = rng.integers(0, 20, size=eng.T, dtype=np.uint8)
        sup = np.ascontiguousarray(np.broadcast_to(col[None, None, :, None], (nrep, 2, eng.T, ram)))
    elif case == "distinct":
        sup = rng.integers(0, 20, size=(nrep, 2, eng.T, ram), dtype=np.uint8)
    else:
        sup = _supplied(eng, 21, nrep, ram)
    _, _, n = _both(eng, engine.STAT_CORRELATION, 0, 0, nrep, ram, supplied=sup)
    want = _distinct(_columns(sup))
    assert n == want
    if case == "identical":
        assert n == 1
    if case == "distinct":
        assert n == 2 * nrep * ram
    _clean(eng, guard)


@pytest.mark.parametrize("bits", [1, 5])
def test_truncated_hash_costs_deduplication_only(bits, guard):
    eng = _protein()
    sup = _supplied(eng, 31, 4, 90)
    was = engine.null_hash_bits(bits)
    try:
        _, _, n = _both(eng, engine.STAT_CORRELATION, 0, 0, 4, 90, supplied=sup)
        _, _, n2 = _both(eng, engine.STAT_COMPENSATION, 13, 0, 3, 70)
    finally:
        engine.null_hash_bits(was)
    assert n >= _distinct(_columns(sup))
    aln, _ = eng.simulate(13, 0, 3 * 2 * 70)
    assert n2 >= _distinct(aln.T)
    _clean(eng, guard)


def test_pass_boundary():
    """CMX_NULL_PASS_BYTES below the pattern scratch of the null: passes of two replicates (2, 2, 1), no pair straddles
    one, deduplication inside each pass; the same bytes as one pass and as mapping every site"""
    eng = _protein()
    nrep, ram = 5, 45
    sup = _supplied(eng, 17, nrep, ram)
    one = [_both(eng, engine.STAT_CORRELATION, 0, 0, nrep, ram, supplied=sup)[1],
           _both(eng, engine.STAT_CORRELATION, 19, 2, 2 + nrep, ram)[1]]
    per_rep = 2 * ram * (eng.B * eng.K * 8 + (eng.T + 15) // 16 * 16 + 68)
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        import torch
        sys.path.insert(0, %r + '/tests')
        from test_gpu_null_patterns import _protein, _both, KEYS
        eng = _protein()
        sup = np.load(sys.argv[1])
        a = _both(eng, 0, 0, 0, %d, %d, supplied=sup)
        b = _both(eng, 0, 19, 2, 2 + %d, %d)
        np.savez(sys.argv[2], n=np.array([a[2], b[2]]), **{"a_" + k: a[1][k] for k in KEYS}, **{"b_" + k: b[1][k] for k in KEYS})
    """ % (ROOT, ROOT, nrep, ram, nrep, ram))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "sup.npy"), sup)
        env = dict(os.environ, CMX_NULL_PASS_BYTES=str(2 * per_rep + per_rep // 2))
        subprocess.check_call([sys.executable, "-c", code, os.path.join(d, "sup.npy"), os.path.join(d, "out.npz")], env=env, cwd=ROOT)
        out = dict(np.load(os.path.join(d, "out.npz")))
    for k in KEYS:
        assert out["a_" + k].tobytes() == one[0][k].tobytes(), k
        assert out["b_" + k].tobytes() == one[1][k].tobytes(), k
    cols = _columns(sup)
    aln, _ = eng.simulate(19, 2 * 2 * ram, nrep * 2 * ram)
    for i, c in enumerate([cols, aln.T]):
        per_pass = sum(_distinct(c[r0 * 2 * ram:min(nrep, r0 + 2) * 2 * ram]) for r0 in range(0, nrep, 2))
        assert out["n"][i] == per_pass >= _distinct(c)
