"""-m gpu: the mapping walk's LDS slot (cmx_walk.h kLdsSlot) on the device.

An LDS copy is exact, so with the slot planned (the default) every output must be the same BYTES as with the slot switched
off (engine.lds_slot(False): every workspace vector through HBM) in the same process, and both must agree with the oracle
within the tolerances of test_gpu_tiny_trees (no branch lengths are equal here, so no site has the degenerate centred vector
that module makes an allowance for: the plain tolerances hold everywhere).  Trees: lds_slot_trees.py (the smallest tree with a two-visited node, nested
and disjoint intervals, trifurcating roots) and the benchmark's 64-taxon tree; protein Gamma-4, K = 1 and K = 2.

* observed mapping of 8 256 sites with one ambiguous symbol and a gap: 129 blocks of 64 sites x 4 classes are more than
  the 512 wave-tasks up to which the class-split launches (16-site blocks, no slot) take an observed alignment, so this
  is map_kernel<20, observed>.  The columns repeat with period 192: the oracle maps the 192 distinct ones.
* the per-site null and the pattern null, 3 replicates x 70 sites (the last block of each is partial)."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from lds_slot_trees import bench64, hand_built
from test_gpu_parity import _check_map

pytestmark = pytest.mark.gpu

NSITES, PERIOD = 8256, 192
NREP, RAM = 3, 70
_B64 = bench64()
TREES = [(s, None) for s in hand_built() if s.name in ("root6", "nested9", "disjoint9", "unrooted9")] + [_B64]
IDS = [s.name for s, _ in TREES]


def _bk(Q):
    W1 = np.random.default_rng(4).uniform(-1, 1, size=Q.shape)
    return np.stack([synthetic.weighted_register(Q, W1), synthetic.weighted_register(Q, np.abs(W1))])


def _setup(shape, blen, K):
    """-> (oracle model, engine arguments, kind of the null statistic)"""
    mdl = synthetic.protein_model(0.5, 4)
    if blen is None:
        blen = np.random.default_rng(shape.nn).uniform(0.05, 0.4, size=shape.nn)
        blen[-1] = 0.0
    Bk = None if K == 1 else _bk(mdl["Q"])
    kw = {} if Bk is None else dict(Bk=Bk)
    args = (shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    om = oracle.Model(*args, nonneg=Bk is None, **kw)
    return om, (args, dict(clamp_negative=Bk is None, **kw)), (engine.STAT_CORRELATION if K == 1 else engine.STAT_COMPENSATION)


def _engine(eargs, slot):
    was = engine.lds_slot(slot)
    try:
        return engine.Engine(*eargs[0], **eargs[1])
    finally:
        engine.lds_slot(was)


def _columns(om, shape, seed):
    """192 distinct columns: 150 simulated, 42 uniform random, one ambiguous symbol (B = D or N) and one gap among them"""
    sim, _ = oracle.simulate(om, seed, 0, 150)
    rnd = np.random.default_rng(seed).integers(0, 20, size=(shape.ntaxa, PERIOD - 150)).astype(np.uint8)
    cols = np.ascontiguousarray(np.concatenate([sim, rnd], axis=1))
    cols[seed % shape.ntaxa, 3] = 20
    cols[(seed + 2) % shape.ntaxa, 160] = 21
    return cols


def _same_bytes(a, b, what):
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


def _run(shape, blen, K):
    om, eargs, kind = _setup(shape, blen, K)
    on, off = _engine(eargs, True), _engine(eargs, False)
    masks = oracle.default_masks(20)
    masks[20] = (1 << 3) | (1 << 2)
    cols = _columns(om, shape, 11 + K)
    aln = np.ascontiguousarray(cols[:, np.arange(NSITES) % PERIOD])
    # ---- observed
    g_on, g_off = on.map_sites(aln, masks=masks[:22]), off.map_sites(aln, masks=masks[:22])
    _same_bytes(g_on, g_off, "observed")
    o = oracle.map_sites(om, cols, masks)
    rep = np.arange(NSITES) % PERIOD
    _check_map(g_on, {k: v[rep] for k, v in o.items()})
    # ---- nulls: per site, then per distinct pattern
    seed = 5 + K
    want = oracle.null_intra(om, kind, seed, 0, NREP, RAM)
    for patterns in (False, True):
        on.set_null_patterns(patterns)
        off.set_null_patterns(patterns)
        n_on, n_off = on.null_intra(kind, seed, 0, NREP, RAM), off.null_intra(kind, seed, 0, NREP, RAM)
        _same_bytes(n_on, n_off, "pattern null" if patterns else "per-site null")
        rel_close(n_on["stat"], want["stat"], 1e-6, 1e-12)
        rel_close(n_on["nmin"], want["nmin"], 1e-6)
        rel_close(n_on["prmin"], want["prmin"], 1e-9)
        assert np.array_equal(n_on["rcmin"], want["rcmin"])
    on.synchronize()
    off.synchronize()
    on.close()
    off.close()


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("shape,blen", TREES, ids=IDS)
def test_slot_on_equals_slot_off_and_the_oracle(shape, blen, K):
    info = engine.debug_walk(*_setup(shape, blen, K)[1][0])
    assert info["lds_loads"] > 0 and info["lds_stores"] > 0          # the tree has something to keep on chip
    _run(shape, blen, K)


def test_under_the_scratch_guard():
    """nested9, K = 1, every buffer followed by a canary: the slot's transfers leave HBM alone and nothing else moved"""
    shape = [s for s, _ in TREES if s.name == "nested9"][0]
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    try:
        _run(shape, None, 1)
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
    finally:
        engine.scratch_guard(was)
        engine.scratch_guard_failures(clear=True)
