"""-m gpu: the planned walk of the 64-site protein kernels (cmx_map.hip: leaf_begin, wait_planned_*; cmx_layout.h: wait plan,
PlanEntry) -- waits read from the stream entry, the operator at class block + entry offset, the entry from a
running pointer that is set at the pass boundary, the wrap to the next pass in the copy of the stream the pass reads.

The proof that no planned wait is too lax is the host's queue model (tests/test_wait_plan.py); a race that reads a stale
operator need not show in any run.  This file is the smoke check on the device: short passes (trees of 4, 5, 9 and 17 taxa:
a wrap every few ops) and the benchmark's 64-taxon tree once, C = 1 (every pass is its block's last) and C = 4 classes, on
an engine capped to ONE workgroup (cmx_debug_map_grid(1): four waves, so a wave maps block after block and the stream
state crosses block boundaries), block queue on and off, LDS slot planned and planned empty.

* observed mode, n in {1, 63, 64, 65, 200} sites and the 200 columns tiled to 600 (ten blocks on four waves).  With C = 4
  the reference is the 16-site class-split walk (map_kernel<20, split, 1, NG = 1>, which keeps the run-time count): an
  uncapped engine maps the 200 columns that way, and counts, logL, norm and rate class must be the same BYTES (post_rate:
  against the oracle only, as in test_gpu_mfma16_products.py -- the class-split launch rounds it differently).  At C = 4
  the capped engine itself takes n <= 64 to the 16-site walk (one block per class fits its four waves); n = 65, 200, 600
  run map_kernel<20, observed>.  With C = 1 there is no class-split launch: every n runs map_kernel<20, observed>, checked
  against the oracle and, as bytes, across queue and LDS slot.
* null mode and pattern mode, 3 replicates of rep_ram in {4, 68}: stat / nmin / prmin / rcmin the same bytes in the two
  modes and with and without the LDS slot, all against oracle.null_intra.

The 64-site class-split instantiation (map_kernel<20, split, 1, NG = 4>) reads the plan too, but no call reaches it: an
alignment small enough for the class-split launch is small enough for its 16-site shape (cmx_api_map.cpp: map_walk).
cmx_debug_map_small_blocks(0) keeps the 64-site blocks: with it the uncapped engine maps every n of the list through that
kernel, same bytes as the 16-site walk.  A wave of that launch maps ONE (block, class) task, so the operator its last op
requests for "the wave's next task" -- the stream copies with a class step other than +1 -- is fetched from inside MAT
and never read; which copy is read there is covered by the host's model of single-pass blocks only."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from lds_slot_trees import bench64
from test_gpu_parity import _check_map

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 200)
NCOLS, TILED = 200, 600
NREP, RAMS = 3, (4, 68)
BYTE_KEYS = ("counts", "logL", "norm", "rate_class")
NULL_KEYS = ("stat", "nmin", "prmin", "rcmin")

CASES = [(t, c) for c in (4, 1) for t in (4, 5, 9, 17)] + [(64, 4)]


def _tree(ntaxa):
    if ntaxa == 64:
        shape, blen = bench64()
        return shape.parent, blen, shape.lot
    parent, blen, lot = synthetic.random_tree(ntaxa, 300 + ntaxa)
    return parent, blen, lot


def _engine(args, workgroups, slot):
    was_g, was_s = engine.map_grid(workgroups), engine.lds_slot(slot)
    try:
        return engine.Engine(*args)
    finally:
        engine.map_grid(was_g)
        engine.lds_slot(was_s)


def _same_bytes(a, b, keys, what):
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


@pytest.mark.parametrize("ntaxa,C", CASES, ids=[f"taxa{t}-C{c}" for t, c in CASES])
def test_planned_walk(ntaxa, C):
    parent, blen, lot = _tree(ntaxa)
    mdl = synthetic.protein_model(0.5, C)
    args = (parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    om = oracle.Model(*args)
    cols, _ = oracle.simulate(om, 7 + ntaxa, 0, NCOLS)
    cols = np.ascontiguousarray(cols)
    want = oracle.map_sites(om, cols)
    capped = {slot: _engine(args, 1, slot) for slot in (True, False)}
    assert all(e.info()["waves"] == 4 for e in capped.values())
    ref = None
    if C > 1:                                   # the 16-site class-split walk: the run-time count
        short = _engine(args, 0, True)
        ref = short.map_sites(cols)
        _check_map(ref, want)
        # ... and the 64-site class-split walk, map_kernel<20, split, 1, NG = 4>, which reads the plan: reached only with the
        # 16-site blocks switched off (every wave maps one (block, class) task: each pass is its block's last)
        was_16 = engine.map_small_blocks(False)
        try:
            for n in SIZES:
                g = short.map_sites(np.ascontiguousarray(cols[:, :n]))
                _check_map(g, {k: v[:n] for k, v in want.items()})
                _same_bytes(g, {k: np.ascontiguousarray(np.asarray(ref[k])[:n]) for k in BYTE_KEYS}, BYTE_KEYS, (n, "64-site class-split walk"))
        finally:
            engine.map_small_blocks(was_16)
        short.synchronize()
        short.close()
    tiled = np.arange(TILED) % NCOLS
    was_q = engine.map_queue()
    try:
        for n in SIZES + (TILED,):
            idx = tiled[:n]
            aln = np.ascontiguousarray(cols[:, idx])
            got = {}
            for slot in (True, False):
                for queue in (True, False):
                    engine.map_queue(queue)
                    got[slot, queue] = g = capped[slot].map_sites(aln)
                    _check_map(g, {k: v[idx] for k, v in want.items()})
                    if ref is not None:
                        _same_bytes(g, {k: np.ascontiguousarray(np.asarray(ref[k])[idx]) for k in BYTE_KEYS}, BYTE_KEYS, (n, slot, queue, "16-site walk"))
            first = got[True, True]
            for key, g in got.items():
                _same_bytes(g, first, BYTE_KEYS + ("post_rate",), (n, key, "queue / LDS slot"))
        # ---- nulls: per site (map_kernel<20, null>) and per distinct pattern (map_kernel<20, patterns>)
        engine.map_queue(True)
        for ram in RAMS:
            seed = 11 + ram
            o = oracle.null_intra(om, engine.STAT_CORRELATION, seed, 0, NREP, ram)
            got = {}
            for slot in (True, False):
                for patterns in (False, True):
                    capped[slot].set_null_patterns(patterns)
                    got[slot, patterns] = g = capped[slot].null_intra(engine.STAT_CORRELATION, seed, 0, NREP, ram)
                    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
                    rel_close(g["nmin"], o["nmin"], 1e-6)
                    rel_close(g["prmin"], o["prmin"], 1e-9)
                    assert np.array_equal(g["rcmin"], o["rcmin"])
            for patterns in (False, True):     # the LDS slot changes nothing
                _same_bytes(got[False, patterns], got[True, patterns], NULL_KEYS, (ram, patterns, "LDS slot"))
            for slot in (True, False):         # null mode and pattern mode: the same bytes in every output
                _same_bytes(got[slot, True], got[slot, False], NULL_KEYS, (ram, slot, "null mode / pattern mode"))
    finally:
        engine.map_queue(was_q)
        for e in capped.values():
            e.synchronize()
            e.close()
