"""No GPU: the integer thresholds of the null's LDS simulator (HostModel::simtab, cmx_layout.h) against the running sums.

The simulators draw a node's state as draw_guided does (cmx_simulate.hip): from the guide entry of u's 32nd on, count the
running sums with u >= cum[j] until one fails or S - 1 is reached, u = w / 2^32 of a 32-bit word w.  The LDS kernel
counts the thresholds of the row below w instead, from the same guide entry on, with no test for the row's end.  Checked:
* a threshold is t = ceil(cum * 2^32) - 1, kept inside 32 bits, and  "w > t  <=>  w / 2^32 >= cum"  for every w where the
  sum is positive -- at the words next to the threshold, where the two sides could part (both are monotone in w), and at
  0 and 2^32 - 1; a row's thresholds are the running maximum of those;
* the last sum of a row and the padding are 2^32 - 1 (never exceeded: the count stops at S - 1 by itself);
* a sum <= 0 in front of a row, which no threshold can stand for (every w counts it), lies in front of every guide entry;
* the count of the thresholds equals draw_guided's scan of the sums, for random words, the words at both ends, at the
  guide's steps and next to a sample of the thresholds;
* the guide bytes of a node's block are the gather kernel's, and the blocks follow the layout of cmx_layout.h.
Trees with branches of length 0 (sums of exactly 0 and 1, some an ulp out of order), 1e-9, 1e-12 (sums within 2^-32 of 0
and 1), 60 and ordinary ones; protein models of 4 and 6 classes; nucleotides get no blocks.
Which models get blocks at all is one rule, more than four states and a node block of at most 24 576 bytes: models on both
sides of it, 20 states with 8 / 9 / 10 classes and 61 with 1 / 2 among them, and the size of the blocks."""
import os

import numpy as np
import pytest

import model_sets as ms
from comap_amd import engine, protein_models as pm, synthetic
from tree_shapes import _balanced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def _tables(ncat, nstates=20):
    parent, lot = _balanced(8)
    blen = np.array([0.0, 1e-9, 60.0, 0.3, 0.0, 1e-12, 1e-9, 0.2, 60.0, 0.0, 0.1, 1e-12, 0.7, 2.5, 0.0])
    mdl = synthetic.protein_model(0.5, ncat) if nstates == 20 else synthetic.dna_model(0.5, ncat)
    return engine.debug_sim_tables(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"]), len(parent)


@pytest.mark.parametrize("ncat", [4, 6])
def test_thresholds_stand_for_the_running_sums(ncat):
    t, nn = _tables(ncat)
    S = 20
    thr = t["thresholds"]                                    # [nn, C, S, R]
    R = t["row"]                                             # cmx_layout.h: sim_thr_row(S), S + kSimThrPad rounded up to 4
    assert R >= S + 4 and R % 4 == 0 and thr.shape == (nn, ncat, S, R) and thr.dtype == np.uint32
    cum = t["cum"].transpose(1, 0, 2, 3)[: nn - 1]           # [node, C, S, S]; the root has no branch
    assert np.array_equal(t["block_guide"][: nn - 1], t["guide"].transpose(1, 0, 2, 3)[: nn - 1])
    assert np.all(thr[: nn - 1, :, :, S - 1:] == 0xFFFFFFFF)
    c = cum[..., : S - 1]
    th = thr[: nn - 1, :, :, : S - 1].astype(np.int64)
    each = np.clip(np.ceil(np.ldexp(c, 32)) - 1.0, 0.0, 4294967295.0).astype(np.int64)
    assert np.array_equal(th, np.maximum.accumulate(each, axis=-1))
    pos = c > 0.0
    assert pos.sum() > 0 and (~pos).sum() > 0 and (c >= 1.0).sum() > 0      # the edges are in the tables
    assert (np.diff(c, axis=-1) < 0).sum() > 0                              # ... and sums out of order
    for w in (each - 1, each, each + 1, each + 2, np.zeros_like(each), np.full_like(each, 0xFFFFFFFF)):
        w = np.clip(w, 0, 0xFFFFFFFF)
        by_sum = w.astype(np.float64) / 4294967296.0 >= c     # (exact: w < 2^32, a power-of-two divisor)
        assert np.array_equal(by_sum[pos], (w > each)[pos])
    # leading sums <= 0: every guide entry (k = 0 .. 31) already stands behind them
    lead = np.cumprod(~pos, axis=-1).sum(axis=-1)
    assert lead.max() > 0 and np.all(t["block_guide"][: nn - 1].min(axis=-1) >= lead)
    # the count itself: thresholds below w from the guide entry on == draw_guided's scan of the sums
    rng = np.random.default_rng(5)
    near = rng.choice(th.ravel(), size=200)
    ws = np.concatenate([rng.integers(0, 1 << 32, size=64), [0, 1, (1 << 32) - 2, (1 << 32) - 1],
                         np.arange(1, 32) << 27, (np.arange(1, 32) << 27) - 1, near - 1, near, near + 1, near + 2])
    j = np.arange(S - 1)
    for w in np.unique(np.clip(ws, 0, 0xFFFFFFFF)).astype(np.int64):
        start = t["block_guide"][: nn - 1, :, :, w >> 27].astype(np.int64)
        fails = ~(w / 4294967296.0 >= c) & (j >= start[..., None])
        want = np.where(fails.any(axis=-1), fails.argmax(axis=-1), np.maximum(start, S - 1))
        got = start + ((w > th) & (j >= start[..., None])).sum(axis=-1)
        assert np.array_equal(got, want), int(w)


def test_nucleotides_get_no_blocks():
    t, _ = _tables(4, nstates=4)
    assert t["thresholds"] is None and t["cum"].shape[-1] == 4


# (states, classes) with a node block of at most kSimNodeBytesMax = 24 576 bytes and more than four states -- the one rule
# for "this model has simulator tables" (cmx_layout.h: sim_has_tables) -- and without
WITH_BLOCKS = [(20, 8), (20, 9), (61, 1), (64, 1), (16, 13)]
WITHOUT_BLOCKS = [(4, 4), (20, 10), (61, 2), (7, 50), (5, 62), (14, 16)]


@pytest.mark.parametrize("S,C", WITH_BLOCKS + WITHOUT_BLOCKS)
def test_which_models_get_blocks(S, C):
    parent, lot = _balanced(4)
    nn = len(parent)
    blen = np.array([0.1, 0.0, 0.4, 1e-9, 0.2, 0.3, 0.0])
    Qs, pis = ms._generators(S, 7)
    rates, probs = pm.gamma_rates(0.6, C)
    t = engine.debug_sim_tables(parent, blen, lot, Qs[0], pis[0], rates, probs)
    row = (S + 4 + 3) // 4 * 4
    assert t["row"] == row
    if (S, C) in WITH_BLOCKS:
        assert t["blocks_bytes"] == nn * C * S * (4 * row + 32) > 0
        assert t["blocks_bytes"] // nn <= 24576
        assert t["thresholds"].shape == (nn, C, S, row) and t["block_guide"].shape == (nn, C, S, 32)
    else:
        assert t["blocks_bytes"] == 0 and t["thresholds"] is None and t["block_guide"] is None
        assert S <= 4 or C * S * (4 * row + 32) > 24576


def test_size_hook_is_exported_and_declared():
    assert "cmx_debug_sim_sites" in engine.EXPORTS
    assert hasattr(engine.load_library(), "cmx_debug_sim_sites")
    with open(os.path.join(ROOT, "include", "comap_mi355x.h")) as f:
        assert "void cmx_debug_sim_sites(long long min_sites, long long four_batch_sites);" in f.read()
