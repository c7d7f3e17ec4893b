"""-m gpu: the 20-state products of the 64-site mapping walk on v_mfma_f64_16x16x4_f64 (cmx_map.hip: mfma16_steps;
DESIGN 4.1) against the oracle and against the 16-site walk, which stays on v_mfma_f64_4x4x4_4b for every state.

Trees: root6, nested9 and unrooted9 of lds_slot_trees.py (a cherry as child A and as child B, a two-visited node, a split
root); protein Gamma-4, K = 1 and K = 2.  Columns: 192 distinct ones, 150 simulated and 42 uniform random so that states
16 .. 19 -- the fifth tile, which the 64-site walk still runs on 4x4x4_4b -- occur at the leaves, with one ambiguous symbol
and one gap among them.

* the 192 columns as a short alignment: at this size the 16-site class-split launch (map_kernel<20, split, 1, NG = 1>).
* the same columns tiled with period 192 to 600 sites on an engine whose mapping grid is capped to 8 workgroups = 32
  waves: 10 blocks x 4 classes are more than the 32 wave-tasks up to which the class-split launch takes an alignment, so
  this is map_kernel<20, observed>; the last block has 24 sites.
* both against the oracle (_check_map at the tolerances of test_gpu_tiny_trees: the transposed products feed the counts,
  the forward ones logL, posterior rate and norm), and against each other as BYTES in counts, logL, norm and rate class.
  Found on the parent commit, where both shapes run every product as 25 tile steps of 4x4x4_4b, with this file: those
  four are the same bytes in all six cases; post_rate is not (last bit, every case) -- the class-split launch rounds
  rate x weight x L per class and sums in map_finalize_kernel, the one-kernel walk accumulates with fused multiply-adds
  -- so post_rate is left to the oracle check.  The comparison is the in-build witness that a chain of five 16x16x4
  rounds like the chain of five 4x4x4_4b it replaces (scripts/probe_mfma_f64_16x16x4.hip shows the same on random
  operands).
* the per-site null and the pattern null, 3 replicates x 70 sites (the last block of each is partial): stat and nmin the
  same bytes in both (the property test_gpu_null_patterns states), both against oracle.null_intra."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from lds_slot_trees import hand_built
from test_gpu_parity import _check_map

pytestmark = pytest.mark.gpu

WG = 8                      # workgroups of the capped engine: 32 waves
NSITES, PERIOD = 600, 192
NREP, RAM = 3, 70
BYTE_KEYS = ("counts", "logL", "norm", "rate_class")   # post_rate: see the module's docstring
SHAPES = {s.name: s for s in hand_built() if s.name in ("root6", "nested9", "unrooted9")}


def _bk(Q):
    W1 = np.random.default_rng(4).uniform(-1, 1, size=Q.shape)
    return np.stack([synthetic.weighted_register(Q, W1), synthetic.weighted_register(Q, np.abs(W1))])


def _setup(shape, K):
    """-> (oracle model, engine arguments, kind of the null statistic)"""
    mdl = synthetic.protein_model(0.5, 4)
    blen = np.random.default_rng(shape.nn).uniform(0.05, 0.4, size=shape.nn)
    blen[-1] = 0.0
    Bk = None if K == 1 else _bk(mdl["Q"])
    kw = {} if Bk is None else dict(Bk=Bk)
    args = (shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    om = oracle.Model(*args, nonneg=Bk is None, **kw)
    return om, (args, dict(clamp_negative=Bk is None, **kw)), (engine.STAT_CORRELATION if K == 1 else engine.STAT_COMPENSATION)


def _engine(eargs, workgroups):
    was = engine.map_grid(workgroups)
    try:
        return engine.Engine(*eargs[0], **eargs[1])
    finally:
        engine.map_grid(was)


def _columns(om, shape, seed):
    """192 distinct columns: 150 simulated, 42 uniform random, one ambiguous symbol (B = D or N) and one gap among them"""
    sim, _ = oracle.simulate(om, seed, 0, 150)
    rnd = np.random.default_rng(seed).integers(0, 20, size=(shape.ntaxa, PERIOD - 150)).astype(np.uint8)
    assert (rnd >= 16).any()
    cols = np.ascontiguousarray(np.concatenate([sim, rnd], axis=1))
    cols[seed % shape.ntaxa, 3] = 20
    cols[(seed + 2) % shape.ntaxa, 160] = 21
    return cols


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma16_products_against_the_oracle_and_the_16_site_walk(name, K):
    shape = SHAPES[name]
    om, eargs, kind = _setup(shape, K)
    short, long_ = _engine(eargs, 0), _engine(eargs, WG)
    assert long_.info()["waves"] == 4 * WG
    masks = oracle.default_masks(20)
    masks[20] = (1 << 3) | (1 << 2)
    cols = _columns(om, shape, 11 + K)
    rep = np.arange(NSITES) % PERIOD
    # ---- observed: the 16-site walk (4x4x4_4b) and map_kernel<20, observed> (16x16x4 + 4x4x4_4b)
    g16 = short.map_sites(cols, masks=masks[:22])
    g64 = long_.map_sites(np.ascontiguousarray(cols[:, rep]), masks=masks[:22])
    o = oracle.map_sites(om, cols, masks)
    _check_map(g16, o)
    _check_map(g64, {k: v[rep] for k, v in o.items()})
    for key in BYTE_KEYS:
        assert np.asarray(g64[key]).tobytes() == np.ascontiguousarray(np.asarray(g16[key])[rep]).tobytes(), key
    # ---- nulls: per site (map_kernel<20, null>), then per distinct pattern (map_kernel<20, patterns>)
    seed = 5 + K
    want = oracle.null_intra(om, kind, seed, 0, NREP, RAM)
    got = {}
    for patterns in (False, True):
        long_.set_null_patterns(patterns)
        got[patterns] = n = long_.null_intra(kind, seed, 0, NREP, RAM)
        rel_close(n["stat"], want["stat"], 1e-6, 1e-12)
        rel_close(n["nmin"], want["nmin"], 1e-6)
        rel_close(n["prmin"], want["prmin"], 1e-9)
        assert np.array_equal(n["rcmin"], want["rcmin"])
    for key in ("stat", "nmin"):
        assert got[False][key].tobytes() == got[True][key].tobytes(), key
    for e in (short, long_):
        e.synchronize()
        e.close()
