"""-m gpu: how the 64-site mapping launches hand their site blocks to the waves (cmx_map.hip next_block).

A wave maps the block of its own index and then draws blocks from a device counter; which wave maps a block changes no
byte of any output, so every result with the queue (the default) must be the same BYTES as with the fixed strided
assignment (engine.map_queue(False)) in the same process -- no block twice, none missed -- and agree with the oracle at
the tolerances of test_gpu_lds_slot.  Protein Gamma-4 on the hand-built trees root6 and nested9, the mapping grid capped
to 8 workgroups = 32 waves (engine.map_grid) so that a few thousand sites are many rounds of blocks.

Block counts: 31, 32, 33 (the strided path, the boundary nb == nwaves where no launch gets a counter, the first drawn
block) and 3 * 32 + 5 = 101 with a last block of 47 sites; each as observed mapping (101 blocks x 4 classes are more than
the 32 wave-tasks up to which the class-split launch takes an alignment: map_kernel<20, observed>), per-site null and
pattern null of supplied columns that are all distinct, patterns = sites (but one repeated column where the pattern count
must be odd).  The oracle maps each distinct column once (one pool per tree, shared by every case)."""
import numpy as np
import pytest
import torch

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from lds_slot_trees import hand_built
from test_gpu_parity import _check_map

pytestmark = pytest.mark.gpu

WG = 8
NW = 4 * WG                                   # waves of a capped launch
BLOCKS = [NW - 1, NW, NW + 1, 3 * NW + 5]
LAST = {3 * NW + 5: 47}                       # sites of the last block where it is partial
POOL = 64 * (3 * NW + 5)                      # distinct columns: the largest case's sites
KIND = engine.STAT_CORRELATION
SHAPES = {s.name: s for s in hand_built() if s.name in ("root6", "nested9")}
_CACHE = {}


def _nsites(nb):
    return 64 * (nb - 1) + LAST.get(nb, 64)


def _case(name):
    """-> (engine arguments, pool of distinct columns [T, POOL], the oracle's mapping of the pool); computed once per tree"""
    if name not in _CACHE:
        shape = SHAPES[name]
        mdl = synthetic.protein_model(0.5, 4)
        blen = np.random.default_rng(shape.nn).uniform(0.05, 0.4, size=shape.nn)
        blen[-1] = 0.0
        args = (shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
        om = oracle.Model(*args, nonneg=True)
        rng = np.random.default_rng(77 + shape.nn)
        codes = rng.choice(20 ** min(shape.ntaxa, 6), size=POOL, replace=False)      # distinct in the first six rows
        pool = np.zeros((shape.ntaxa, POOL), dtype=np.uint8)
        for t in range(shape.ntaxa):
            pool[t] = (codes // 20 ** t) % 20 if t < 6 else rng.integers(0, 20, size=POOL)
        pool = np.ascontiguousarray(pool)
        assert len(np.unique(pool, axis=1).T) == POOL
        _CACHE[name] = args, pool, oracle.map_sites(om, pool)
    return _CACHE[name]


def _engine(args):
    was = engine.map_grid(WG)
    try:
        return engine.Engine(*args)
    finally:
        engine.map_grid(was)


def _queued(on, fn, *a, **kw):
    was = engine.map_queue(on)
    try:
        return fn(*a, **kw)
    finally:
        engine.map_queue(was)


def _same_bytes(a, b, what):
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


def _null_want(o, i0, i1):
    """the null of the pairs (pool column i0[j], pool column i1[j]) from the oracle's mapping of the pool"""
    return dict(stat=np.array([oracle.stat_pair(oracle.ST_CORRELATION, o["counts"][a], o["counts"][b]) for a, b in zip(i0, i1)]),
                rcmin=np.minimum(o["rate_class"][i0], o["rate_class"][i1]), prmin=np.minimum(o["post_rate"][i0], o["post_rate"][i1]),
                nmin=np.minimum(o["norm"][i0], o["norm"][i1]))


def _check_null(got, want):
    rel_close(got["stat"], want["stat"], 1e-6, 1e-12)
    rel_close(got["nmin"], want["nmin"], 1e-6)
    rel_close(got["prmin"], want["prmin"], 1e-9)
    assert np.array_equal(got["rcmin"], want["rcmin"])


def _null_both(on, off, patterns, pool, i0, i1, what):
    sup = np.ascontiguousarray(np.stack([pool[:, i0], pool[:, i1]])[None])   # [1, 2, T, pairs]
    for e in (on, off):
        e.set_null_patterns(patterns)
    n_on = _queued(True, on.null_intra, KIND, 1, 0, 1, len(i0), supplied=sup)
    n_off = _queued(False, off.null_intra, KIND, 1, 0, 1, len(i0), supplied=sup)
    _same_bytes(n_on, n_off, what)
    return n_on


@pytest.mark.parametrize("nb", BLOCKS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_queue_equals_strided_and_the_oracle(name, nb):
    args, pool, o = _case(name)
    on, off = _engine(args), _engine(args)
    assert on.info()["waves"] == NW
    n = _nsites(nb)
    # ---- observed: nb blocks of the pool's first n columns
    g_on, g_off = _queued(True, on.map_sites, pool[:, :n]), _queued(False, off.map_sites, pool[:, :n])
    _same_bytes(g_on, g_off, "observed")
    _check_map(g_on, {k: v[:n] for k, v in o.items()})
    # ---- per-site null: n pairs = nb blocks; pair j = (column j, column POOL - 1 - j)
    i0, i1 = np.arange(n), POOL - 1 - np.arange(n)
    _check_null(_null_both(on, off, False, pool, i0, i1, "per-site null"), _null_want(o, i0, i1))
    # ---- pattern null: 2 * pairs sites, all distinct (n odd: the last site repeats the first column) = n patterns = nb blocks
    pairs = (n + 1) // 2
    i0, i1 = np.arange(pairs), pairs + np.arange(pairs)
    if n % 2:
        i1[-1] = 0
    got = _null_both(on, off, True, pool, i0, i1, "pattern null")
    assert on.null_pattern_count() == n
    _check_null(got, _null_want(o, i0, i1))
    for e in (on, off):
        e.synchronize()
        e.close()


def test_pattern_count_far_below_the_site_count():
    """6 distinct columns over 2 x 3 232 sites: the grid and the counter are sized for 101 blocks, the waves read one"""
    args, pool, o = _case("nested9")
    on, off = _engine(args), _engine(args)
    rng = np.random.default_rng(5)
    pairs = _nsites(3 * NW + 5) // 2
    i0, i1 = rng.integers(0, 6, size=pairs), rng.integers(0, 6, size=pairs)
    i0[:6] = np.arange(6)
    got = _null_both(on, off, True, pool, i0, i1, "pattern null of 6 columns")
    assert on.null_pattern_count() == 6
    _check_null(got, _null_want(o, i0, i1))
    for e in (on, off):
        e.close()


def _dev_runs(eng, pool, n_obs, sup, pairs, both):
    """observed mapping of n_obs sites and the per-site null of `sup`: on two streams at once (both) or one after the other"""
    dev = torch.device("cuda", 0)
    d_aln, d_sup = torch.from_numpy(pool[:, :n_obs].copy()).to(dev), torch.from_numpy(sup).to(dev)
    BK = eng.B * eng.K
    obs = dict(counts=torch.zeros((BK, n_obs), dtype=torch.float64, device=dev), logL=torch.zeros(n_obs, dtype=torch.float64, device=dev),
               post_rate=torch.zeros(n_obs, dtype=torch.float64, device=dev), rate_class=torch.zeros(n_obs, dtype=torch.int32, device=dev),
               norm=torch.zeros(n_obs, dtype=torch.float64, device=dev))
    nul = dict(stat=torch.zeros(pairs, dtype=torch.float64, device=dev), rcmin=torch.zeros(pairs, dtype=torch.int32, device=dev),
               prmin=torch.zeros(pairs, dtype=torch.float64, device=dev), nmin=torch.zeros(pairs, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    side, main = torch.cuda.Stream(device=dev), torch.cuda.current_stream()
    if both:
        side.wait_stream(main)
        with torch.cuda.stream(side):
            eng.map_sites_dev(d_aln, **obs)
        eng.null_intra_dev(KIND, 1, 0, 1, pairs, supplied=d_sup, **nul)
        main.wait_stream(side)
    else:
        eng.map_sites_dev(d_aln, **obs)
        torch.cuda.synchronize()
        eng.null_intra_dev(KIND, 1, 0, 1, pairs, supplied=d_sup, **nul)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in {**obs, **{"null_" + k: v for k, v in nul.items()}}.items()}


def test_two_queued_launches_in_flight():
    """observed mapping on a side stream beside a queued null on the main stream, twice on one context: each launch has a
    counter of its own, so both results are those of the solo runs"""
    args, pool, _ = _case("nested9")
    eng = _engine(args)
    eng.set_null_patterns(False)
    n = _nsites(3 * NW + 5)
    sup = np.ascontiguousarray(np.stack([pool[:, :n], pool[:, ::-1][:, :n]])[None])
    solo = _dev_runs(eng, pool, n, sup, n, both=False)
    for turn in range(2):
        _same_bytes(solo, _dev_runs(eng, pool, n, sup, n, both=True), f"turn {turn}")
    eng.close()


def test_ring_reuse():
    """600 queued launches back to back on one context: every one of the ring's 256 counters is taken at least twice"""
    args, pool, _ = _case("root6")
    eng = _engine(args)
    eng.set_null_patterns(False)
    dev = torch.device("cuda", 0)
    n = 64 * (NW + 1)
    d_sup = torch.from_numpy(np.ascontiguousarray(np.stack([pool[:, :n], pool[:, n:2 * n]])[None])).to(dev)
    first, last = (dict(stat=torch.zeros(n, dtype=torch.float64, device=dev), nmin=torch.zeros(n, dtype=torch.float64, device=dev))
                   for _ in range(2))
    for i in range(600):
        eng.null_intra_dev(KIND, 1, 0, 1, n, supplied=d_sup, **(first if i == 0 else last))
    torch.cuda.synchronize()
    _same_bytes({k: v.cpu().numpy() for k, v in first.items()}, {k: v.cpu().numpy() for k, v in last.items()}, "launch 600")
    assert float(first["stat"].abs().sum()) > 0.0
    eng.close()
