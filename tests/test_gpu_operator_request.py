"""-m gpu: the operator request of the 64-site protein walk, issued from inside a product (cmx_map.hip: op_wait,
DevWalk::ProductRequest).

A product of that walk waits for its own operator, starts its matrix instructions and requests the NEXT op's operator,
symbols and stream entry from the gaps between them.  What can go wrong is an op reading a stage buffer before its operator
has landed, or after the next request has overwritten it, so the cases put a product at every kind of neighbour:

* in front of a leaf op whose symbols travel with the request (an outside visit's last product, then the leaf counts);
* in front of another product (W = J^T U, then Up = P^T U; K = 2: three products in a row);
* as the last op of a class pass (the request takes entry 0 of the next class from mat_after: four Gamma classes) and of
  the last class of a block (no symbols: the next block's prologue fetches them; one class: every pass is such a pass);
* right behind a visit's workspace loads (nested9, unrooted9: stored siblings) and right behind an LDS-slot load (root6,
  nested9, unrooted9: a two-visited node) -- and with neither (cherry3 = (x,(x,x)): one cherry and a leaf).

Which kernel a call runs (cmx_api_map.cpp: map_walk).  One rate class: every observed call, at 1, 64, 65 and 600 columns,
is map_kernel<20, observed> at 64 sites per wave.  Four classes: 600 columns on the engine capped to 8 workgroups = 32 waves
are map_kernel<20, observed> too (10 blocks x 4 classes > 32 wave-tasks, a wave maps several blocks in a row); 1, 64 and 65
columns are taken by the 16-site class-split launch, whose text this change leaves alone, at any cap -- they run all the
same and must agree with it.  Both nulls (3 replicates x 70 sites: map_kernel<20, null> and <20, patterns>) run the
64-site walk for every model.

Checks: the oracle at the tolerances of test_gpu_tiny_trees (_check_map; the nulls as test_gpu_mfma16_products); BYTES in
counts, logL, norm and rate class between every size and the 600-column call (a column's result does not depend on its
block or its neighbours) and, for four classes, against the 16-site class-split walk on an uncapped engine (post_rate goes
to the oracle only: the class-split launch rounds it differently, test_gpu_mfma16_products says why; with one class there
is no class-split walk to compare with); BYTES in every output between three repetitions of each call on one context.

A missed wait is a race, and equal repetitions are a cheap witness that there is none, not a proof.  The proof is the
counting argument in the comment above DevWalk::ProductRequest: LDS reads return in order, so the first matrix instruction
of a product -- which has waited for its operand -- stands behind every LDS read of the buffer the request overwrites, and
VMEM completes in order, so vmcnt(vs - cur_seq) covers this op's operator whatever was issued behind it."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from lds_slot_trees import V, hand_built
from test_gpu_parity import _check_map
from tree_shapes import Shape, _arrays, _parse

pytestmark = pytest.mark.gpu

WG = 8                      # workgroups of the capped engine: 32 waves
SIZES, PERIOD = (1, 64, 65, 600), 192
NREP, RAM = 3, 70
REPEATS = 3
BYTE_KEYS = ("counts", "logL", "norm", "rate_class")   # post_rate: see the module's docstring
ALL_KEYS = BYTE_KEYS + ("post_rate",)


def _shapes():
    out = {s.name: s for s in hand_built() if s.name in ("root6", "nested9", "unrooted9")}
    par, lot = _arrays(_parse(V), seed=77)
    out["cherry3"] = Shape("cherry3", par, lot)
    return out


SHAPES = _shapes()


def _setup(shape, K, ncat):
    """-> (oracle model, engine arguments, kind of the null statistic)"""
    mdl = synthetic.protein_model(0.5, ncat)
    blen = np.random.default_rng(shape.nn).uniform(0.05, 0.4, size=shape.nn)
    blen[-1] = 0.0
    Bk = None
    if K == 2:
        W1 = np.random.default_rng(4).uniform(-1, 1, size=mdl["Q"].shape)
        Bk = np.stack([synthetic.weighted_register(mdl["Q"], W1), synthetic.weighted_register(mdl["Q"], np.abs(W1))])
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
    """192 distinct columns: 150 simulated, 42 uniform random (states 16 .. 19 at the leaves), one ambiguous symbol
    (B = D or N) and one gap among them"""
    sim, _ = oracle.simulate(om, seed, 0, 150)
    rnd = np.random.default_rng(seed).integers(0, 20, size=(shape.ntaxa, PERIOD - 150)).astype(np.uint8)
    cols = np.ascontiguousarray(np.concatenate([sim, rnd], axis=1))
    cols[seed % shape.ntaxa, 3] = 20
    cols[(seed + 2) % shape.ntaxa, 160] = 21
    return cols


def _same_bytes(a, b, keys, what):
    for key in keys:
        assert np.ascontiguousarray(a[key]).tobytes() == np.ascontiguousarray(b[key]).tobytes(), (what, key)


def _repeat(call, keys, what):
    """three repetitions of one call on one context, the same bytes; -> the first result"""
    first = call()
    for i in range(1, REPEATS):
        _same_bytes(call(), first, keys, (what, "repetition", i))
    return first


@pytest.mark.parametrize("ncat", [1, 4])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_products_request_the_next_operator_from_their_gaps(name, K, ncat):
    shape = SHAPES[name]
    om, eargs, kind = _setup(shape, K, ncat)
    eng = _engine(eargs, WG)
    assert eng.info()["waves"] == 4 * WG
    masks = oracle.default_masks(20)
    masks[20] = (1 << 3) | (1 << 2)
    cols = _columns(om, shape, 11 + K + ncat)
    want = oracle.map_sites(om, cols, masks)
    # ---- observed mode, every size; the columns repeat with period 192
    got = {}
    for n in SIZES:
        rep = np.arange(n) % PERIOD
        aln = np.ascontiguousarray(cols[:, rep])
        got[n] = g = _repeat(lambda: eng.map_sites(aln, masks=masks[:22]), ALL_KEYS, ("observed", n))
        _check_map(g, {k: v[rep] for k, v in want.items()})
    big = got[SIZES[-1]]
    for n in SIZES[:-1]:
        _same_bytes(got[n], {k: np.asarray(big[k])[:n] for k in BYTE_KEYS}, BYTE_KEYS, ("size", n))
    if ncat > 1:   # the 16-site class-split walk on an uncapped engine: four 4x4x4_4b tile rows per product, request-then-wait
        short = _engine(eargs, 0)
        g16 = short.map_sites(cols, masks=masks[:22])
        _check_map(g16, want)
        rep = np.arange(SIZES[-1]) % PERIOD
        _same_bytes(big, {k: np.asarray(g16[k])[rep] for k in BYTE_KEYS}, BYTE_KEYS, "16-site walk")
        short.synchronize()
        short.close()
    # ---- nulls: per site (map_kernel<20, null>), then per distinct pattern (map_kernel<20, patterns>)
    seed = 5 + K + ncat
    wantn = oracle.null_intra(om, kind, seed, 0, NREP, RAM)
    gotn = {}
    for patterns in (False, True):
        eng.set_null_patterns(patterns)
        gotn[patterns] = n = _repeat(lambda: eng.null_intra(kind, seed, 0, NREP, RAM), ("stat", "nmin", "prmin", "rcmin"),
                                     ("null", patterns))
        rel_close(n["stat"], wantn["stat"], 1e-6, 1e-12)
        rel_close(n["nmin"], wantn["nmin"], 1e-6)
        rel_close(n["prmin"], wantn["prmin"], 1e-9)
        assert np.array_equal(n["rcmin"], wantn["rcmin"])
    _same_bytes(gotn[False], gotn[True], ("stat", "nmin"), "per-site null against pattern null")
    eng.synchronize()
    eng.close()
