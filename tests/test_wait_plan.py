"""The wait plan of the 64-site protein walk (cmx_layout.h, cmx_host_tree.cpp: plan_waits), no GPU.

An op of the mapping walk waits for its operator with `s_waitcnt vmcnt(n)`, n = the counted memory instructions the walk
issues between the operator's request and the wait: 4 DMA rows of the next request (+ 1 with symbols) and 10 per workspace
vector that moves through HBM in between.  The host records that distance per stream entry and the device reads the
immediate from the entry; `cmx_debug_wait_plan` returns both, and every build of a model (this call included) fails
unless the plan passes the engine's model of the wave's in-order memory queue (cmx_host_verify.cpp: WaitModel).

Here, from the outside:

* every immediate is a member of the run-time count's set (cmx_map.hip: wait_vm<20, 20>: 0 .. 6, 10 .. 16, 20 .. 26, 30),
  at most its distance, and the largest such member;
* a product waits with nothing newly issued (distance = whole vectors), a leaf op behind its own request (4 or 5 more);
* the distances of a pass add up to what the pass issues: every HBM vector is counted at exactly one op (the next one),
  every leaf op counts its own request, and the symbols of op 0 are not counted at the last op (smallest instance: the
  next site block's symbols are not requested);
* with the LDS slot planned empty (cmx_debug_lds_slot(0)) every transfer that went back to HBM adds exactly 10 to one
  entry, and nothing else changes;
* a plan with one immediate raised by one is refused, before any context exists."""
import numpy as np
import pytest

from comap_amd import engine, synthetic
from comap_amd.engine import CmxError
from lds_slot_trees import bench64, hand_built
from tree_shapes import Shape, _arrays, _balanced, _caterpillar, _parse

WAIT_VM_SET = sorted(set(range(0, 7)) | set(range(10, 17)) | set(range(20, 27)) | {30})
PROTEIN = {1: synthetic.protein_model(0.5, 1), 4: synthetic.protein_model(0.5, 4)}


def _shapes():
    out = []
    for n in (3, 4, 5, 8):
        par, lot = _caterpillar(n)
        out.append(Shape(f"rooted{n}", par, lot))
        parent, _, lot = synthetic.random_tree(n, 40 + n)
        out.append(Shape(f"unrooted{n}", parent, lot, rooted=False))
    par, lot = _caterpillar(12)                       # no node with two visited children
    out.append(Shape("caterpillar12", par, lot))
    par, lot = _balanced(16)                          # two-visited nodes, LDS-slot transfers
    out.append(Shape("balanced16", par, lot))
    for name, s in (("multifurcation", "(x,x,(x,x),(x,(x,x)),x)"),     # pseudo nodes
                    ("cherry_as_a", "((x,x),(x,(x,x)))"), ("cherry_as_b", "((x,(x,x)),(x,x))")):
        par, lot = _arrays(_parse(s), seed=77)
        out.append(Shape(name, par, lot))
    out += [s for s in hand_built() if s.name in ("root6", "nested9", "disjoint9", "unrooted9")]
    return out


SHAPES = _shapes()
BENCH, BENCH_BLEN = bench64()


def _bk(Q):
    W1 = np.random.default_rng(4).uniform(-1, 1, size=Q.shape)
    return np.stack([synthetic.weighted_register(Q, W1), synthetic.weighted_register(Q, np.abs(W1))])


def _args(shape, K, C=4, blen=None):
    mdl = PROTEIN[C]
    blen = shape.blen_variants()[0][1] if blen is None else blen
    kw = {} if K == 1 else dict(Bk=_bk(mdl["Q"]))
    return (shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"]), kw


def _plan(shape, K, C=4, blen=None):
    a, kw = _args(shape, K, C, blen)
    walk, plan = engine.debug_walk(*a, **kw), engine.debug_wait_plan(*a, **kw)
    assert len(plan["distance"]) == len(plan["immediate"]) == len(walk["msched"])
    return walk, plan["distance"].astype(np.int64), plan["immediate"].astype(np.int64)


def _check(walk, dist, imm):
    leaf = walk["msched"][:, 1] >= 0
    for i, (d, w) in enumerate(zip(dist, imm)):
        assert w in WAIT_VM_SET and w <= d, (i, d, w)
        assert w == max(m for m in WAIT_VM_SET if m <= d), (i, d, w)
    assert (dist[~leaf] % 10 == 0).all()
    assert np.isin(dist[leaf] % 10, (4, 5)).all()
    # the pass's counted instructions, each at exactly one op
    hbm = walk["loads"] + walk["stores"] - walk["lds_loads"] - walk["lds_stores"]
    own = sum(4 + (1 if i + 1 < len(leaf) and leaf[i + 1] else 0) for i in np.flatnonzero(leaf))
    assert dist.sum() == 10 * hbm + own
    assert walk["products"] == int((~leaf).sum()) and walk["leaf_ops"] == int(leaf.sum())


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_plan_of_small_trees(shape, K):
    for C in (4, 1):
        _check(*_plan(shape, K, C))


@pytest.mark.parametrize("K", [1, 2])
def test_plan_of_the_benchmark_tree(K):
    walk, dist, imm = _plan(BENCH, K, blen=BENCH_BLEN)
    _check(walk, dist, imm)
    leaf = walk["msched"][:, 1] >= 0
    print(f"benchmark tree, K = {K}: {len(dist)} ops; product immediates {sorted(set(imm[~leaf]))}, leaf immediates {sorted(set(imm[leaf]))}")
    assert set(imm[~leaf]) <= {0, 10, 20, 30} and set(imm[leaf]) <= {4, 5, 14, 15, 24, 25, 30}


def test_a_caterpillar_moves_one_vector_per_visit():
    """no LDS-slot transfer and no two vectors between two ops of the inside pass: no distance beyond two vectors + a request"""
    _, dist, _ = _plan(SHAPES[[s.name for s in SHAPES].index("caterpillar12")], 1)
    assert dist.max() <= 25


@pytest.mark.parametrize("shape", [s for s in SHAPES if s.name in ("balanced16", "root6", "nested9", "disjoint9", "unrooted9")] + [BENCH],
                         ids=lambda s: s.name)
def test_without_the_lds_slot_every_returned_transfer_is_ten_instructions_at_one_op(shape):
    blen = BENCH_BLEN if shape is BENCH else None
    was = engine.lds_slot()
    try:
        engine.lds_slot(True)
        on, d_on, _ = _plan(shape, 1, blen=blen)
        engine.lds_slot(False)
        off, d_off, i_off = _plan(shape, 1, blen=blen)
    finally:
        engine.lds_slot(was)
    _check(off, d_off, i_off)
    moved = on["lds_loads"] + on["lds_stores"]
    assert moved > 0 and off["lds_loads"] == off["lds_stores"] == 0
    assert np.array_equal(on["msched"], off["msched"])
    diff = d_off - d_on
    assert (diff >= 0).all() and (diff % 10 == 0).all()
    assert diff.sum() == 10 * moved                   # exactly 10 per transfer that went back to HBM, nothing else
    assert np.count_nonzero(diff) <= moved


def _refused(shape, entry):
    a, kw = _args(shape, 1)
    assert engine.wait_skew(entry) == -1
    try:
        with pytest.raises(CmxError) as e:
            engine.debug_wait_plan(*a, **kw)
    finally:
        engine.wait_skew(None)
    return str(e.value)


def test_a_wait_that_is_too_lax_is_refused_before_a_context_exists():
    shape = SHAPES[[s.name for s in SHAPES].index("balanced16")]
    walk, dist, imm = _plan(shape, 1)
    leaf = walk["msched"][:, 1] >= 0
    # a leaf op at distance 4 = its own request of four rows: vmcnt(5) leaves the last row of ITS operator in flight
    k = int(np.flatnonzero(leaf & (dist == 4))[0])
    msg = _refused(shape, k)
    assert "wait plan refused" in msg and f"op {k} " in msg and "not landed" in msg, msg
    # a product at distance 0 (its operator is the last thing requested): vmcnt(1) is no wait the device has, and would
    # leave the operator's last row in flight
    k = int(np.flatnonzero(~leaf & (dist == 0))[0])
    assert "wait plan refused" in _refused(shape, k)
    # a leaf op at distance 5: vmcnt(6) is in the run-time count's set, not the choice for 5
    k = int(np.flatnonzero(leaf & (dist == 5))[0])
    assert "wait plan refused" in _refused(shape, k)
    # the hook is spent by the build it skews: the next one passes
    _check(*_plan(shape, 1))
    # ... and it sits in front of everything a context does: creating an engine fails on the plan, not on the device
    a, kw = _args(shape, 1)
    k = int(np.flatnonzero(leaf & (dist == 4))[0])
    engine.wait_skew(k)
    try:
        with pytest.raises(CmxError) as e:
            engine.Engine(*a, **kw)
    finally:
        engine.wait_skew(None)
    assert "wait plan refused" in str(e.value), str(e.value)


def test_a_model_without_a_plan_does_not_spend_the_skew():
    """only a build that makes a plan consumes the hook (include/comap_mi355x.h)"""
    mdl = synthetic.dna_model(0.7, 4)
    shape = SHAPES[0]
    engine.wait_skew(0)
    try:
        engine.debug_wait_plan(shape.parent, shape.blen_variants()[0][1], shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
        assert engine.wait_skew(None) == 0
    finally:
        engine.wait_skew(None)


def test_the_split16_switch_is_a_host_side_flag():
    was = engine.map_small_blocks()
    try:
        assert engine.map_small_blocks(False) == was
        assert engine.map_small_blocks() is False
        assert engine.map_small_blocks(True) is False
    finally:
        engine.map_small_blocks(was)
    assert was is True


def test_models_without_the_walk_have_no_plan():
    mdl = synthetic.dna_model(0.7, 4)
    shape = SHAPES[0]
    p = engine.debug_wait_plan(shape.parent, shape.blen_variants()[0][1], shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    assert len(p["distance"]) == 0 and len(p["immediate"]) == 0
