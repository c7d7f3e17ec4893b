"""The resolved protein walk with the cherry message table (cmx_walk.h: kCherryMsg; cmx_layout.h), no GPU.

On fully resolved alignments the message of an inlined cherry is a row of a device-built table, so the walk of the null's
kernels gathers it (no stream entry) where the plain walk spends two leaf ops and a product -- once in the inside pass and
once more where the outside pass rebuilds it.  `debug_cherry_msg_walk` compiles a tree into that walk's operator stream
and wait plan and fails unless the numeric walk that consumes the stream (its gather computed from the host matrices)
reproduces a direct pruning computation, moves the plain walk's workspace vectors through the plain walk's LDS-slot plan,
and the plan passes the engine's model of the wave's memory queue with the gathers as uncounted loads.  From the outside:

* per inlined cherry the products drop by 2 and the leaf ops by 4 per pass, with 2 gathers; loads, stores and LDS-slot
  transfers are the plain walk's; the stream is the plain one less those ops, in order;
* the benchmark tree: 165 products and 170 leaf ops against 201 and 242;
* the plan obeys the rules of the plain plan (tests/test_wait_plan.py), and one immediate raised by one is refused;
* no table: with the switch off, for a model whose tables exceed the byte limit, without an inlined cherry, and for
  other alphabets -- `cherry_tables`, `products_tables`, `leaf_ops_tables` of debug_walk stay 0 for unfused models."""
import numpy as np
import pytest

from comap_amd import engine, synthetic
from comap_amd.engine import CmxError
from tree_shapes import Shape, _balanced, catalogue

REC_A, REC_B, CH_KIND, KIND_CHERRY = 4, 9, 0, 2
ROW_BYTES, PAIRS = 192, 400
WAIT_VM_SET = sorted(set(range(0, 7)) | set(range(10, 17)) | set(range(20, 27)) | {30})

PROTEIN = synthetic.protein_model(0.5, 4)
_bench = synthetic.random_tree(64, 20260101)
BENCH = Shape("bench64", _bench[0], _bench[2], rooted=False)
SHAPES = catalogue(2, 7)
IDS = [s.name for s in SHAPES]


def _bk(Q):
    W1 = np.random.default_rng(4).uniform(-1, 1, size=Q.shape)
    return np.stack([synthetic.weighted_register(Q, W1), synthetic.weighted_register(Q, np.abs(W1))])


BK2 = _bk(PROTEIN["Q"])


def _args(shape, blen, mdl=PROTEIN):
    return (shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])


def _both(shape, blen, K, mdl=PROTEIN):
    kw = {} if K == 1 else dict(Bk=BK2)
    return engine.debug_walk(*_args(shape, blen, mdl), **kw), engine.debug_cherry_msg_walk(*_args(shape, blen, mdl), **kw)


def _inlined(walk):
    return int((walk["nrec"][:, REC_A + CH_KIND] == KIND_CHERRY).sum() + (walk["nrec"][:, REC_B + CH_KIND] == KIND_CHERRY).sum())


def _is_subsequence(sub, seq):
    it = iter(map(tuple, seq))
    return all(any(x == y for y in it) for x in map(tuple, sub))


def _check_plan(r, plain):
    """the rules of tests/test_wait_plan.py on the resolved walk's plan"""
    dist, imm = r["distance"].astype(np.int64), r["immediate"].astype(np.int64)
    leaf = r["msched"][:, 1] >= 0
    assert len(dist) == len(imm) == len(leaf) == r["products"] + r["leaf_ops"]
    for i, (d, w) in enumerate(zip(dist, imm)):
        assert w == max(m for m in WAIT_VM_SET if m <= d), (i, d, w)
    assert (dist[~leaf] % 10 == 0).all() and np.isin(dist[leaf] % 10, (4, 5)).all()
    # every HBM vector counted at one op, every leaf op its own request; a gather adds nothing
    hbm = plain["loads"] + plain["stores"] - plain["lds_loads"] - plain["lds_stores"]
    own = sum(4 + (1 if i + 1 < len(leaf) and leaf[i + 1] else 0) for i in np.flatnonzero(leaf))
    assert dist.sum() == 10 * hbm + own


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_products_and_four_leaf_ops_less_per_inlined_cherry(shape):
    for vname, blen in shape.blen_variants():
        plain, r = _both(shape, blen, 2)              # fails unless both numeric walks reproduce direct pruning
        n = _inlined(plain)
        assert plain["cherry_tables"] == plain["products_tables"] == plain["leaf_ops_tables"] == 0
        assert r["tables"] == n and r["table_bytes"] == 4 * n * PAIRS * ROW_BYTES, vname
        assert r["products"] == plain["products"] - 2 * n and r["leaf_ops"] == plain["leaf_ops"] - 4 * n, vname
        assert r["gathers"] == 2 * n
        for key in ("loads", "stores", "lds_loads", "lds_stores", "lds_copies"):
            assert r[key] == plain[key], (vname, key)
        if n == 0:
            assert len(r["msched"]) == 0
            continue
        assert len(r["msched"]) == len(plain["msched"]) - 6 * n
        assert _is_subsequence(r["msched"], plain["msched"]), vname
        _check_plan(r, plain)


def _refused(shape, blen, entry):
    assert engine.wait_skew(engine.WAIT_SKEW_RESOLVED + entry) == -1
    try:
        with pytest.raises(CmxError) as e:
            engine.debug_cherry_msg_walk(*_args(shape, blen), Bk=BK2)
    finally:
        engine.wait_skew(None)
    return str(e.value)


WITH_CHERRIES = [s for s in SHAPES if s.cherries()]       # (the others have no resolved plan)


@pytest.mark.parametrize("shape", WITH_CHERRIES, ids=[s.name for s in WITH_CHERRIES])
def test_a_wait_of_the_resolved_plan_that_is_too_lax_is_refused(shape):
    blen = shape.blen_variants()[0][1]
    plain, r = _both(shape, blen, 2)
    assert r["tables"] == len(shape.cherries()) > 0
    leaf, dist = r["msched"][:, 1] >= 0, r["distance"]
    picks = {0, len(dist) - 1, len(dist) // 2}
    picks |= {int(np.flatnonzero(leaf & (dist == 4))[0])} if (leaf & (dist == 4)).any() else set()
    picks |= {int(np.flatnonzero(~leaf & (dist == 0))[0])} if (~leaf & (dist == 0)).any() else set()
    for k in sorted(picks):
        msg = _refused(shape, blen, k)
        assert "wait plan refused" in msg and "resolved walk" in msg, (k, msg)
    # the hook is spent by the build it skews, and it names one plan: the plain plan's entry is the plain walk's to refuse
    _check_plan(engine.debug_cherry_msg_walk(*_args(shape, blen), Bk=BK2), plain)
    engine.wait_skew(0)
    try:
        with pytest.raises(CmxError) as e:
            engine.debug_cherry_msg_walk(*_args(shape, blen), Bk=BK2)
    finally:
        engine.wait_skew(None)
    assert "wait plan refused" in str(e.value) and "resolved walk" not in str(e.value)


def test_a_lax_leaf_wait_behind_a_gather_has_not_landed():
    """a leaf op at distance 4 waits for its own request of four rows: vmcnt(5) leaves its last row in flight, also with a
    gather's fourteen uncounted loads somewhere in the queue"""
    shape = next(s for s in SHAPES if s.name == "((x,x),(x,(x,x)))")
    blen = shape.blen_variants()[0][1]
    _, r = _both(shape, blen, 2)
    leaf, dist = r["msched"][:, 1] >= 0, r["distance"]
    k = int(np.flatnonzero(leaf & (dist == 4))[0])
    msg = _refused(shape, blen, k)
    assert f"op {k} " in msg and "not landed" in msg, msg


@pytest.mark.parametrize("K", [1, 2])
def test_benchmark_tree_counts(K):
    plain, r = _both(BENCH, _bench[1], K)
    assert _inlined(plain) == r["tables"] == 18 and r["gathers"] == 36
    assert r["table_bytes"] == 4 * 18 * PAIRS * ROW_BYTES == 5_529_600 <= r["max_bytes"]
    if K == 1:
        assert (plain["products"], plain["leaf_ops"]) == (201, 242)
        assert (r["products"], r["leaf_ops"]) == (165, 170)
    assert (r["products"], r["leaf_ops"]) == (plain["products"] - 36, plain["leaf_ops"] - 72)
    for key in ("loads", "stores", "lds_loads", "lds_stores", "lds_copies"):
        assert r[key] == plain[key], key
    assert (r["loads"], r["stores"]) == (56, 50)
    _check_plan(r, plain)
    leaf = r["msched"][:, 1] >= 0
    assert set(r["immediate"][~leaf]) <= {0, 10, 20, 30} and set(r["immediate"][leaf]) <= {4, 5, 14, 15, 24, 25, 30}


def test_the_switch_and_the_plain_plan_do_not_know_each_other():
    blen = _bench[1]
    was = engine.cherry_msg()
    try:
        assert engine.cherry_msg(False) == was
        plain_off, off = _both(BENCH, blen, 1)
        assert engine.cherry_msg(True) is False
        plain_on, on = _both(BENCH, blen, 1)
    finally:
        engine.cherry_msg(was)
    assert was is True                                        # the default is on
    assert off["tables"] == off["table_bytes"] == off["gathers"] == 0 and len(off["msched"]) == 0
    assert (off["products"], off["leaf_ops"]) == (plain_off["products"], plain_off["leaf_ops"])
    assert on["tables"] == 18
    for key in ("nrec", "ldsched", "msched"):                # records, load schedule and plain stream: untouched by the table
        assert np.array_equal(plain_on[key], plain_off[key]), key
    a = engine.debug_wait_plan(*_args(BENCH, blen))
    assert len(a["distance"]) == len(plain_on["msched"])


def test_a_model_over_the_byte_limit_has_no_table():
    par, lot = _balanced(256)                                # 126 inlined cherries x 4 classes x 76 800 bytes > 32 MiB
    shape = Shape("balanced256", par, lot)
    blen = np.full(shape.nn, 0.05)
    blen[-1] = 0.0
    plain, r = _both(shape, blen, 1)
    n = _inlined(plain)
    assert 4 * n * PAIRS * ROW_BYTES > r["max_bytes"] == 32 << 20
    assert r["tables"] == r["gathers"] == 0 and (r["products"], r["leaf_ops"]) == (plain["products"], plain["leaf_ops"])
    one = synthetic.protein_model(0.5, 1)                    # one class: a quarter of the bytes, under the limit
    _, r1 = _both(shape, blen, 1, one)
    assert r1["tables"] == n and r1["table_bytes"] == n * PAIRS * ROW_BYTES <= r1["max_bytes"]


@pytest.mark.parametrize("mdl", [synthetic.dna_model(0.7, 3), synthetic.dna_model(0.7, 4)], ids=["dna_3cls", "dna_g4"])
def test_other_alphabets_have_no_message_table(mdl):
    shape = next(s for s in SHAPES if s.name == "((x,x),(x,(x,x)))")
    r = engine.debug_cherry_msg_walk(*_args(shape, shape.blen_variants()[0][1], mdl))
    assert r["tables"] == r["gathers"] == 0 and len(r["msched"]) == 0
