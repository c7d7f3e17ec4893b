"""-m gpu: the cherry message table of 20-state models (cmx_walk.h: kCherryMsg; cmx_layout.h).

On the null's resolved alignments map_kernel<20, null> and map_kernel<20, patterns> gather an inlined cherry's message from
a table that a setup kernel filled with the walk's own leaf gathers and product.  The table holds what the walk computes,
so with the table (engine.cherry_msg(True), the default) and without it a null over the same supplied alignments must
give THE SAME BYTES in stat, nmin, prmin and rcmin, on the pattern path and on the per-site path.  Beside that: the null
against the generic observed walk (eng.map_sites) at 1e-11 and against the oracle at 1e-6, as test_gpu_cherry_tables.py
does for nucleotides; the downloaded table against P_c (A o B) from numpy at 1e-13; a model over the byte limit has no
table and its null is the switch-off run.

Shapes: balanced 16 (every leaf in a cherry), caterpillar 9 (one cherry at the bottom), random_tree(40, 77), and the rooted
trees of 3 and 4 leaves whose cherries hang under the root (a walk with no stored vector).  1 and 4 rate classes, one and
two substitution types, 3 replicates x 53 sites (five blocks of the per-site path, the last one partial)."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from tree_shapes import _arrays, _balanced, _caterpillar, _parse

pytestmark = pytest.mark.gpu

OUT = ("stat", "nmin", "prmin", "rcmin")
PROTEIN = {1: synthetic.protein_model(0.5, 1), 4: synthetic.protein_model(0.5, 4)}


def _tree(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "random40":
        return synthetic.random_tree(40, 77)
    if name == "balanced16":
        parent, lot = _balanced(16)
    elif name == "balanced256":
        parent, lot = _balanced(256)
    elif name == "caterpillar9":
        parent, lot = _caterpillar(9)
    else:
        parent, lot = _arrays(_parse(name), seed=len(name))
    blen = np.maximum(rng.exponential(0.1, size=len(parent)), 1e-6)
    blen[-1] = 0.0
    return parent, blen, lot


def _engines(tree, C, K, grid=None):
    """(engine with the table, engine without) of the same model and tree"""
    parent, blen, lot = tree
    mdl = PROTEIN[C]
    kw = {}
    if K == 2:
        W1 = np.random.default_rng(4).uniform(-1, 1, size=mdl["Q"].shape)
        kw = dict(Bk=np.stack([synthetic.weighted_register(mdl["Q"], W1), synthetic.weighted_register(mdl["Q"], np.abs(W1))]),
                  clamp_negative=False)
    was, was_g = engine.cherry_msg(), engine.map_grid()
    try:
        if grid is not None:
            engine.map_grid(grid)
        out = []
        for on in (True, False):
            engine.cherry_msg(on)
            out.append(engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], **kw))
    finally:
        engine.cherry_msg(was)
        engine.map_grid(was_g)
    return out


def _same_bytes(eng_on, eng_off, kind, sup):
    """the null over `sup` on both paths of both engines; every output the same bytes, engine against engine within a path
    and the pattern path against the per-site path (what test_gpu_null_patterns._both compares); -> the pattern path's result"""
    nrep, _, _, ram = sup.shape
    first = None
    for patterns in (True, False):
        res = []
        for eng in (eng_on, eng_off):
            eng.set_null_patterns(patterns)
            res.append(eng.null_intra(kind, 0, 0, nrep, ram, supplied=sup))
            eng.set_null_patterns(None)
        for key in OUT:
            a, b = res[0][key], res[1][key]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (key, "patterns" if patterns else "per site", int((a != b).sum()))
        first = first or res[0]
        for key in OUT:
            a, b = first[key], res[0][key]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (key, "patterns against per site", int((a != b).sum()))
    return first


def _supplied(eng, nrep, ram, seed=5):
    return np.stack([np.stack([eng.simulate(seed, (r * 2 + h) * ram, ram)[0] for h in range(2)]) for r in range(nrep)])


SHAPES = ["balanced16", "caterpillar9", "random40", "((x,x),x)", "(x,(x,x))", "((x,x),(x,x))"]


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_null_is_the_same_bytes_with_and_without_the_table(shape, C, K):
    tree = _tree(shape)
    eng_on, eng_off = _engines(tree, C, K)
    on, off = eng_on.cherry_msg_info(), eng_off.cherry_msg_info()
    info = eng_on.info()
    assert info["cherry_tables"] == info["products_per_pass_null"] == info["leaf_ops_per_pass_null"] == 0
    assert on["tables"] >= 1 and on["table_bytes"] == C * on["tables"] * 400 * 192 and off["tables"] == off["gathers"] == 0
    if shape == "balanced16":
        assert on["tables"] >= 6                   # (the two cherries under the root's children may be visited)
    assert on["products"] == off["products"] - 2 * on["tables"] == info["products_per_pass"] - 2 * on["tables"]
    assert on["leaf_ops"] == off["leaf_ops"] - 4 * on["tables"] and on["gathers"] == 2 * on["tables"]
    nrep, ram = 3, 53
    sup = _supplied(eng_on, nrep, ram)
    kind = engine.STAT_CORRELATION if K == 1 else engine.STAT_COMPENSATION
    nl = _same_bytes(eng_on, eng_off, kind, sup)
    # ... and what the generic observed walk (leaf gathers and products) gives for the same columns
    okind = oracle.ST_CORRELATION if K == 1 else oracle.ST_COMPENSATION
    for r in range(nrep):
        m0, m1 = eng_on.map_sites(sup[r, 0]), eng_on.map_sites(sup[r, 1])
        sl = slice(r * ram, (r + 1) * ram)
        rel_close(nl["nmin"][sl], np.minimum(m0["norm"], m1["norm"]), 1e-11, 1e-300)
        rel_close(nl["prmin"][sl], np.minimum(m0["post_rate"], m1["post_rate"]), 1e-12)
        assert np.array_equal(nl["rcmin"][sl], np.minimum(m0["rate_class"], m1["rate_class"]))
        st = np.array([oracle.stat_pair(okind, m0["counts"][j], m1["counts"][j]) for j in range(ram)])
        rel_close(nl["stat"][sl], st, 1e-8, 1e-11)


def test_a_wave_that_maps_several_blocks():
    """the grid capped to 8 workgroups = 32 waves, about 40 blocks of pairs (80 of columns): the queue hands a wave several
    blocks, and the last op of a block requests the first operator of the next over the resolved stream"""
    eng_on, eng_off = _engines(_tree("random40"), 4, 1, grid=8)
    sup = _supplied(eng_on, 8, 317, seed=11)
    _same_bytes(eng_on, eng_off, engine.STAT_CORRELATION, sup)


def test_every_row_of_a_table_is_gathered():
    """one supplied replicate of 400 sites in which the leaves of one cherry run through all 400 symbol pairs"""
    tree = _tree("balanced16")
    eng_on, eng_off = _engines(tree, 4, 1)
    _, nodes = eng_on.cherry_msg_table()
    lot = np.asarray(tree[2])
    t1, t2 = int(np.flatnonzero(lot == nodes[0, 1])[0]), int(np.flatnonzero(lot == nodes[0, 2])[0])
    sup = _supplied(eng_on, 1, 400, seed=3)
    p = np.arange(400)
    for h in range(2):
        sup[0, h, t1], sup[0, h, t2] = (p // 20, p % 20) if h == 0 else (p % 20, p // 20)
    nl = _same_bytes(eng_on, eng_off, engine.STAT_CORRELATION, sup)
    m0, m1 = eng_on.map_sites(sup[0, 0]), eng_on.map_sites(sup[0, 1])
    rel_close(nl["nmin"], np.minimum(m0["norm"], m1["norm"]), 1e-11, 1e-300)
    assert np.array_equal(nl["rcmin"], np.minimum(m0["rate_class"], m1["rate_class"]))


@pytest.mark.parametrize("shape,C", [("balanced16", 4), ("random40", 4), ("((x,x),x)", 1)])
def test_the_table_holds_the_messages(shape, C):
    """M_c[x] = sum_z P_c[x, z] P_l1[z, s1] P_l2[z, s2] for every class, cherry and symbol pair: 20 products summed, a
    relative error of a few 1e-15 whatever the order (all terms are positive)"""
    tree = _tree(shape)
    eng, _ = _engines(tree, C, 1)
    table, nodes = eng.cherry_msg_table()
    P = eng.transition_matrices()                  # [C, B, S, S], branch = node
    assert table.shape == (C, eng.cherry_msg_info()["tables"], 400, 20)
    kids = {}
    for c, par in enumerate(tree[0]):
        kids.setdefault(int(par), []).append(c)
    for ci, (node, l1, l2) in enumerate(nodes):
        assert kids[int(node)] == [int(l1), int(l2)]
        for c in range(C):
            ab = (P[c, l1][:, :, None] * P[c, l2][:, None, :]).reshape(20, 400)      # [z, 20 s1 + s2]
            rel_close(table[c, ci], (P[c, node] @ ab).T, 1e-13)


def test_against_the_oracle_with_many_cherries():
    parent, lot = _balanced(32)
    blen = np.maximum(np.random.default_rng(3).exponential(0.15, size=len(parent)), 1e-6)
    mdl = PROTEIN[4]
    eng = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    assert eng.cherry_msg_info()["tables"] >= 14
    om = oracle.Model(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    g, o = eng.null_intra(1, 91, 2, 5, 70), oracle.null_intra(om, 1, 91, 2, 5, 70)
    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
    rel_close(g["nmin"], o["nmin"], 1e-6)
    assert np.array_equal(g["rcmin"], o["rcmin"])


def test_a_model_over_the_byte_limit_walks_as_before():
    eng_on, eng_off = _engines(_tree("balanced256"), 4, 1)
    on = eng_on.cherry_msg_info()
    assert on["tables"] == on["table_bytes"] == on["gathers"] == 0 and on == eng_off.cherry_msg_info()
    assert 4 * 126 * 400 * 192 > on["max_bytes"]
    with pytest.raises(engine.CmxError):
        eng_on.cherry_msg_table()
    _same_bytes(eng_on, eng_off, engine.STAT_CORRELATION, _supplied(eng_on, 3, 53))
