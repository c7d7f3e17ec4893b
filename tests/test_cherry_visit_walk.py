"""The outside visit of an inlined cherry gathers each of its two leaf rows once (cmx_walk.h, kCherryRows), no GPU.

`debug_walk` compiles a tree into what the mapping kernel reads and fails unless the numeric walk, consuming the recorded
operator stream exactly as the device does, reproduces likelihood and every joint count of a direct pruning computation.
Here the per-pass operator counts it returns are set against the walk's own book-keeping, recomputed from the returned
node records (K = number of substitution types):

* a leaf outside an inlined cherry costs 2 + K leaf ops: one in the inside pass, one where the outside pass takes its
  message, K dot products for its own branch;
* an inlined cherry costs 4 leaf ops and 2 products for its message (inside pass, and rebuilt in the outside pass) plus its
  outside visit: K + 1 products and, for unfused models, 2 + 3 K leaf ops as child A (one row stays in a register, the
  sibling's outside message occupies another) or 2 + 2 K as child B (both rows stay); class-fused nucleotide models keep
  the plain visit of 2 + 4 K (their null runs on the cherry tables);
* a visited tree node below the root costs K + 2 products (M inside; K counts and Up outside);
* workspace loads and stores follow from the records alone and do not depend on the visit."""
import numpy as np
import pytest

from comap_amd import engine, synthetic
from tree_shapes import Shape, catalogue

# record layout (cmx_walk.h)
REC_NODE, REC_FLAGS, REC_A, REC_B = 0, 3, 4, 9
CH_KIND = 0
KIND_LEAF, KIND_STORED, KIND_CHERRY = 0, 1, 2
FLAG_PSEUDO, FLAG_HAND, FLAG_U_HANDED, FLAG_ROOT = 1, 2, 4, 8

_bench = synthetic.random_tree(64, 20260101)
SHAPES = catalogue(2, 7) + [Shape("bench64", _bench[0], _bench[2], rooted=False)]
IDS = [s.name for s in SHAPES]


def _two_types(m):
    W1 = np.random.default_rng(4).uniform(-1, 1, size=(4, 4))
    return np.stack([synthetic.weighted_register(m["Q"], W1), synthetic.weighted_register(m["Q"], np.abs(W1))])


def _model(name):
    """-> (model dict, Bk or None, class-fused)"""
    if name == "protein_g4":
        return synthetic.protein_model(0.5, 4), None, False
    if name == "dna_3cls":
        return synthetic.dna_model(0.7, 3), None, False
    if name == "dna_3cls_2types":
        m = synthetic.dna_model(0.7, 3)
        return m, _two_types(m), False
    if name == "dna_g4":
        return synthetic.dna_model(0.7, 4), None, True
    if name == "dna_g4_2types":
        m = synthetic.dna_model(0.7, 4)
        return m, _two_types(m), True
    assert name == "dna_5cls"
    return synthetic.dna_model(0.7, 5), None, True


def _expected(nrec, K, rows):
    """per-pass counts from the node records: dict(leaf_ops, products, loads, stores, cherries_a, cherries_b)"""
    leaves = na = nb = real = loads = stores = 0
    for r in np.asarray(nrec).tolist():         # plain ints: numpy adds booleans as a logical or
        flags, ka, kb = r[REC_FLAGS], r[REC_A + CH_KIND], r[REC_B + CH_KIND]
        hand, root = bool(flags & FLAG_HAND), bool(flags & FLAG_ROOT)
        leaves += (ka == KIND_LEAF) + (kb == KIND_LEAF)
        na += ka == KIND_CHERRY
        nb += kb == KIND_CHERRY
        real += (not root) and not (flags & FLAG_PSEUDO)
        # inside pass: stored children are loaded unless handed over in a register; every node but the root stores M
        loads += (ka == KIND_STORED) + (kb == KIND_STORED and not hand)
        stores += not root
        # outside pass: U unless handed or at the root; both sibling messages; U of every stored child not handed on
        loads += (not root) and not (flags & FLAG_U_HANDED)
        loads += (ka == KIND_STORED) + (kb == KIND_STORED)
        stores += (ka == KIND_STORED) + (kb == KIND_STORED and not hand)
    visit_a, visit_b = (2 + 3 * K, 2 + 2 * K) if rows else (2 + 4 * K, 2 + 4 * K)
    return dict(leaf_ops=(2 + K) * leaves + na * (4 + visit_a) + nb * (4 + visit_b),
                products=(K + 2) * real + (K + 3) * (na + nb), loads=loads, stores=stores, cherries_a=na, cherries_b=nb)


def _walk(shape, blen, mdl, Bk):
    return engine.debug_walk(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk)


def _blen(shape):
    if shape.name == "bench64":
        return [("bench", _bench[1])]
    return shape.blen_variants()


@pytest.mark.parametrize("model", ["protein_g4", "dna_3cls", "dna_3cls_2types"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_unfused_models_gather_each_leaf_row_once(shape, model):
    mdl, Bk, fused = _model(model)
    K = 1 if Bk is None else len(Bk)
    for vname, blen in _blen(shape):
        d = _walk(shape, blen, mdl, Bk)             # fails unless the numeric walk reproduces direct pruning
        assert d["cherry_tables"] == 0 and d["products_tables"] == 0 and d["leaf_ops_tables"] == 0
        e = _expected(d["nrec"], K, rows=True)
        assert e["cherries_a"] + e["cherries_b"] == len(shape.cherries()), vname
        for key in ("leaf_ops", "products", "loads", "stores"):
            assert d[key] == e[key], (vname, key, d[key], e[key])
        ops = d["msched"]
        assert (ops[:, 1] >= 0).sum() == d["leaf_ops"] and (ops[:, 1] < 0).sum() == d["products"]
        assert d["loads"] == len(d["ldsched"])


@pytest.mark.parametrize("model", ["dna_g4", "dna_5cls", "dna_g4_2types"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_models_keep_the_plain_visit(shape, model):
    mdl, Bk, fused = _model(model)
    K = 1 if Bk is None else len(Bk)
    for vname, blen in _blen(shape):
        d = _walk(shape, blen, mdl, Bk)
        e = _expected(d["nrec"], K, rows=False)
        assert d["cherry_tables"] == e["cherries_a"] + e["cherries_b"] == len(shape.cherries()), vname
        for key in ("leaf_ops", "products", "loads", "stores"):
            assert d[key] == e[key], (vname, key, d[key], e[key])


def test_both_child_sides_occur():
    """the catalogue holds cherries as child A and as child B, beside a leaf, a stored and a handed sibling"""
    mdl, _, _ = _model("protein_g4")
    seen = set()
    for shape in SHAPES:
        d = _walk(shape, _blen(shape)[0][1], mdl, None)
        for r in d["nrec"]:
            for side, o, other in (("A", REC_A, REC_B), ("B", REC_B, REC_A)):
                if r[o + CH_KIND] == KIND_CHERRY:
                    sib = r[other + CH_KIND]
                    seen.add((side, "handed" if sib == KIND_STORED and side == "A" and r[REC_FLAGS] & FLAG_HAND else int(sib)))
    assert {("A", KIND_LEAF), ("B", KIND_LEAF), ("A", KIND_CHERRY), ("B", KIND_CHERRY), ("A", "handed")} <= seen, seen


def test_benchmark_tree_counts():
    """the 64-taxon benchmark tree: 18 inlined cherries; 201 products, 56 loads and 50 stores per pass as before, the leaf
    ops fall from 264 by one per cherry as child A and two per cherry as child B (K = 1)"""
    mdl, _, _ = _model("protein_g4")
    parent, blen, lot = _bench
    d = engine.debug_walk(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    e = _expected(d["nrec"], 1, rows=True)
    assert e["cherries_a"] + e["cherries_b"] == 18
    assert (d["products"], d["loads"], d["stores"]) == (201, 56, 50)
    assert d["leaf_ops"] == 264 - e["cherries_a"] - 2 * e["cherries_b"]
    assert 239 <= d["leaf_ops"] <= 246
