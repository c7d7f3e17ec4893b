"""The plan of the mapping walk's LDS slot (cmx_walk.h kLdsSlot, cmx_host_tree.cpp plan_lds_slot), no GPU.

A wave keeps ONE workspace vector on chip.  At a node whose child A is a visited node two vectors are short-lived:

* inside pass: M_a, stored at A's visit (end) and loaded at the node's (start) -- the slot saves the load, weight 1;
* outside pass: U_a, stored at the node's visit (end) and loaded at A's (start) -- the slot saves both, weight 2.

`debug_walk` returns the plan as FLAG_LDS_* bits of the node records and fails unless the numeric walk, which models the
slot as a fifth vector that is NaN until written and again after each read, reproduces direct pruning.  Here the plan is
replayed from the records alone at visit granularity (a visit loads at its start and stores at its end) and its count --
HBM transfers removed per class pass = lds_loads + lds_stores -- is set against a brute-force optimum over all subsets of
the candidates.  The benchmark tree's count is printed (run with -s) and pinned."""
import itertools

import numpy as np
import pytest

from comap_amd import engine, synthetic
from lds_slot_trees import bench64, hand_built
from tree_shapes import Shape, _caterpillar, catalogue

REC_SLOT, REC_FLAGS, REC_A, REC_B = 1, 3, 4, 9
CH_KIND, CH_SLOT = 0, 2
KIND_STORED = 1
M_PUT, M_GET, UA_PUT, U_GET = 16, 32, 64, 128
LDS_BITS = M_PUT | M_GET | UA_PUT | U_GET

HAND = hand_built()
RANDOM = []
for _n in range(8, 13):
    for _seed in (1, 2, 3):
        _p, _, _l = synthetic.random_tree(_n, 100 * _n + _seed)
        RANDOM.append(Shape(f"random{_n}_{_seed}", _p, _l, rooted=False))
SMALL = catalogue(2, 7) + HAND + RANDOM            # all of at most 12 leaves
PROTEIN = synthetic.protein_model(0.5, 4)


def _walk(shape, mdl=PROTEIN, blen=None):
    blen = shape.blen_variants()[0][1] if blen is None else blen
    return engine.debug_walk(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])


def _candidates(nrec):
    """[(start, end, weight)] at visit granularity: visit v of the inside pass loads at 2 v and stores at 2 v + 1, the
    outside pass follows in reverse visit order with the same two half-steps"""
    nrec = np.asarray(nrec).tolist()
    NV = len(nrec)
    visit_of = {r[REC_SLOT]: v for v, r in enumerate(nrec)}
    out = []
    for vp, r in enumerate(nrec):
        if r[REC_A + CH_KIND] != KIND_STORED:
            continue
        va = visit_of[r[REC_A + CH_SLOT]]
        assert va < vp
        out.append((2 * va + 1, 2 * vp, 1))
        base = 2 * NV
        out.append((base + 2 * (NV - 1 - vp) + 1, base + 2 * (NV - 1 - va), 2))
    return out


def _brute_force(cands):
    best = 0
    for k in range(len(cands) + 1):
        for pick in itertools.combinations(sorted(cands), k):
            if all(a[1] < b[0] for a, b in zip(pick, pick[1:])):
                best = max(best, sum(c[2] for c in pick))
    return best


def _replay(nrec):
    """follows the flags through both passes; returns (LDS loads, LDS stores, copies).  Every flagged load must find the
    vector it names in the slot -- so its store came earlier and no other flagged store in between -- and every flagged
    store must find the slot free"""
    nrec = np.asarray(nrec).tolist()
    slot, loads, stores, copies = None, 0, 0, 0
    for r in nrec:                                                    # inside pass
        f = r[REC_FLAGS]
        if f & M_GET:
            assert r[REC_A + CH_KIND] == KIND_STORED and slot == ("M", r[REC_A + CH_SLOT]), (slot, r)
            slot, loads = None, loads + 1
        if f & M_PUT:
            assert slot is None, (slot, r)
            slot, copies = ("M", r[REC_SLOT]), copies + 1
    assert slot is None, "a message put into the slot is never read"
    for r in reversed(nrec):                                          # outside pass
        f = r[REC_FLAGS]
        if f & U_GET:
            assert slot == ("U", r[REC_SLOT]), (slot, r)
            slot, loads = None, loads + 1
        if f & UA_PUT:
            assert r[REC_A + CH_KIND] == KIND_STORED and slot is None, (slot, r)
            slot, stores = ("U", r[REC_A + CH_SLOT]), stores + 1
    assert slot is None, "an outside message put into the slot is never read"
    return loads, stores, copies


@pytest.mark.parametrize("shape", SMALL, ids=[s.name for s in SMALL])
def test_plan_is_consistent_and_optimal(shape):
    d = _walk(shape)
    loads, stores, copies = _replay(d["nrec"])
    assert (d["lds_loads"], d["lds_stores"], d["lds_copies"]) == (loads, stores, copies)
    cands = _candidates(d["nrec"])
    assert len(cands) <= 16
    assert d["lds_loads"] + d["lds_stores"] == _brute_force(cands), (shape.name, cands)
    assert d["loads"] == len(d["ldsched"])                            # the walk's transfers, whichever memory serves them


def test_hand_built_counts():
    """root6: the inside load and the U pair of the root; nested9: the inner node's interval lies inside the outer one's,
    only one of them is served; disjoint9: both are"""
    got = {s.name: _walk(s) for s in HAND}
    count = {k: d["lds_loads"] + d["lds_stores"] for k, d in got.items()}
    print("LDS-slot plan, HBM transfers removed per pass:", count)
    assert count["root6"] == 3 and count["nested9"] == 3 and count["disjoint9"] == 6
    assert (got["disjoint9"]["lds_loads"], got["disjoint9"]["lds_stores"], got["disjoint9"]["lds_copies"]) == (4, 2, 2)
    assert any(count[k] > 0 for k in count if k.startswith("unrooted"))


@pytest.mark.parametrize("ntaxa", [3, 12, 40])
def test_a_caterpillar_flags_nothing(ntaxa):
    par, lot = _caterpillar(ntaxa)
    d = _walk(Shape(f"caterpillar{ntaxa}", par, lot))
    assert not (d["nrec"][:, REC_FLAGS] & LDS_BITS).any()
    assert (d["lds_loads"], d["lds_stores"], d["lds_copies"]) == (0, 0, 0)


def test_only_the_twenty_state_layout_is_planned():
    """no other layout has a device backend with a slot (class-fused and 4-state walks ignore the bits anyway)"""
    for mdl in (synthetic.dna_model(0.7, 4), synthetic.dna_model(0.7, 3)):
        for shape in HAND:
            d = _walk(shape, mdl)
            assert not (d["nrec"][:, REC_FLAGS] & LDS_BITS).any() and d["lds_loads"] == d["lds_stores"] == 0


def test_switched_off_the_records_are_the_plain_ones():
    bench, blen = bench64()
    was = engine.lds_slot()
    try:
        for shape, bl in [(s, None) for s in HAND] + [(bench, blen)]:
            engine.lds_slot(True)
            on = _walk(shape, blen=bl)
            assert engine.lds_slot(False) is True
            off = _walk(shape, blen=bl)
            assert not (off["nrec"][:, REC_FLAGS] & LDS_BITS).any()
            assert (off["lds_loads"], off["lds_stores"], off["lds_copies"]) == (0, 0, 0)
            plain = on["nrec"].copy()
            plain[:, REC_FLAGS] &= ~LDS_BITS
            assert np.array_equal(off["nrec"], plain)
            for key in ("ldsched", "msched", "slot"):
                assert np.array_equal(on[key], off[key]), key
            for key in ("loads", "stores", "products", "leaf_ops"):
                assert on[key] == off[key], key
    finally:
        engine.lds_slot(was)


def test_benchmark_tree_count():
    """64 taxa, seed 20260101: six nodes have two visited children; one slot serves four of the six U pairs and four of the
    six inside loads (the other two nodes are nested inside an occupied interval): 12 of the 106 transfers of a pass"""
    bench, blen = bench64()
    d = _walk(bench, blen=blen)
    _replay(d["nrec"])
    two_visited = sum(1 for r in d["nrec"] if r[REC_A + CH_KIND] == KIND_STORED and r[REC_B + CH_KIND] == KIND_STORED)
    count = d["lds_loads"] + d["lds_stores"]
    print(f"benchmark tree: {two_visited} two-visited nodes, {count} of {d['loads'] + d['stores']} transfers through the LDS slot "
          f"({d['lds_loads']} loads, {d['lds_stores']} stores, {d['lds_copies']} copies)")
    assert (d["products"], d["loads"], d["stores"]) == (201, 56, 50)
    assert two_visited == 6
    assert (count, d["lds_loads"], d["lds_stores"], d["lds_copies"]) == (12, 8, 4, 4)
    # the same optimum from the records alone (12 candidates: brute force over 4 096 subsets)
    assert count == _brute_force(_candidates(d["nrec"]))
