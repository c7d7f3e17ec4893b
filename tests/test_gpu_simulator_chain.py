"""-m gpu: the null's LDS-table simulator (simulate_chain_kernel, cmx_simulate.hip) at small sizes.

The kernel normally serves calls of 75 000 sites and more, with one batch of 1 024 sites per workgroup, and with four
from 4 Mi sites on (the shape the benchmark's target runs); engine.sim_sites(min_sites=0) makes it serve every call
with an even number of sites, and four_batch_sites = 0 / huge picks the four-batch / one-batch shape, so the cases here
are a few thousand sites.  Its draws are pinned bit for bit: every call must give the bytes of oracle.simulate at the
same g in BOTH shapes, and so must the gather kernel (simulate_blocked_kernel, min_sites above the call).

What can go wrong in the kernel, and the case that would show it:
* the search compares a draw's 32-bit word with the host's integer thresholds instead of u = w / 2^32 with the running
  sums: every case checks that against the oracle's doubles; the tree `edges` has branches of length 0 (running sums of
  exactly 0 and 1: no threshold for the one, a saturated one for the other), 1e-9 (sums within 2^-32 of 0 and 1) and 60
  (rows equal to the stationary frequencies);
* a node's parent states are loaded one node ahead, or taken from registers when the parent is the node just drawn:
  the rooted 3-taxon tree and the caterpillar have such a node on every level, the balanced tree and the benchmark
  tree on none but the first;
* a workgroup draws one batch of 1 024 sites, or four from one copy of a node's tables: 2 sites, one pair short of a
  batch, a batch, a batch and a pair, 2 .. 4 batches and a pair, 5 batches and a pair, 6 batches and two pairs, 6 batches
  over two replicates -- in the four-batch shape a last workgroup with some batches full, one partial and the rest off,
  in every combination up to a full workgroup and one pair; and once 4 Mi sites and a pair through the built-in
  threshold, compared with the gather kernel;
* a pair of sites is stored as one 16-bit word for an even rep_ram and as two bytes, the second possibly in the next
  replicate block, for an odd one;
* a thread stages two 16-byte pieces of a node's block (up to 16 384 B: six classes of 20 states) or three, each with one
  and with four batches: every tree and the models of four and six classes run the two-piece shapes, with even and odd
  rep_ram, the model sets below the three-piece shapes;
* the kernel serves the models whose node block fits three 16-byte pieces per thread (cmx_layout.h: sim_has_tables) and
  every other model takes the gather kernel whatever min_sites says: model sets on both sides of that rule
  (tests/model_sets.py: CHAIN_EDGE_CASES) -- 20 states x 9 classes (a block of 23 040 B, three pieces), 64 x 1 (the longest
  row, 68 thresholds, and states up to 63 in a pair's 8-bit halves), 61 x 1, and 7 x 50 and 61 x 2 without tables --
  against eng.simulate byte for byte and against the oracle off its fragile sites.

Not here: the issue's plan of keeping the parents' states in LDS slots was not built, so there is no slot
plan and no fallback for a live set that does not fit."""
import numpy as np
import pytest

import model_sets as ms
import oracle
from comap_amd import engine, synthetic
from lds_slot_trees import bench64
from tree_shapes import _arrays, _balanced, _caterpillar, _parse

pytestmark = pytest.mark.gpu

BATCH = 1024   # sites of one batch of a workgroup (512 threads, a pair of sites each)
SEED = 4711
FRAGILE_CAP = 1e-3   # tests/test_oracle_model_sets.py holds the oracle to it on the same ranges


def _trees():
    p3, l3 = _arrays(_parse("((x,x),x)"), seed=3)
    pc, lc = _caterpillar(12)
    pb, lb = _balanced(16)
    b64, blen64 = bench64()
    pe, le = _balanced(8)
    blen_e = np.array([0.0, 1e-9, 60.0, 0.3, 0.0, 0.0, 1e-9, 0.2, 60.0, 0.0, 0.1, 1e-9, 0.0, 60.0, 0.0])
    return {"rooted3": (p3, l3, None), "caterpillar12": (pc, lc, None), "balanced16": (pb, lb, None),
            "bench64": (b64.parent, b64.lot, blen64), "edges": (pe, le, blen_e)}


TREES = _trees()
# (rep_begin, rep_end, rep_ram): n = (rep_end - rep_begin) * 2 * rep_ram sites
H = BATCH // 2
CALLS = ([(0, 1, 1), (0, 1, H - 1), (3, 5, H // 2), (0, 1, H + 1), (0, 1, H + 2)] + [(0, 1, k * H + 1) for k in (2, 3, 4, 5)]
         + [(1, 2, 4 * H + 2), (0, 1, 6 * H + 2), (2, 4, 3 * H)])
ONE, FOUR = 1 << 40, 0     # four_batch_sites: no call reaches it / every call does
_cache = {}


def _setup(tree, ncat):
    key = (tree, ncat)
    if key not in _cache:
        parent, lot, blen = TREES[tree]
        nn = len(parent)
        if blen is None:
            blen = np.random.default_rng(nn).uniform(0.05, 0.6, size=nn)
            blen[-1] = 0.0
        mdl = synthetic.protein_model(0.5, ncat)
        args = (np.asarray(parent, dtype=np.int32), blen, np.asarray(lot, dtype=np.int32), mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
        _cache[key] = (oracle.Model(*args), engine.Engine(*args), len(lot))
    return _cache[key]


def _null_aln(eng, T, rb, re, ram, min_sites, four=-1, seed=SEED):
    import torch
    engine.sim_sites(min_sites, four)
    try:
        buf = torch.full(((re - rb) * 2 * T * ram,), 255, dtype=torch.uint8, device="cuda:0")
        eng.null_simulate_dev(seed, rb, re, ram, buf)
        torch.cuda.synchronize()
        return buf.cpu().numpy().reshape(re - rb, 2, T, ram)
    finally:
        engine.sim_sites(-1, -1)


def _check(tree, ncat, calls):
    om, eng, T = _setup(tree, ncat)
    for rb, re, ram in calls:
        n = (re - rb) * 2 * ram
        want, _ = oracle.simulate(om, SEED, rb * 2 * ram, n)          # [T, n], column s <-> g = rb * 2 * ram + s
        want = want.reshape(T, re - rb, 2, ram).transpose(1, 2, 0, 3)
        for four, what in ((ONE, "chain kernel, one batch"), (FOUR, "chain kernel, four batches")):
            assert np.array_equal(_null_aln(eng, T, rb, re, ram, 0, four), want), (tree, ncat, rb, re, ram, what)
        assert np.array_equal(_null_aln(eng, T, rb, re, ram, 1 << 40), want), (tree, ncat, rb, re, ram, "gather kernel")


@pytest.mark.parametrize("tree", list(TREES))
def test_protein_gamma4_every_size(tree):
    _check(tree, 4, CALLS)


@pytest.mark.parametrize("tree", list(TREES))
def test_six_classes_take_the_other_launch_shapes(tree):
    _check(tree, 6, CALLS)


def test_four_batches_per_workgroup():
    """4 Mi sites and a pair: the four-batch launch shape by the built-in threshold, its last workgroup holding one pair;
    the gather kernel draws the same call, and the first and last columns of every replicate block are the oracle's"""
    om, eng, T = _setup("caterpillar12", 4)
    rb, re, ram = 1, 2, (1 << 21) + 1
    got = _null_aln(eng, T, rb, re, ram, -1)
    assert np.array_equal(got, _null_aln(eng, T, rb, re, ram, 1 << 40))
    for batch in (0, 1):
        for lo, hi in ((0, 1500), (ram - 1500, ram)):
            g = (rb * 2 + batch) * ram
            want, _ = oracle.simulate(om, SEED, g + lo, hi - lo)
            assert np.array_equal(got[0, batch, :, lo:hi], want)


@pytest.mark.parametrize("name", ms.CHAIN_EDGE_CASES)
def test_models_on_both_sides_of_the_table_rule(name):
    """an odd rep_ram, an even one and two replicates, through both batch shapes (the gather kernel for a model without
    tables) and through the gather kernel by min_sites"""
    c = ms.case(name)
    eng, om, T = ms.engine_of(c), ms.oracle_of(c), len(c["lot"])
    try:
        for rb, re, ram in ms.CHAIN_EDGE_CALLS:
            g0, n = rb * 2 * ram, (re - rb) * 2 * ram
            assert n <= 6148
            plain, _ = eng.simulate(ms.CHAIN_EDGE_SEED, g0, n)
            want, _, near = oracle.simulate(om, ms.CHAIN_EDGE_SEED, g0, n, want_near=True)
            frag = ms.fragile(near)
            print(f"{name} {(rb, re, ram)}: {int(frag.sum())} fragile of {frag.size} sites left out")
            assert frag.mean() <= FRAGILE_CAP
            for min_sites, four, what in ((0, ONE, "one batch"), (0, FOUR, "four batches"), (1 << 40, -1, "gather kernel")):
                got = _null_aln(eng, T, rb, re, ram, min_sites, four, seed=ms.CHAIN_EDGE_SEED)
                got = got.transpose(2, 0, 1, 3).reshape(T, n)
                assert np.array_equal(got, plain), (name, rb, re, ram, what)
                assert np.array_equal(got[:, ~frag], want[:, ~frag]), (name, rb, re, ram, what)
    finally:
        eng.close()


def test_under_the_scratch_guard():
    """the states scratch is sized [nn][n]: no batch, partial or outside n, writes past it"""
    parent, lot, blen = TREES["bench64"]
    mdl = synthetic.protein_model(0.5, 4)
    args = (parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    om = oracle.Model(*args)
    was = engine.scratch_guard(True)
    try:
        engine.scratch_guard_failures(clear=True)
        eng = engine.Engine(*args)
        for rb, re, ram in ((0, 1, H + 1), (1, 2, 4 * H + 2), (0, 1, 5 * H + 1)):
            n = (re - rb) * 2 * ram
            want, _ = oracle.simulate(om, SEED, rb * 2 * ram, n)
            for four in (ONE, FOUR):
                got = _null_aln(eng, len(lot), rb, re, ram, 0, four)
                assert np.array_equal(got, want.reshape(len(lot), re - rb, 2, ram).transpose(1, 2, 0, 3))
        eng.scratch_check()
        eng.close()
        assert engine.scratch_guard_failures() == []
    finally:
        engine.scratch_guard(was)
