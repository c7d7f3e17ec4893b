"""-m gpu: the three simulators on trees beyond 64 leaves (tests/large_tree_cases.py), bit for bit against oracle.simulate at
the same g, as test_gpu_simulator_chain._check does on trees of 3 to 64 leaves.

What a larger tree adds to simulate_kernel, simulate_blocked_kernel (the gather kernel) and simulate_chain_kernel
(cmx_simulate.hip), and the case that reaches it:
* more than 126 nodes (u66, 130) and node indices above 255 (u131, 260 nodes; cat130, 259): the order and the groups of
  four that the host stages per level (simord, simg), and the states scratch [nn][n];
* many levels and long parent chains: cat130 has 129 levels and, on every one of them, a node whose parent is the node just
  drawn (the chain shortcut); bal128 has 7 levels of up to 128 nodes; multi140 has 2 to 5 children under every node;
* myo: the reference's own example tree (56 branches of length 1e-6) under its own model;
* u131 with six rate classes: the largest node block that a thread stages as two 16-byte pieces, on 260 nodes.

Every case: eng.simulate (alignment and classes, 700 sites from an odd g0) and eng.null_simulate_dev through
engine.sim_sites in all three shapes -- the chain kernel with one batch per workgroup, with four, and the gather kernel --
for a pair of sites, a batch and a pair with an odd rep_ram, a full four-batch workgroup and a pair with an even rep_ram in
replicate 1, and two replicates.  tests/test_large_tree_cases.py proves that no site of these ranges is fragile, so nothing
is left out.  The simulate_kernel side of the unfused null (rep_ram and gstep) runs in test_gpu_large_tree_null.py."""
import numpy as np
import pytest

import large_tree_cases as ltc
import oracle
from comap_amd import engine
from test_gpu_simulator_chain import FOUR, ONE, _null_aln

pytestmark = pytest.mark.gpu

SHAPES = ((0, ONE, "chain kernel, one batch"), (0, FOUR, "chain kernel, four batches"), (1 << 40, -1, "gather kernel"))


def _want(om, rb, re, ram):
    n = (re - rb) * 2 * ram
    aln, _ = oracle.simulate(om, ltc.CHAIN_SEED, rb * 2 * ram, n)          # [T, n], column s <-> g = rb * 2 * ram + s
    return aln.reshape(om.T, re - rb, 2, ram).transpose(1, 2, 0, 3)


@pytest.mark.parametrize("case", ltc.SIM_CASES)
def test_simulate_is_the_oracle_bit_for_bit(case):
    om, eng = ltc.oracle_of(case), ltc.engine_of(case)
    aln, cls = eng.simulate(ltc.SIM_SEED, ltc.SIM_G0, ltc.SIM_N)
    aln_o, cls_o = oracle.simulate(om, ltc.SIM_SEED, ltc.SIM_G0, ltc.SIM_N)
    assert np.array_equal(cls, cls_o)
    assert np.array_equal(aln, aln_o), int((aln != aln_o).any(axis=0).sum())


@pytest.mark.parametrize("case", ltc.SIM_CASES)
def test_the_nulls_simulator_in_its_three_shapes(case):
    om, eng = ltc.oracle_of(case), ltc.engine_of(case)
    assert ltc.H == 512
    for rb, re, ram in ltc.CHAIN_CALLS:
        want = _want(om, rb, re, ram)
        for min_sites, four, what in SHAPES:
            got = _null_aln(eng, om.T, rb, re, ram, min_sites, four, seed=ltc.CHAIN_SEED)
            assert np.array_equal(got, want), (case, rb, re, ram, what, int((got != want).any(axis=(0, 1, 2)).sum()))


def test_under_the_scratch_guard():
    """the states scratch is [nn][n] with nn = 260: no shape writes past it"""
    case = "u131-p4"
    om = ltc.oracle_of(case)
    was = engine.scratch_guard(True)
    try:
        engine.scratch_guard_failures(clear=True)
        eng = ltc.new_engine(case)
        for rb, re, ram in ltc.CHAIN_CALLS[1:]:
            want = _want(om, rb, re, ram)
            for min_sites, four, what in SHAPES:
                got = _null_aln(eng, om.T, rb, re, ram, min_sites, four, seed=ltc.CHAIN_SEED)
                assert np.array_equal(got, want), (rb, re, ram, what)
        eng.scratch_check()
        eng.close()
        assert engine.scratch_guard_failures() == []
    finally:
        engine.scratch_guard(was)
