"""The oracle-only preconditions of tests/large_tree_cases.py, so that a failure of tests/test_gpu_large_tree_simulators.py
or tests/test_gpu_large_tree_null.py can be read as the device's:

* every tree has the B, nn and T its table states, and the shape it is there for (cherries, levels, children per node);
* the engine does not rescale by default, and a case that underflowed would compare NaN with NaN: oracle.map_sites of
  every alignment a null of those files maps -- its own draws, the forced repeats, the inter-gene and the continuous-rate
  draws -- has a finite logL on every site, finite counts, and a statistic that is finite for every kind the case runs;
* the forced-repeat alignments have exactly 171 distinct columns, strictly between 128 (two tiles) and their 222 sites;
* no (tree, model) pair draws a fragile site (a draw within oracle.FRAGILE of a boundary of its cumulative row) on any
  range the GPU tests compare bit for bit: they have no exclusions;
* the reference those files use, composed from oracle.simulate, oracle.map_sites and oracle.stat_pair, is
  oracle.null_intra / oracle.null_inter byte for byte;
* no branch total of the unfused null lies within 1e-6 relative of a bound of its MI statistic (a count the device has to
  1e-6 could otherwise fall into the neighbouring class)."""
import numpy as np
import pytest

import large_tree_cases as ltc
import model_sets as ms
import oracle

KEYS = ("stat", "nmin", "prmin", "rcmin")


@pytest.mark.parametrize("name", list(ltc.SIZES))
def test_the_trees_are_what_the_table_says(name):
    parent, blen, lot = ltc.tree(name)
    B, nn, T = ltc.SIZES[name]
    assert (len(parent) - 1, len(parent), len(lot)) == (B, nn, T)
    assert parent[-1] == -1 and blen[-1] == 0.0 and (blen[:-1] > 0).all() and (parent[:-1] > np.arange(nn - 1)).all()
    nkids = np.bincount(parent[:-1], minlength=nn)
    assert (nkids[lot] == 0).all() and (nkids > 0).sum() == nn - T
    inner = nkids[nkids > 0]
    depth = np.zeros(nn, dtype=int)
    for n in range(nn - 2, -1, -1):
        depth[n] = depth[parent[n]] + 1
    if name in ("u65", "u66", "u131"):
        assert B == 2 * T - 3 and nkids[-1] == 3 and (inner[:-1] == 2).all()
    if name in ("r65", "bal128", "cat130"):
        assert B == 2 * T - 2 and (inner == 2).all()
    if name == "bal128":
        assert T % 16 == 0 and len(ltc.cherries(name)) == 64 and depth.max() == 7
        assert 64 * 4 * 400 * 192 < 32 << 20                   # its message table is under the byte limit
    if name == "cat130":
        assert len(ltc.cherries(name)) == 1 and depth.max() == 129
    if name == "multi140":
        assert inner.min() == 2 and inner.max() == 5 and nkids[-1] >= 3 and all((inner == k).any() for k in (2, 3, 4, 5))
    if name in ("u65", "r65", "u66", "u131"):
        assert len(ltc.cherries(name)) >= 1
    assert {"u65": B == 127, "r65": B == 128, "u66": B == 129}.get(name, True)      # kMomentRows = 128 between them
    if name in ("u66", "u131"):
        assert ((T + 15) // 16, T % 16) == {"u66": (5, 2), "u131": (9, 3)}[name]
    if name == "u131":
        assert nn > 256


@pytest.mark.parametrize("case", ltc.NULL_CASES)
def test_no_null_alignment_underflows_and_every_statistic_is_finite(case):
    for inp in ltc.INPUTS:
        ref = ltc.mapped(case, inp)
        assert np.isfinite(ref["logL"]).all(), (inp, int((~np.isfinite(ref["logL"])).sum()))
        assert all(np.isfinite(c).all() for c in ref["counts"]), inp
        assert np.isfinite(ref["nmin"]).all() and np.isfinite(ref["prmin"]).all()
        for kind in ltc.null_kinds(case):
            assert np.isfinite(ltc.reference(case, inp, kind)["stat"]).all(), (inp, kind)


@pytest.mark.parametrize("case", ltc.NULL_CASES)
def test_the_forced_repeats_have_171_distinct_columns(case):
    sup = ltc.alignments(case, ltc.FORCED)
    om = ltc.oracle_of(case)
    nrep, ram = ltc.FORCED_SHAPE
    assert sup.shape == (nrep, 2, om.T, ram) and sup.max() < om.S
    assert 128 < ltc.distinct(sup) == ltc.FORCED_PATTERNS < nrep * 2 * ram


@pytest.mark.parametrize("case", ltc.PROTEIN_CASES)
def test_large_trees_make_nearly_every_simulated_column_distinct(case):
    """why the forced repeats exist; yet every drawn input has a few repeats, so the pattern count is told from the site count"""
    for inp, (nrep, ram) in ltc.NULL_INPUTS.items():
        n = ltc.distinct(ltc.alignments(case, inp))
        assert 0.5 * nrep * 2 * ram < n <= nrep * 2 * ram, (inp, n)


def test_no_range_of_the_gpu_tests_draws_a_fragile_site():
    bad = {}
    for label, om, seed, g0, n in ltc.discrete_ranges():
        near = oracle.simulate(om, seed, g0, n, want_near=True)[2]
        if ms.fragile(near).sum() != 0:
            bad[label] = int(ms.fragile(near).sum())
    assert bad == {}
    _, near = ltc.continuous_alignments(want_near=True)
    assert ms.fragile(near).sum() == 0


@pytest.mark.parametrize("case,inp,kinds", [("u66-p4", "3x53", ltc.KINDS), ("u131-p4", "2x48", (0,)), ("u66-k2", "3x53", (1,)),
                                            ("bal128-d5", "2x48", (0, 1)), ("myo-p4", "forced", (4,))])
def test_the_composed_reference_is_oracle_null_intra(case, inp, kinds):
    """every kind on one case (the statistic's code is the same on every tree), one kind each on the largest tree, two
    substitution types, nucleotides and supplied alignments"""
    om = ltc.oracle_of(case)
    nrep, ram = ltc.shape_of(inp)
    for kind in kinds:
        if inp == ltc.FORCED:
            o = oracle.null_intra(om, kind, 0, 0, nrep, ram, supplied=ltc.alignments(case, inp))
        else:
            o = oracle.null_intra(om, kind, ltc.null_seed(case), 0, nrep, ram)
        ref = ltc.reference(case, inp, kind)
        for k in KEYS:
            assert o[k].dtype == ref[k].dtype and o[k].tobytes() == ref[k].tobytes(), (kind, k)


def test_the_unfused_inputs_of_u131():
    """the unfused null (MI with bounds), the inter-gene null and the continuous-rate null of UNFUSED_CASE"""
    case = ltc.UNFUSED_CASE
    om = ltc.oracle_of(case)
    ref = ltc.unfused_mapped()
    assert np.isfinite(ref["logL"]).all()
    k = ltc.UNFUSED
    o = oracle.null_intra(om, oracle.ST_DISCRETE_MI, k["seed"], 0, k["nrep"], k["ram"], params=ltc.mi_params())
    st = ltc.stat_of(ref, oracle.ST_DISCRETE_MI, ltc.mi_params())
    assert o["stat"].tobytes() == st.tobytes() and np.isfinite(st).all() and (st > 0).any()
    for c in ref["counts"]:
        tot = c.sum(-1)
        assert tot.min() >= ltc.MI_BOUNDS[0] and tot.max() < ltc.MI_BOUNDS[-1]
        gap = np.abs(tot[:, :, None] / ltc.MI_BOUNDS[None, None, 1:] - 1.0)
        assert gap.min() > 1e-6, gap.min()
    # inter: the second data set is the same tree with every branch 1.3 times as long
    k = ltc.INTER
    om2 = ltc.oracle_of(case, k["blen_scale"])
    nrep = k["rep_end"] - k["rep_begin"]
    o = oracle.null_inter(om, om2, 0, k["seed"], k["rep_begin"], k["rep_end"], k["ram"])
    assert all(np.isfinite(o[key]).all() for key in KEYS)
    a1 = oracle.simulate(om, k["seed"], k["rep_begin"] * 2 * k["ram"], nrep * 2 * k["ram"])[0]
    a2 = oracle.simulate(om2, k["seed"], k["rep_begin"] * 2 * k["ram"], nrep * 2 * k["ram"])[0]
    assert (a1 != a2).mean() > 0.01                         # the scaled tree draws other alignments
    # continuous rates
    sup = ltc.continuous_alignments()
    ref = ltc.compose(om, om, sup)
    assert np.isfinite(ref["logL"]).all() and np.isfinite(ltc.stat_of(ref, 0)).all()
