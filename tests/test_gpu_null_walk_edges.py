"""-m gpu: every device path of the null over supplied alignments against 50-digit answers, at branch and rate edges.

The answers and the bars are those of tests/null_walk_cases.py (from the fixtures tests/golden/operator_edges.npz and
tests/golden/null_walk_edges.npz alone; tests/test_null_walk_reference.py shows on the CPU that the oracle meets them a
thousandfold and that they are what the counts' own bar allows): nmin to the counts' relative bar (1e-9 unless the fp64 closed
form itself needs more) beside the operator's absolute term, prmin to 1e-12, rcmin equal where the classes are clear, the
statistic to a first-order perturbation bound of that counts bar (a few 1e-9 for the normalised kinds), Cosubstitution equal,
MI to the rounding of its logarithms.  The supplied pairs (null_walk_cases.supplied_pairs) are the fixture's resolved columns
against themselves rotated, reversed and unchanged: 198 pairs on the trees of 4 and 5 leaves, 135 on the 12-leaf tree.

Paths:
  * 20 states, unfused classes: map_kernel<20, patterns, msg>, <20, patterns>, <20, null, msg> and <20, null> -- the cherry
    message table on and off times the pattern path on and off; of the table's 400 rows of a zero-length cherry only the 20
    with s1 == s2 are possible: the other 380 are exact zeros under a rate-zero class (P = I) and below the rounding of
    V Vinv under a positive rate;
  * nucleotides with 4 or 5 rate classes: the class-fused 16- and 20-state layouts with their cherry tables, per site and by
    pattern; one class: the unfused layout with the row-reusing cherry visit, both;
  * the unfused null (simulate -> observed kernels -> pair_diag_kernel): 7 and 61 states, and 20 states with likelihood scaling.

Each test prints error / bar of every output per path and kind (`pytest -s`)."""
import numpy as np
import pytest

import null_walk_cases as nw
import operator_edge_cases as oe
import test_gpu_operator_edges as gpu_edges
import test_null_walk_reference as ref
from comap_amd import engine
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu

KINDS = (0, 4, 3, 1, 7, 2, 5)        # 0 and 4 first: on the pattern path they go through the moments


def _engine(c):
    return engine.Engine(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"], Bk=oe.register_of(c),
                         clamp_negative=bool(c["clamp"]))


def _tables(name):
    """inlined cherries of the case's tree"""
    return 4 if name in oe.DEEP_CASES else 2


def _run(eng, name, path, kinds=KINDS):
    """the null over the case's supplied pairs for every kind, against the expected outputs at their bars"""
    sup, _, _ = ref.pairs(name)
    for kind in kinds:
        exp = ref.expected(name, kind)
        got = eng.null_intra(kind, 0, 0, 3, sup.shape[3], supplied=sup, threshold=nw.MI_THRESHOLD)
        fig = nw.figures(got, exp, name)
        print(f"{path:>22s} {name:26s} {nw.KIND_NAMES[kind]:17s} nmin {fig['nmin']:.1e} prmin {fig['prmin']:.1e} "
              f"stat {fig['stat']:.1e} compared {fig['compared']} left out {fig['left_out']}")
        assert np.isfinite(got["nmin"]).all() and np.isfinite(got["prmin"]).all()
        assert nw.leaves_out(name, kind) or fig["left_out"] == 0
        for key in ("nmin", "prmin", "rcmin", "stat"):
            assert fig[key] <= 1.0, (path, name, nw.KIND_NAMES[kind], key, fig[key])


def _patterns(eng, name, path, kinds=KINDS):
    try:
        for on in (True, False):
            eng.set_null_patterns(on)
            _run(eng, name, f"{path}{', patterns' if on else ', per site'}", kinds)
    finally:
        eng.set_null_patterns(None)


def _zero_cherry_rows_are_zero(eng, c):
    """the cherry whose two leaves have no length: a row 20 s1 + s2 with s1 != s2 is sum_z P[x, z] P_1[z, s1] P_2[z, s2] with
    an off-diagonal of P(0) in every term.  Under a rate-zero class P(0) is the identity itself and the 380 rows are exact
    zeros.  Under a positive rate the host keeps the eigen product V Vinv at t = 0 (cmx_host_model.cpp), whose
    off-diagonals are not 0 but at most eta = S eps max(|V| |Vinv|) in size: the rows are at most 2 eta (the rows of P sum
    to 1), against messages of order 1e-2 ... 1 in the 20 rows s1 == s2."""
    table, nodes = eng.cherry_msg_table()
    zero = [i for i, (_, l1, l2) in enumerate(nodes) if c["blen"][l1] == 0.0 and c["blen"][l2] == 0.0]
    assert len(zero) == 1
    rows = table[:, zero[0]].reshape(len(c["rates"]), 20, 20, 20)
    off = ~np.eye(20, dtype=bool)
    _, V, Vinv = npo.eigen_reversible(c["Q"], c["pi"])
    eta = 20 * np.finfo(np.float64).eps * float(np.max(np.abs(V) @ np.abs(Vinv)))
    for cls, rate in enumerate(c["rates"]):
        worst = float(np.abs(rows[cls][off]).max())
        print(f"    zero-length cherry, class {cls} (rate {rate:.3g}): largest |entry| of the 380 rows {worst:.1e}, 2 eta {2 * eta:.1e}")
        assert worst == 0.0 if rate == 0.0 else worst <= 2 * eta
        assert (rows[cls][~off].max(axis=-1) > 1e-3).all()


@pytest.mark.parametrize("name", [n for n in ref.WALK_CASES if oe.Inputs(n).S == 20])
def test_protein_null_walks(name):
    c = ref.case(name)
    was = engine.cherry_msg()
    try:
        for table in (True, False):
            engine.cherry_msg(table)
            eng = _engine(c)
            info = eng.cherry_msg_info()
            assert info["tables"] == (_tables(name) if table else 0), info
            assert eng.info()["cherry_tables"] == 0
            if table and name.rsplit("-", 1)[1] in ("q1", "p2"):
                _zero_cherry_rows_are_zero(eng, c)
            _patterns(eng, name, "20 states, table" if table else "20 states, no table")
            eng.close()
    finally:
        engine.cherry_msg(was)


@pytest.mark.parametrize("name", [n for n in ref.WALK_CASES if oe.Inputs(n).S == 4])
def test_nucleotide_null_walks(name):
    c = ref.case(name)
    eng = _engine(c)
    info, C = eng.info(), len(c["rates"])
    if C == 1:
        assert info["device_states"] == 4 and info["cherry_tables"] == 0
        path = "4 states, unfused"
    else:
        assert info["device_states"] == 4 * C
        assert info["cherry_tables"] == 4 if name in oe.DEEP_CASES else info["cherry_tables"] >= 2, info
        path = f"{4 * C} fused states"
    _patterns(eng, name, path)


@pytest.mark.parametrize("name", oe.DEEP_CASES)
def test_observed_mapping_meets_the_deep_fixture(name):
    """the observed walk of the 12-leaf tree, as test_gpu_operator_edges holds the trees of 4 and 5 leaves: counts 1e-9
    beside the operator's absolute term, exact zeros on zero-length branches, logL and post_rate 1e-12.  The signed
    register on the 1e-100 branch is the case in which an entry of P that is exactly 0 lost J(x, y) to the non-finite guard
    (2e-3 of a count in the oracle before the joint operator kept it)."""
    c = ref.case(name)
    gpu_edges._check(_engine(c).map_sites(c["aln"]), c, ref.rows()[name])


UNFUSED = [n for n in oe.CASES if n.startswith(("s7", "s61"))]


@pytest.mark.parametrize("name", UNFUSED + ["protein-g4-t5-p6", "protein-g4-t12-q3"])
def test_unfused_null(name):
    """null_unfused_dev, then the observed kernels, then pair_diag_kernel: the plain kernels (7 states), the wide ones (61)
    and the scaled walk of a 20-state model"""
    c = ref.case(name)
    eng = _engine(c)
    if len(c["pi"]) == 20:
        eng.set_likelihood_scaling(True)
    _run(eng, name, f"unfused, {len(c['pi'])} states", kinds=(0,))


def test_a_supplied_unknown_is_refused():
    c = ref.case("protein-g4-t5-p1")
    sup, _, _ = ref.pairs("protein-g4-t5-p1")
    bad = sup.copy()
    bad[2, 1, 3, 17] = 20
    eng = _engine(c)
    with pytest.raises(engine.CmxError, match="fully resolved"):
        eng.null_intra(0, 0, 0, 3, sup.shape[3], supplied=bad)
    _run(eng, "protein-g4-t5-p1", "after a refusal", kinds=(0,))
