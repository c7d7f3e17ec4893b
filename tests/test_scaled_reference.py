"""tests/scaled_reference.py pinned on the CPU: the numpy restatement of the mapping with per-site power-of-two scaling that
tests/test_gpu_likelihood_scaling.py holds the device against.

1. Where nothing underflows it is the oracle's mapping (oracle.c, uniformization counts), and scaling on / off inside the
   reference gives the same bits: counts, norms, posterior rates and rate classes.  logL is ln(mantissa) + exponent ln 2 by
   definition, so where a rescale took place (150 protein taxa: vectors fall below 2^-256 without leaving fp64) it equals
   ln(L) to rounding, not to the bit; on a small tree, where no rescale takes place, to the bit as well.
2. Where fp64 underflows it is the unscaled computation in long double (x87 extended, exponents down to -16382): counts to
   1e-12, logL to 1e-13, rate classes equal; every case holds at least two sites the C oracle loses (logL = -inf) and at
   least two it keeps, so none of this can pass on a case that never underflows.  The three mapping variants and marginal
   ancestral states get both pins at the smallest shape; where a variant chooses states (no averaging) the counts are
   compared where the choice is clear in the long-double run (the two best candidates more than 1e-9 apart, relative).
3. A star of 320 leaves, where one node's product underflows on its own: only the per-factor rule can pass."""
import numpy as np
import pytest

import oracle
import ancestral_reference as ar
import scaled_cases as sc
import scaled_reference as sr
from conftest import make_case, rel_close

needs_long_double = pytest.mark.skipif(not sr.has_extended_range(), reason="long double has no extended exponent range here")


def _model_args(case):
    return (case["parent"], case["blen"], case["lot"], case["aln"], case["Q"], case["pi"], case["rates"], case["probs"])


@pytest.mark.parametrize("ntaxa,nstates", [(150, 20), (150, 4), (12, 20)])
def test_reference_is_the_oracle_where_nothing_underflows(ntaxa, nstates):
    case = make_case(ntaxa, 16, nstates, 4321)
    om = oracle.Model(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    ops = sr.operators(case["parent"], case["blen"], case["Q"], case["pi"], case["rates"])
    on, off = sr.map_sites(*_model_args(case), ops=ops), sr.map_sites(*_model_args(case), ops=ops, scale=False)
    o = oracle.map_sites(om, case["aln"])
    assert np.isfinite(o["logL"]).all()
    rel_close(on["counts"], o["counts"], 1e-10, 1e-300)
    rel_close(on["norm"], o["norm"], 1e-10)
    rel_close(on["logL"], o["logL"], 1e-12)
    rel_close(on["post_rate"], o["post_rate"], 1e-12)
    assert np.array_equal(on["rate_class"], o["rate_class"])
    for k in ("counts", "norm", "post_rate", "rate_class"):
        assert np.array_equal(on[k], off[k]), k
    rel_close(on["logL"], off["logL"], 4e-16)
    if ntaxa == 12:
        assert np.array_equal(on["logL"], off["logL"])
    # the variants and the ancestral states: the same bits scaled and unscaled, and the oracle's / the ASR reference's values
    for average, joint in sc.OPTIONS[1:]:
        a = sr.map_sites(*_model_args(case), ops=ops, average=average, joint=joint)
        b = sr.map_sites(*_model_args(case), ops=ops, average=average, joint=joint, scale=False)
        assert np.array_equal(a["counts"], b["counts"]), (average, joint)
        if ntaxa == 12:
            o = oracle.map_sites_noavg(om, case["aln"]) if joint else oracle.map_sites_marginal(om, case["aln"], average)
            clear = a["margin"] > 1e-9
            assert clear.mean() > 0.9
            assert np.allclose(a["counts"][clear], o["counts"][clear], rtol=1e-9, atol=1e-13)
    a, b = sr.ancestral_states(*_model_args(case), ops=ops), sr.ancestral_states(*_model_args(case), ops=ops, scale=False)
    assert np.array_equal(a["post"], b["post"]) and np.array_equal(a["states"], b["states"])
    if ntaxa == 12:
        r = ar.ancestral_states(case["parent"], case["blen"], case["lot"], case["Q"], case["rates"], case["probs"], case["pi"], case["aln"])
        assert a["nodes"] == r["nodes"]
        assert np.allclose(a["post"], r["post"], rtol=1e-9, atol=1e-13)


def _check_against_long_double(case, kept=2):
    lost = np.isinf(oracle.map_sites(case.om, case.aln)["logL"])
    assert lost.sum() >= 2 and (~lost).sum() >= kept, lost
    r, l = case.reference(), case.reference(dtype=np.longdouble, scale=False)
    assert np.isfinite(r["logL"]).all() and np.isfinite(r["counts"]).all()
    rel_close(r["counts"], l["counts"], 1e-12, 1e-300)
    rel_close(r["norm"], l["norm"], 1e-12)
    rel_close(r["logL"], l["logL"], 1e-13)
    rel_close(r["post_rate"], l["post_rate"], 1e-12)
    assert np.array_equal(r["rate_class"], l["rate_class"])
    off = case.reference(scale=False)                      # what the unscaled fp64 computation makes of the lost sites
    assert not np.isfinite(off["logL"][lost]).any()
    return lost


@needs_long_double
@pytest.mark.parametrize("S,T", sc.LONG)
def test_reference_is_the_long_double_run_where_fp64_underflows(S, T):
    case = sc.long(S, T)
    _check_against_long_double(case)
    if (S, T) == (20, 600):                                # more than one rescale on the way to some root
        assert (case.reference()["exponent"] < -1074).any()


@needs_long_double
@pytest.mark.parametrize("average,joint", sc.OPTIONS[1:])
def test_variants_are_the_long_double_run_where_fp64_underflows(average, joint):
    case = sc.long(20, 300)
    r = case.reference(average, joint)
    l = case.reference(average, joint, dtype=np.longdouble, scale=False)
    assert np.isfinite(r["counts"]).all()
    clear = l["margin"] > 1e-9
    assert clear.mean() > 0.5
    assert np.allclose(r["counts"][clear], l["counts"][clear], rtol=1e-12, atol=1e-300)
    whole = clear.all(axis=1)
    rel_close(r["norm"][whole], l["norm"][whole], 1e-12)


@needs_long_double
def test_ancestral_states_are_the_long_double_run_where_fp64_underflows():
    case = sc.long(20, 300)
    r, l = case.ancestral(), case.ancestral(dtype=np.longdouble, scale=False)
    assert np.isfinite(r["post"]).all()
    rel_close(r["post"], l["post"], 1e-12, 1e-300)
    clear = l["gap"] > 1e-9
    assert clear.mean() > 0.9 and np.array_equal(r["states"][clear], l["states"][clear])
    rel_close(r["post"].sum(axis=-1), np.ones(r["post"].shape[:2]), 1e-12)


@needs_long_double
def test_star_of_320_leaves_one_product_underflows():
    case = sc.star()
    _check_against_long_double(case, kept=0)             # (every site of such a star is lost without scaling)
