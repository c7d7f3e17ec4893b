"""The device paths at the edges of branch length and rate, against tests/golden/operator_edges.npz (50-digit known answers;
cases in tests/operator_edge_cases.py, the CPU restatements against the same fixture in tests/test_operator_edges.py): zero,
1e-100, 1e-12 and saturated branches (150 and Bio++'s bound of 10000), a rate-zero class, degenerate spectra, K = 2 and a
signed register, through every consumer of the host-built operators.

Bars: the suite's device bars -- counts 1e-9 relative, logL and post_rate 1e-12, rate class exact -- widened only to the
bound of the case's row in test_operator_edges' MEASURED-CASES table where that is larger (the fp64 closed form itself), and
with that module's absolute term of the counts (operator_rounding x t_b r_top: a count between equal states on a 1e-12 branch is O(t^2),
below the rounding of the operator it is read from).  The rate class is compared where the fixture's two best classes are
more than 1e-9 apart.  Every comparison is against the fixture or, for the simulator and the null, against the oracle;
scaled_reference.map_sites (pinned by test_operator_edges) serves the one case that needs a rescale.
No case holds impossible data: every stored logL is finite."""
import os

import numpy as np
import pytest

import oracle
import ancestral_reference as ar
import operator_edge_cases as oe
import scaled_reference as sr
import test_operator_edges as cpu
from comap_amd import engine
from conftest import ROOT, rel_close
from test_gpu_likelihood_scaling import _check_null

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(ROOT, "tests", "golden", "operator_edges.npz"))


@pytest.fixture(scope="module")
def bounds():
    return cpu._table("MEASURED-CASES")


def _engine(c):
    return engine.Engine(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"], Bk=oe.register_of(c),
                         clamp_negative=bool(c["clamp"]))


def _check(r, c, row):
    """a device mapping against the fixture's case c; row: the case's measured figures (counts unif, decomp, logL, post_rate)"""
    counts_bar = max(1e-9, cpu.bound(row[1]))               # the engine evaluates the decomposition form
    zero = c["blen"][:-1] == 0.0
    assert not np.isnan(r["counts"]).any()
    assert (r["counts"][:, zero] == 0.0).all()
    if c["clamp"]:
        assert (r["counts"] >= 0.0).all()
    need = cpu.needed_rtol(r["counts"], c)
    assert need <= counts_bar, f"counts need rtol {need:.3e} (bar {counts_bar:.1e})"
    rel_close(r["logL"], c["logL"], max(1e-12, cpu.bound(row[2])))
    rel_close(r["post_rate"], c["post_rate"], max(1e-12, cpu.bound(row[3])))
    clear = c["class_clear"]
    assert np.array_equal(r["rate_class"][clear], c["rate_class"][clear])
    # the norm of the per-branch sums over the K types: each sum carries K absolute terms
    rel_close(r["norm"], np.sqrt((c["counts"].sum(axis=2) ** 2).sum(axis=1)), counts_bar,
              c["counts"].shape[2] * np.linalg.norm(cpu.count_atol(c)))


class _Switch:
    def __init__(self, setter, on):
        self.setter, self.on = setter, on

    def __enter__(self):
        self.was = self.setter(self.on)

    def __exit__(self, *exc):
        self.setter(self.was)


# ------------------------------------------------------------------------------------------------ the default mapping
@pytest.mark.parametrize("name", oe.CASES)
def test_default_mapping_meets_the_fixture(fix, bounds, name):
    """S = 20: the 64-site walk; S = 4: 16 fused states (Gamma(4)), 20 fused states (Invariant + Gamma(4)), unfused (C = 1);
    S = 7: the plain kernels; S = 61: the wide matrix-core kernels"""
    c = oe.load(fix, name)
    _check(_engine(c).map_sites(c["aln"]), c, bounds[name])


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("name", [n for n in oe.CASES if n.startswith("protein")])
def test_protein_class_split_launch(fix, bounds, name, small):
    c = oe.load(fix, name)
    with _Switch(engine.map_small_blocks, small):
        _check(_engine(c).map_sites(c["aln"]), c, bounds[name])


@pytest.mark.parametrize("name", [n for n in oe.CASES if n.startswith("s61")])
def test_61_states_on_the_plain_kernels(fix, bounds, name):
    c = oe.load(fix, name)
    with _Switch(engine.map_wide_plain, True):
        _check(_engine(c).map_sites(c["aln"]), c, bounds[name])


# ------------------------------------------------------------------------------------------------ likelihood scaling
@pytest.mark.parametrize("name", [n for n in oe.CASES if "-ig5-" in n or n.endswith("p6")])
def test_scaled_mapping_meets_the_fixture(fix, bounds, name):
    """with a rate-zero class a variable site has likelihood 0 (to rounding, of either sign) under class 0: the site
    exponent must come from the classes with a positive share"""
    c = oe.load(fix, name)
    eng = _engine(c)
    eng.set_likelihood_scaling(True)
    r = eng.map_sites(c["aln"])
    assert np.isfinite(r["logL"]).all()
    _check(r, c, bounds[name])


def test_scaled_star_with_a_rate_zero_class_rescales():
    """operator_edge_cases.STAR_LEAVES = 62 leaves: the fewest at which a site is rescaled (found and held on the CPU by
    test_operator_edges.test_star_is_the_smallest_that_rescales); the reference is scaled_reference.map_sites"""
    base, rates, probs, aln = oe.star_case()
    ref = sr.map_sites(base.parent, base.blen, base.lot, aln, base.Q, base.pi, rates, probs)
    assert (ref["exponent"] != 0).any() and np.isfinite(ref["logL"]).all()
    eng = engine.Engine(base.parent, base.blen, base.lot, base.Q, base.pi, rates, probs)
    eng.set_likelihood_scaling(True)
    r = eng.map_sites(aln)
    rel_close(r["counts"], ref["counts"], 1e-9, 1e-300)
    rel_close(r["logL"], ref["logL"], 1e-12)
    rel_close(r["post_rate"], ref["post_rate"], 1e-12)
    assert np.array_equal(r["rate_class"], ref["rate_class"])


# ------------------------------------------------------------------------------------------------ the three other options
@pytest.mark.parametrize("name", cpu.VARIANT_CASES)
def test_variant_mappings_meet_the_fixture(fix, bounds, name):
    """nijt.average / nijt.joint through N1 and NC: conditional counts without time (zero-length branches, the rate-zero
    class: exact zeros) and on saturated branches.  Counts are compared on the branches whose choice of states is clear in
    the fixture (cpu.variant_figure); logL, posterior rate and rate class as in the default mapping."""
    c = oe.load(fix, name)
    eng, row = _engine(c), bounds[name]
    for key, (average, joint) in cpu.VARIANTS.items():
        eng.set_mapping_options(average, joint)
        r = eng.map_sites(c["aln"])
        assert not np.isnan(r["counts"]).any(), key
        assert (r["counts"][:, c["blen"][:-1] == 0.0] == 0.0).all(), key
        fig = cpu.variant_figure(r["counts"], c, key)
        assert fig <= max(1e-9, cpu.VARIANT_BOUND), f"{key}: counts need rtol {fig:.3e}"
        rel_close(r["logL"], c["logL"], max(1e-12, cpu.bound(row[2])))
        rel_close(r["post_rate"], c["post_rate"], max(1e-12, cpu.bound(row[3])))
        assert np.array_equal(r["rate_class"][c["class_clear"]], c["rate_class"][c["class_clear"]])


# ------------------------------------------------------------------------------------------------ ancestral states
@pytest.mark.parametrize("name", [n for n in oe.CASES if n[-1] in "136" and (n.split("-")[0] in ("dna", "s7")
                                                                             or n in oe.ANCESTRAL_CASES)])
def test_marginal_ancestral_states(fix, monkeypatch, name):
    """tests/ancestral_reference.py fed the fixture's P (4, 7 and 20 states); the bars of tests/test_gpu_ancestral.py"""
    c = oe.load(fix, name)
    P = oe.ancestral_P(fix, c)
    P = np.concatenate([P, np.zeros_like(P[:, :1])], axis=1)                    # [C, nn, S, S], the root's entry unused
    monkeypatch.setattr(ar, "transition_matrices", lambda *a, **k: P)
    ref = ar.ancestral_states(c["parent"], c["blen"], c["lot"], c["Q"], c["rates"], c["probs"], c["pi"], c["aln"])
    r = _engine(c).ancestral_states(c["aln"], want_posterior=True)
    assert r["nodes"] == ref["nodes"] and np.isfinite(r["post"]).all()
    assert np.max(np.abs(r["post"] - ref["post"])) <= 1e-9
    s = np.sort(ref["post"], axis=-1)
    clear = s[..., -1] - s[..., -2] > 1e-9
    assert clear.mean() > 0.5 and np.array_equal(r["states"][clear], ref["states"][clear])


# ------------------------------------------------------------------------------------------------ the simulator
def _sim_engine(gen, rates, probs, blen=None, tree="t5"):
    parent, base, lot = oe.TREES[tree]
    Q, pi, _, _ = oe.generator(gen)
    return engine.Engine(parent, base if blen is None else blen, lot, Q, pi, rates, probs)


@pytest.mark.parametrize("gen", ["dna", "protein", "s7"])
def test_simulated_taxa_are_equal_without_time(gen):
    zero = np.zeros(len(oe.TREES["t5"][0]))
    aln, _ = _sim_engine(gen, *oe.rate_set("g4"), blen=zero).simulate(11, 0, 4096)
    assert (aln == aln[:1]).all()
    aln, _ = _sim_engine(gen, np.array([0.0]), np.array([1.0])).simulate(12, 0, 4096)
    assert (aln == aln[:1]).all()
    aln, cls = _sim_engine(gen, *oe.rate_set("ig5")).simulate(13, 0, 4096)
    assert 600 < (cls == 0).sum() < 1050                    # 0.2 x 4096 = 819, sd 26
    assert (aln[:, cls == 0] == aln[:1, cls == 0]).all()
    assert not (aln[:, cls != 0] == aln[:1, cls != 0]).all()


@pytest.mark.parametrize("name", ["dna-g4-t4-p6", "dna-ig5-t5-p7", "protein-g4-t5-p6", "protein-g4-t5-p7", "s7-g4-t5-p7"])
def test_simulator_equals_the_oracle_on_saturated_branches(fix, name):
    """4096 sites: the guide-table search over cumulative rows that all equal the running sums of pi"""
    c = oe.load(fix, name)
    om = oracle.Model(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"])
    want, want_cls = oracle.simulate(om, 21, 0, 4096)
    aln, cls = _engine(c).simulate(21, 0, 4096)
    assert np.array_equal(cls, want_cls)
    assert aln.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ a null
@pytest.mark.parametrize("name", ["protein-g4-t5-p6", "dna-g4-t4-p6"])
def test_null_intra_on_saturated_branches(fix, name):
    c = oe.load(fix, name)
    om = oracle.Model(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"])
    g = _engine(c).null_intra(oracle.ST_CORRELATION, 5, 0, 3, 40)
    assert not np.isnan(g["stat"]).any()
    _check_null(g, oracle.null_intra(om, oracle.ST_CORRELATION, 5, 0, 3, 40))
