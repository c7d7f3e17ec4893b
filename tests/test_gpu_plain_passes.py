"""The plain-kernel stage (cmx_variants.hip) where the suite did not reach it: a mapping that crosses a pass boundary --
the site offsets of counts, logL, post_rate and rate_class in the second pass, and the norms of the whole alignment after
the last pass -- and the norms of a call that asks for no counts (the stage's own counts scratch).

A pass holds 1 GiB of per-node vectors: 4 vectors x 8 bytes x C classes x nn nodes x device states per site, rounded down
to whole workgroups of 256 sites.  A 3-taxon star tree (nn = 4) with four rate classes keeps the smallest alignment that
needs a second pass at 32 769 (61 states, padded to 64), 104 705 (20 states) and 524 289 (4 states) columns of three rows.
Against the oracle on a fixed sample of 300 columns (the first, the last of pass one, the only one of pass two among
them), at the tolerances of test_gpu_codon_alphabets.py (plain path), test_noavg_mapping_matches_oracle and
test_marginal_mappings_match_oracle; and, exactly, against the two calls on the columns of either pass."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, protein_models as pm, synthetic
from conftest import make_case, rel_close

pytestmark = pytest.mark.gpu

PASS_BYTES = 1 << 30


def _sites_per_pass(C, nn, device_states):
    per_site = 32 * C * nn * device_states
    return max(256, PASS_BYTES // per_site // 256 * 256)


def _star_case(S, seed):
    parent, blen, lot = np.array([3, 3, 3, -1], dtype=np.int32), np.array([0.11, 0.23, 0.37, 0.0]), np.arange(3, dtype=np.int32)
    if S in (4, 20):
        mdl = synthetic.protein_model(0.5, 4) if S == 20 else synthetic.dna_model(0.5, 4)
    else:
        Q, pi = pm.synthetic_reversible(S, seed)
        rates, probs = pm.gamma_rates(0.5, 4)
        mdl = dict(Q=Q, pi=pi, rates=rates, probs=probs)
    return dict(parent=parent, blen=blen, lot=lot, **mdl)


def _pair(case):
    args = (case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    return engine.Engine(*args), oracle.Model(*args)


# (states, device states, (average, joint), sites per pass worked out by hand)
CROSSING = [(61, 64, (True, True), 32768), (20, 20, (False, True), 104704), (4, 4, (True, False), 524288)]


@pytest.mark.parametrize("S,SD,options,spp", CROSSING, ids=["plain61_joint", "protein_noavg", "dna_marginal"])
def test_mapping_crosses_a_pass_and_equals_its_two_halves(S, SD, options, spp):
    case = _star_case(S, 700 + S)
    eng, om = _pair(case)
    n = spp + 1
    assert spp == _sites_per_pass(len(case["rates"]), len(case["parent"]), SD)
    assert spp < n <= 2 * spp                                   # two passes: fails if the budget moves
    aln = np.ascontiguousarray(oracle.simulate(om, 900 + S, 0, n)[0])
    assert aln.shape == (3, n)
    eng.set_mapping_options(*options)
    full = eng.map_sites(aln)
    # pass offsets: columns are independent, so the two passes on their own give the same bits -- of what the stage writes:
    # at 4 / 20 states the site scalars are the matrix-core walk's, which takes another path for a single column
    first, second = eng.map_sites(aln[:, :spp]), eng.map_sites(aln[:, spp:])
    for k in ("counts", "norm") + (("logL", "post_rate", "rate_class") if S == 61 else ()):
        assert np.array_equal(full[k], np.concatenate([first[k], second[k]], axis=0)), k
    rest = np.setdiff1d(np.arange(n), [0, spp - 1, spp])
    idx = np.sort(np.concatenate([[0, spp - 1, spp], np.random.default_rng(S).choice(rest, 297, replace=False)]))
    sub = np.ascontiguousarray(aln[:, idx])
    g = {k: v[idx] for k, v in full.items()}
    if options == (True, True):          # plain path: tolerances of test_plain_alphabet_mapping_matches_oracle
        o = oracle.map_sites(om, sub)
        rel_close(g["counts"], o["counts"], 1e-9, 1e-300)
        rel_close(g["norm"], o["norm"], 1e-9)
        rel_close(g["logL"], o["logL"], 1e-12)
        rel_close(g["post_rate"], o["post_rate"], 1e-12)
        assert np.array_equal(g["rate_class"], o["rate_class"])
    elif options == (False, True):       # test_noavg_mapping_matches_oracle
        o = oracle.map_sites_noavg(om, sub)
        clear = o["margin"] > 1e-9
        assert clear.mean() > 0.97
        assert np.allclose(g["counts"][clear], o["counts"][clear], rtol=1e-6, atol=1e-12)
        whole = clear.all(axis=1)
        rel_close(g["norm"][whole], o["norm"][whole], 1e-6, 1e-12)
    else:                                # test_marginal_mappings_match_oracle, average = yes
        o = oracle.map_sites_marginal(om, sub, True)
        rel_close(g["counts"], o["counts"], 1e-6, 1e-14)
        rel_close(g["norm"], o["norm"], 1e-6, 1e-14)


def _six_taxa(S):
    case = make_case(6, 70, 20 if S == 61 else S, 500 + S)
    if S == 61:
        Q, pi = pm.synthetic_reversible(S, 561)
        rng = np.random.default_rng(61)
        aln = rng.integers(0, S, size=case["aln"].shape).astype(np.uint8)
        aln = np.where(rng.random(aln.shape) < 0.6, rng.integers(0, S, size=(1, 70)), aln).astype(np.uint8)     # columns with signal
        case.update(Q=Q, pi=pi, aln=aln)
    case["aln"][2, ::7] = S                                     # unknowns at a leaf
    return case


NORM_ONLY = [(S, opt) for S in (20, 4) for opt in ((False, True), (True, False), (False, False))] + [(61, (True, True))]


@pytest.mark.parametrize("S,options", NORM_ONLY, ids=[f"S{S}_avg{int(a)}_joint{int(j)}" for S, (a, j) in NORM_ONLY])
def test_norms_without_counts_equal_the_norms_with_counts(S, options):
    case = _six_taxa(S)
    eng, om = _pair(case)
    eng.set_mapping_options(*options)
    bare, withc = eng.map_sites(case["aln"], want_counts=False), eng.map_sites(case["aln"])
    assert bare["counts"] is None and withc["counts"] is not None
    assert np.array_equal(bare["norm"], withc["norm"])
    for k in ("logL", "post_rate", "rate_class"):
        assert np.array_equal(bare[k], withc[k]), k
    # and they are the oracle's, where its choice of states is clear (tolerances of the tests named in the module docstring)
    average, joint = options
    if joint and average:
        rel_close(bare["norm"], oracle.map_sites(om, case["aln"])["norm"], 1e-9)
    elif joint:
        o = oracle.map_sites_noavg(om, case["aln"])
        whole = (o["margin"] > 1e-9).all(axis=1)
        assert whole.mean() > 0.8
        rel_close(bare["norm"][whole], o["norm"][whole], 1e-6, 1e-12)
    elif average:
        rel_close(bare["norm"], oracle.map_sites_marginal(om, case["aln"], True)["norm"], 1e-6, 1e-14)
    else:
        o = oracle.map_sites_marginal(om, case["aln"], False)
        parent = np.asarray(case["parent"])
        whole = ((o["margin"][:, :-1] > 1e-9) & (o["margin"][:, parent[:-1]] > 1e-9)).all(axis=1)     # every node and father clear
        assert whole.mean() > 0.8                               # (the ten columns with the unknown leaf are ties by construction)
        rel_close(bare["norm"][whole], o["norm"][whole], 1e-6, 1e-12)
