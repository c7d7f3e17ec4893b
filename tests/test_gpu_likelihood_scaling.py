"""Per-site likelihood scaling (cmx_set_likelihood_scaling, the scaled kernels of cmx_variants.hip) on the device, against
tests/scaled_reference.py (pinned on the CPU by tests/test_scaled_reference.py) and, where nothing underflows, against the
oracle and the unscaled call.

Tolerances: the project's plain-kernel bars (tests/test_gpu_codon_alphabets.py, _check_map("c61")) -- counts and norm 1e-9
(atol 1e-300), logL and post_rate 1e-12, rate_class equal -- unless a test says otherwise.  Where a mapping variant chooses
states (nijt.average = no) the counts are compared where the reference's two best candidates are more than 1e-9 apart
(relative), as tests/test_gpu_parity.py does for the unscaled variants."""
from functools import lru_cache

import numpy as np
import pytest

import oracle
from oracle import candidates as ocand
from oracle import cluster as oc
import model_sets as ms
import scaled_cases as sc
import scaled_reference as sr
from comap_amd import engine, protein_models as pm, synthetic
from conftest import make_case, rel_close
from test_gpu_plain_passes import _sites_per_pass

pytestmark = pytest.mark.gpu

KEYS = ("counts", "norm", "logL", "post_rate", "rate_class")


def _engine(case, **kw):
    return engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"], **kw)


def _omodel(case):
    return oracle.Model(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])


def _check_plain(r, o):
    """the plain-kernel bars"""
    rel_close(r["counts"], o["counts"], 1e-9, 1e-300)
    rel_close(r["norm"], o["norm"], 1e-9)
    rel_close(r["logL"], o["logL"], 1e-12)
    rel_close(r["post_rate"], o["post_rate"], 1e-12)
    assert np.array_equal(r["rate_class"], o["rate_class"])


def _check_walk(r, o):
    """test_gpu_parity._check_map"""
    rel_close(r["counts"], o["counts"], 1e-6, 1e-300)
    rel_close(r["logL"], o["logL"], 1e-9)
    rel_close(r["post_rate"], o["post_rate"], 1e-9)
    rel_close(r["norm"], o["norm"], 1e-6)
    assert np.array_equal(r["rate_class"], o["rate_class"])


def _check_null(r, o):
    rel_close(r["stat"], o["stat"], 1e-6, 1e-12)
    rel_close(r["prmin"], o["prmin"], 1e-9)
    rel_close(r["nmin"], o["nmin"], 1e-6)
    assert np.array_equal(r["rcmin"], o["rcmin"])


def _check_option(r, ref, average, joint):
    """a device mapping under (average, joint) against the reference's of the same option"""
    if average and joint:
        return _check_plain(r, ref)
    rel_close(r["logL"], ref["logL"], 1e-12)
    rel_close(r["post_rate"], ref["post_rate"], 1e-12)
    assert np.array_equal(r["rate_class"], ref["rate_class"])
    clear = ref["margin"] > 1e-9
    assert clear.mean() > 0.5
    assert not np.isnan(r["counts"]).any()
    assert np.allclose(r["counts"][clear], ref["counts"][clear], rtol=1e-9, atol=1e-300)
    whole = clear.all(axis=1)
    rel_close(r["norm"][whole], ref["norm"][whole], 1e-9)


@lru_cache(maxsize=None)
def _taxa600():
    """make_case(600, 257, 20, 4321): its first 40 columns are make_case(600, 40, 20, 4321)'s, the alignment of
    test_large_trees_150_and_600_taxa; with the reference's operators"""
    case = make_case(600, 257, 20, 4321)
    case["ops"] = sr.operators(case["parent"], case["blen"], case["Q"], case["pi"], case["rates"])
    return case


def _reference(case, aln, **kw):
    return sr.map_sites(case["parent"], case["blen"], case["lot"], aln, case["Q"], case["pi"], case["rates"], case["probs"],
                        ops=case.get("ops"), **kw)


# ------------------------------------------------------------------------------------------------ the capability
def test_600_taxa_are_finite_with_scaling_and_underflow_without():
    case = _taxa600()
    aln = np.ascontiguousarray(case["aln"][:, :40])
    assert np.array_equal(aln, make_case(600, 40, 20, 4321)["aln"])
    eng, om = _engine(case), _omodel(case)
    eng.set_likelihood_scaling(True)
    r = eng.map_sites(aln)
    for k in KEYS:
        assert np.isfinite(r[k]).all(), k
    _check_plain(r, _reference(case, aln))
    eng.set_likelihood_scaling(False)                       # the same context afterwards: the old pattern is back
    with np.errstate(invalid="ignore"):
        u, o = eng.map_sites(aln), oracle.map_sites(om, aln)
        assert np.isinf(u["logL"]).sum() >= 2 and np.isnan(u["counts"]).any()
        _check_walk(u, o)


# ------------------------------------------------------------------------------------------------ nothing underflows
def _masked_protein_case():
    case = make_case(12, 70, 20, 77)
    masks = oracle.default_masks(20)[:22].copy()
    masks[21] = (1 << 2) | (1 << 3)                         # B = D or N
    case["aln"][3, ::5] = 21
    case["aln"][7, 1::9] = 20                               # and the unknown
    return case, masks


@pytest.mark.parametrize("name", ["protein12_masks", "protein150", "dna14_five_classes", "model_set"])
def test_scaling_changes_nothing_where_nothing_underflows(name):
    masks = None
    if name == "model_set":
        c = ms.case("p20x4")
        eng, om, aln = ms.engine_of(c), ms.oracle_of(c), ms.alignment(c, 70)
    else:
        if name == "protein12_masks":
            case, masks = _masked_protein_case()
        else:
            case = make_case(150, 40, 20, 4322) if name == "protein150" else make_case(14, 70, 4, 31, ncat=5)
        eng, om, aln = _engine(case), _omodel(case), case["aln"]
    o = oracle.map_sites(om, aln, masks)
    assert np.isfinite(o["logL"]).all()
    off = eng.map_sites(aln, masks)
    eng.set_likelihood_scaling(True)
    on = eng.map_sites(aln, masks)
    _check_walk(on, o)
    _check_walk(off, o)
    _check_walk(on, off)
    bare = eng.map_sites(aln, masks, want_counts=False)     # norms from the stage's own counts scratch
    assert bare["counts"] is None
    for k in KEYS[1:]:
        assert np.array_equal(bare[k], on[k]), k
    asr_on = eng.ancestral_states(aln, masks, want_posterior=True)
    eng.set_likelihood_scaling(False)
    asr_off = eng.ancestral_states(aln, masks, want_posterior=True)
    assert np.max(np.abs(asr_on["post"] - asr_off["post"])) <= 1e-12
    assert (asr_on["states"] != asr_off["states"]).mean() < 0.01
    again = eng.map_sites(aln, masks)                       # and the walk is back, bit for bit
    for k in KEYS:
        assert np.array_equal(again[k], off[k]), k


def test_61_states_scaled_equals_unscaled_for_every_option():
    case = make_case(8, 70, 20, 5)
    Q, pi = pm.synthetic_reversible(61, 105)
    rng = np.random.default_rng(5)
    aln = rng.integers(0, 61, size=case["aln"].shape).astype(np.uint8)
    aln = np.where(rng.random(aln.shape) < 0.6, rng.integers(0, 61, size=(1, 70)), aln).astype(np.uint8)
    aln[2, ::7] = 61
    case.update(Q=Q, pi=pi, aln=aln)
    eng = _engine(case)
    for average, joint in sc.OPTIONS:
        eng.set_mapping_options(average, joint)
        eng.set_likelihood_scaling(False)
        off = eng.map_sites(aln)
        eng.set_likelihood_scaling(True)
        on = eng.map_sites(aln)
        rel_close(on["logL"], off["logL"], 1e-12)
        rel_close(on["post_rate"], off["post_rate"], 1e-12)
        assert np.array_equal(on["rate_class"], off["rate_class"])
        if average:
            rel_close(on["counts"], off["counts"], 1e-12, 1e-300)
            rel_close(on["norm"], off["norm"], 1e-12)
        else:                                               # a choice of states: the two best may tie to rounding
            assert np.isclose(on["counts"], off["counts"], rtol=1e-12, atol=1e-300).mean() > 0.995


# ------------------------------------------------------------------------------------------------ fp64 underflows
SHAPES = [("long", 20, 300), ("long", 4, 600), ("long", 20, 600), ("multi",), ("star",)]


@pytest.mark.parametrize("shape", SHAPES, ids=["_".join(map(str, s)) for s in SHAPES])
def test_underflowing_shapes_under_every_mapping_option(shape):
    case = getattr(sc, shape[0])(*shape[1:])
    lost = np.isinf(oracle.map_sites(case.om, case.aln)["logL"])
    assert lost.sum() >= 2                                  # the unscaled computation loses sites here
    eng = case.engine()
    eng.set_likelihood_scaling(True)
    for average, joint in sc.OPTIONS:
        eng.set_mapping_options(average, joint)
        r = eng.map_sites(case.aln)
        for k in KEYS:
            assert np.isfinite(r[k]).all(), (k, average, joint)
        _check_option(r, case.reference(average, joint), average, joint)


def test_mapping_crosses_a_pass_at_600_taxa():
    case = _taxa600()
    nn = len(case["parent"])
    assert _sites_per_pass(4, nn, 20) == 256 < case["aln"].shape[1] == 257
    eng = _engine(case)
    eng.set_likelihood_scaling(True)
    full = eng.map_sites(case["aln"])
    first, second = eng.map_sites(case["aln"][:, :256]), eng.map_sites(case["aln"][:, 256:])
    for k in KEYS:
        assert np.array_equal(full[k], np.concatenate([first[k], second[k]], axis=0)), k
    idx = np.array([0, 1, 100, 254, 255, 256])
    ref = _reference(case, np.ascontiguousarray(case["aln"][:, idx]))
    _check_plain({k: full[k][idx] for k in KEYS}, ref)


def _asr_sites_per_pass(C, nn, device_states, nsites, budget=2 << 30):
    """the ancestral states' rule: 2 GiB of per-node vectors a pass, balanced passes rounded up to whole workgroups"""
    most = max(256, budget // (32 * C * nn * device_states) // 256 * 256)
    passes = -(-nsites // most)
    return min(nsites, (-(-nsites // passes) + 255) // 256 * 256)


def test_ancestral_states_cross_a_pass_at_600_taxa():
    case = _taxa600()
    aln = np.ascontiguousarray(np.tile(case["aln"], (1, 2))[:, :513])
    first = _asr_sites_per_pass(4, len(case["parent"]), 20, aln.shape[1])
    assert first == 512 < aln.shape[1] == 513               # a pass of 512 and a pass of 1
    eng = _engine(case)
    eng.set_likelihood_scaling(True)
    full = eng.ancestral_states(aln, want_posterior=True)
    parts = [eng.ancestral_states(np.ascontiguousarray(a), want_posterior=True) for a in (aln[:, :first], aln[:, first:])]
    for k in ("states", "post"):
        assert np.array_equal(full[k], np.concatenate([p[k] for p in parts], axis=1)), k
    idx = np.array([0, first - 1, first])
    ref = sr.ancestral_states(case["parent"], case["blen"], case["lot"], np.ascontiguousarray(aln[:, idx]), case["Q"], case["pi"],
                              case["rates"], case["probs"], ops=case["ops"])
    assert full["nodes"] == ref["nodes"] and np.isfinite(full["post"]).all()
    assert np.max(np.abs(full["post"][:, idx] - ref["post"])) <= 1e-9
    clear = ref["gap"] > 1e-9
    assert clear.any() and np.array_equal(full["states"][:, idx][clear], ref["states"][clear])


def test_ancestral_states_where_fp64_underflows():
    case = sc.long(20, 300)
    eng = case.engine()
    eng.set_likelihood_scaling(True)
    r, ref = eng.ancestral_states(case.aln, want_posterior=True), case.ancestral()
    assert r["nodes"] == ref["nodes"] and np.isfinite(r["post"]).all()
    assert np.max(np.abs(r["post"] - ref["post"])) <= 1e-9
    clear = ref["gap"] > 1e-9
    assert clear.mean() > 0.9 and np.array_equal(r["states"][clear], ref["states"][clear])
    assert np.array_equal(eng.ancestral_states(case.aln)["states"], r["states"])
    eng.set_likelihood_scaling(False)                       # without it the lost sites have no posterior
    assert np.isnan(eng.ancestral_states(case.aln, want_posterior=True)["post"]).any()


# ------------------------------------------------------------------------------------------------ pipelines
@pytest.mark.parametrize("kind", [oracle.ST_CORRELATION, oracle.ST_COMPENSATION])
def test_null_intra_where_fp64_underflows(kind):
    case = sc.long(20, 300)
    nrep, rep_ram = 2, 33
    sup = np.stack([np.stack([oracle.simulate(case.om, 5, (r * 2 + h) * rep_ram, rep_ram)[0] for h in range(2)]) for r in range(nrep)])
    eng = case.engine()
    eng.set_likelihood_scaling(True)
    g = eng.null_intra(kind, 5, 0, nrep, rep_ram, supplied=sup)
    want = dict(stat=[], rcmin=[], prmin=[], nmin=[])
    lost = 0
    for r in range(nrep):
        a, b = case.map(sup[r, 0]), case.map(sup[r, 1])
        lost += int(np.isinf(oracle.map_sites(case.om, sup[r, 0])["logL"]).sum())
        want["stat"] += [oracle.stat_pair(kind, a["counts"][j], b["counts"][j]) for j in range(rep_ram)]
        want["rcmin"].append(np.minimum(a["rate_class"], b["rate_class"]))
        want["prmin"].append(np.minimum(a["post_rate"], b["post_rate"]))
        want["nmin"].append(np.minimum(a["norm"], b["norm"]))
    assert lost >= 2
    want = dict(stat=np.array(want["stat"]), rcmin=np.concatenate(want["rcmin"]), prmin=np.concatenate(want["prmin"]),
                nmin=np.concatenate(want["nmin"]))
    for k in g:
        assert not np.isnan(g[k]).any(), k
    _check_null(g, want)


def test_pipelines_at_12_taxa_scaled_equal_unscaled():
    case = make_case(12, 60, 20, 9)
    eng, other, om = _engine(case), _engine(make_case(12, 4, 20, 9, alpha=0.9)), _omodel(case)
    mp = oracle.map_sites(om, case["aln"])
    rng = np.random.default_rng(7)
    groups = [list(rng.choice(60, size=int(rng.integers(2, 5)), replace=False)) for _ in range(5)]
    windows = [[(mp["norm"][i] - 0.3, mp["norm"][i] + 0.3) for i in g] for g in groups]
    observed = eng.group_stats(0, mp["counts"], groups)
    cand = dict(min_sim=25, rep_ram=48, max_trials=4, seed=2024)
    # the clustering null as tests/test_gpu_cluster.py sets it up: long branches and distinct simulated columns (equal
    # columns give distances that tie or not depending on rounding, and the tree is then not a function of the data)
    parent, blen, lot = synthetic.random_tree(12, 8)
    mdl = synthetic.protein_model(5.0, 4)
    cl_args = (parent, np.asarray(blen) * 6.0, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    cl = engine.Engine(*cl_args)
    for k in (1, 2):
        sim = oracle.simulate(oracle.Model(*cl_args), 123, k * 50, 50)[0]
        assert np.unique(sim, axis=1).shape[1] == 50, "test precondition: simulated columns must be distinct"

    def run():
        return dict(intra=eng.null_intra(0, 7, 1, 3, 33), comp=eng.null_intra(1, 7, 0, 2, 33),
                    cont=eng.null_intra_continuous(0, 8, 0, 2, 27, 0.7), inter=eng.null_inter(other, 0, 11, 0, 2, 23),
                    cluster=cl.cluster_null(oc.DIST_CORRELATION, oc.LINK_COMPLETE, 123, 1, 3, 50),
                    cand=eng.candidate_groups(0, windows, [1, 1, 0, 1, 1], observed, **cand),
                    mica=eng.mica_parametric_null(5, 2, 37, with_norms=True))
    off = run()
    for e in (eng, other, cl):
        e.set_likelihood_scaling(True)
    on = run()
    for k in ("intra", "comp", "cont", "inter"):
        _check_null(on[k], off[k])
    _check_null(on["intra"], oracle.null_intra(om, 0, 7, 1, 3, 33))
    a, b = on["cluster"], off["cluster"]                    # tests/test_gpu_cluster.py::test_cluster_null_against_oracle
    for k in range(2):
        assert np.array_equal(a["merge"][k], b["merge"][k]) and np.array_equal(a["size"][k], b["size"][k])
        assert np.allclose(a["dmax"][k], b["dmax"][k], rtol=1e-6, atol=1e-12)
        assert np.allclose(a["stat"][k], b["stat"][k], rtol=1e-6, atol=1e-9)
        assert np.allclose(a["nmin"][k], b["nmin"][k], rtol=1e-6, atol=0)
    a, b = on["cand"], off["cand"]                          # tests/test_gpu_candidates.py::test_candidate_groups_against_oracle
    ties = ocand.candidate_groups(om, 0, windows, [1, 1, 0, 1, 1], observed, **cand)["near_ties"]
    assert np.array_equal(a["n2"], b["n2"]) and a["trials"] == b["trials"] and a["batches"] == b["batches"]
    assert np.all(np.abs(a["n1"].astype(np.int64) - b["n1"]) <= ties)
    assert np.array_equal(on["mica"]["mi"], off["mica"]["mi"])
    rel_close(on["mica"]["nmin"], off["mica"]["nmin"], 1e-6)


# ------------------------------------------------------------------------------------------------ the switch, the guard
def test_setter_and_getter():
    case = make_case(6, 20, 4, 3)
    eng = _engine(case)
    assert eng.likelihood_scaling() is False
    eng.set_likelihood_scaling(True)
    assert eng.likelihood_scaling() is True
    eng.map_sites(case["aln"])
    eng.set_mapping_options(False, True)
    eng.null_intra(0, 1, 0, 1, 16)
    eng.pair_stats(0, np.random.default_rng(0).random((5, eng.B, 1)))
    assert eng.likelihood_scaling() is True                 # survives other calls
    eng.set_likelihood_scaling(False)
    assert eng.likelihood_scaling() is False
    import ctypes
    lib, on = engine.load_library(), ctypes.c_int32(7)
    assert lib.cmx_set_likelihood_scaling(None, 1) == -1                # CMX_ERR_INVALID
    assert lib.cmx_get_likelihood_scaling(None, ctypes.byref(on)) == -1 and on.value == 7


def test_scaled_mapping_and_null_under_the_scratch_guard():
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    try:
        case = _taxa600()
        eng = _engine(case)
        eng.set_likelihood_scaling(True)
        r = eng.map_sites(case["aln"])                      # two passes
        assert np.isfinite(r["logL"]).all()
        lng = sc.long(20, 300)
        e2 = lng.engine()
        e2.set_likelihood_scaling(True)
        g = e2.null_intra(0, 5, 0, 3, 33)
        assert not np.isnan(g["stat"]).any()
        e2.ancestral_states(lng.aln, want_posterior=True)
        for e in (eng, e2):
            e.synchronize()
            e.scratch_check()
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
    finally:
        engine.scratch_guard(was)
