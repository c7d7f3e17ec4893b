"""-m gpu: every path of the device that a non-homogeneous model set reaches (one generator per branch, root frequencies,
the tree kept rooted) against the model-set oracle (oracle.ModelSet; proved on the CPU in tests/test_oracle_model_sets.py).
Cases and simulator inputs come from tests/model_sets.py.

Tolerances are the suite's for the same quantities: counts and statistics rel_close(1e-6, 1e-12); logL and post_rate 1e-6;
prmin 1e-9; nmin 1e-6; continuous rates 1e-12; rate classes exact where the oracle's margin between the two most
probable classes exceeds 1e-9 (a column of unknowns only ties them exactly), everywhere in the nulls; argmax / anc
entries compared where the oracle's margin exceeds 1e-9; simulated symbols byte-identical on every site that is not fragile (no draw within 1e-9 of a boundary of
its cumulative row in the restatement), the fragile sites counted against the cap of 1e-3.

Every comparison prints its largest relative deviation, every simulator comparison the number of fragile sites it left
out (pytest -s shows them)."""
from functools import lru_cache

import numpy as np
import pytest
import scipy.linalg

import model_sets as ms
import oracle
from oracle import candidates as ocand, cluster as oc
from comap_amd import engine
from conftest import rel_close

pytestmark = pytest.mark.gpu

FRAGILE_CAP = 1e-3


@lru_cache(maxsize=None)
def _eng(name, variant=0):
    """one engine per case for the whole module; a test that changes an option of it puts the default back"""
    return ms.engine_of(ms.case(name, variant))


@lru_cache(maxsize=None)
def _om(name, variant=0):
    return ms.oracle_of(ms.case(name, variant))


def _close(label, got, want, rtol, atol=0.0):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = ~np.isnan(want) & (np.abs(want) > atol)
    dev = np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])) if ok.any() else 0.0
    print(f"{label}: largest relative deviation {dev:.3g}")
    rel_close(got, want, rtol, atol)


def _same_symbols(label, got, want, near):
    """byte-identical off the fragile sites; got / want [..., n] with the sites last, near [n]"""
    frag = ms.fragile(near)
    print(f"{label}: {int(frag.sum())} fragile of {frag.size} sites left out")
    assert frag.mean() <= FRAGILE_CAP
    assert np.array_equal(got[..., ~frag], want[..., ~frag])


def _class_margin(om, aln, masks=None):
    """(best - second) / best of the classes' posterior probabilities, from the oracle: a column of unknowns only has the
    prior of every class, an exact tie that rounding decides"""
    post = np.sort(oracle.map_sites_marginal(om, aln, True, masks, want_post=True)["post"][:, -1].sum(-1), axis=1)
    return (post[:, -1] - post[:, -2]) / post[:, -1]


def _check_map(label, r, o, class_margin):
    _close(label + " counts", r["counts"], o["counts"], 1e-6, 1e-12)
    _close(label + " norm", r["norm"], o["norm"], 1e-6, 1e-12)
    _close(label + " logL", r["logL"], o["logL"], 1e-6)
    _close(label + " post_rate", r["post_rate"], o["post_rate"], 1e-6)
    clear = class_margin > 1e-9
    assert clear.mean() > 0.9 and np.array_equal(r["rate_class"][clear], o["rate_class"][clear])


def _check_null(label, g, o):
    _close(label + " stat", g["stat"], o["stat"], 1e-6, 1e-12)
    _close(label + " prmin", g["prmin"], o["prmin"], 1e-9)
    _close(label + " nmin", g["nmin"], o["nmin"], 1e-6)
    assert np.array_equal(g["rcmin"], o["rcmin"])


def _no_fragile(c, seed, g0, n):
    """the nulls compare statistics, not symbols: their simulated ranges must hold no fragile site at all"""
    assert not ms.fragile(oracle.simulate(ms.oracle_of(c), seed, g0, n, want_near=True)[2]).any()


# ---------------------------------------------------------------------------------------------- 1. transition matrices
@pytest.mark.parametrize("name", ms.MAPPING_CASES)
def test_transition_matrices_of_every_class_and_branch(name):
    c = ms.case(name)
    P = _eng(name).transition_matrices()
    ref = np.array([[scipy.linalg.expm(c["Qs"][c["mob"][b]] * (c["blen"][b] * r)) for b in range(len(c["parent"]) - 1)]
                    for r in c["rates"]])
    _close(f"P {name}", P, ref, 1e-9, 1e-13)


# ---------------------------------------------------------------------------------------------- 2. averaged mapping
@pytest.mark.parametrize("ambiguous", [False, True], ids=["states", "ambiguity"])
@pytest.mark.parametrize("name", ms.MAPPING_CASES)
def test_averaged_mapping(name, ambiguous):
    """70 sites: a ragged second tile of 64"""
    c = ms.case(name)
    aln = ms.alignment(c, 70, ambiguous)
    masks = ms.IUPAC if ambiguous and c["S"] == 4 else None
    _check_map(f"map {name}", _eng(name).map_sites(aln, masks=masks), oracle.map_sites(_om(name), aln, masks),
               _class_margin(_om(name), aln, masks))


@pytest.mark.parametrize("name", ["p20x4", "n4x4", "c61x2"])
def test_averaged_mapping_two_types(name):
    c = ms.case(name)
    aln = ms.alignment(c, 70)
    Bks = ms.registers(c, 2)
    r = ms.engine_of(c, Bk=Bks).map_sites(aln)
    _check_map(f"map K=2 {name}", r, oracle.map_sites(ms.oracle_of(c, Bks=Bks), aln), _class_margin(_om(name), aln))
    _close(f"linearity over types {name}", r["counts"].sum(-1), _eng(name).map_sites(aln)["counts"][:, :, 0], 1e-9)


# ---------------------------------------------------------------------------------------------- 3. variant mappings
@pytest.mark.parametrize("name", ["p20x4", "n4x4", "c61x2"])
def test_variant_mappings(name):
    c = ms.case(name)
    aln = ms.alignment(c, 70)
    aln[2, ::7] = c["S"]                                    # some unknowns at a leaf
    eng, om = _eng(name), _om(name)
    parent = c["parent"]
    try:
        eng.set_mapping_options(average=False, joint=True)
        g, o = eng.map_sites(aln), oracle.map_sites_noavg(om, aln)
        clear = o["margin"] > 1e-9
        assert clear.mean() > 0.97
        _close(f"noavg {name}", g["counts"][clear], o["counts"][clear], 1e-6, 1e-12)
        full = clear.all(axis=1)
        _close(f"noavg norm {name}", g["norm"][full], o["norm"][full], 1e-6, 1e-12)
        eng.set_mapping_options(average=True, joint=False)
        g, o = eng.map_sites(aln), oracle.map_sites_marginal(om, aln, True)
        _close(f"marginal {name}", g["counts"], o["counts"], 1e-6, 1e-12)
        _close(f"marginal norm {name}", g["norm"], o["norm"], 1e-6, 1e-12)
        eng.set_mapping_options(average=False, joint=False)
        g, o = eng.map_sites(aln), oracle.map_sites_marginal(om, aln, False)
        clear = (o["margin"][:, :-1] > 1e-9) & (o["margin"][:, parent[:-1]] > 1e-9)     # node and father both clear
        assert clear.mean() > 0.97
        _close(f"marginal noavg {name}", g["counts"][clear], o["counts"][clear], 1e-6, 1e-12)
    finally:
        eng.set_mapping_options(True, True)
    # nijt = Label: the label of the most probable substitution of every branch
    W = engine.label_substitution_weights(c["S"])
    lab = ms.engine_of(c, count_method=engine.COUNT_NAIVE, naive_weights=W)
    lab.set_mapping_options(average=False, joint=True)
    g = lab.map_sites(aln)
    o = oracle.map_sites_noavg(ms.oracle_of(c, method=oracle.METHOD_NAIVE, naive_W=W), aln)
    clear = o["margin"] > 1e-9
    assert np.array_equal(g["counts"][clear], o["counts"][clear])
    assert np.array_equal(g["counts"][clear][:, 0], W[o["argmax"][clear] // c["S"], o["argmax"][clear] % c["S"]])


# ---------------------------------------------------------------------------------------------- 4. discrete simulator
@pytest.mark.parametrize("name", ms.SIMULATOR_CASES)
def test_discrete_simulator(name):
    import torch
    c, eng, om = ms.case(name), _eng(name), _om(name)
    a, cl = eng.simulate(ms.SIM_SEED, ms.SIM_G0, ms.SIM_N)
    ao, co, near = oracle.simulate(om, ms.SIM_SEED, ms.SIM_G0, ms.SIM_N, want_near=True)
    _same_symbols(f"simulate {name}", np.concatenate([a, cl[None].astype(np.uint8)]), np.concatenate([ao, co[None].astype(np.uint8)]),
                  near)
    a2, c2 = eng.simulate(ms.SIM_SEED, ms.SIM_G0 + 1000, 10)
    assert np.array_equal(a2, a[:, 1000:1010]) and np.array_equal(c2, cl[1000:1010])     # counter-based: any sub-range
    # the null's simulator (gather kernel, blocked layout [replicate][batch][taxon][rep_ram]) against the restatement
    k = ms.GATHER
    T, nrep, ram = len(c["lot"]), k["rep_end"] - k["rep_begin"], k["rep_ram"]
    n = nrep * 2 * ram
    buf = torch.empty(n * T, dtype=torch.uint8, device="cuda:0")
    eng.null_simulate_dev(k["seed"], k["rep_begin"], k["rep_end"], ram, buf)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nrep, 2, T, ram).transpose(2, 0, 1, 3).reshape(T, n)
    plain, _ = eng.simulate(k["seed"], k["rep_begin"] * 2 * ram, n)
    assert np.array_equal(got, plain)
    wo, _, near = oracle.simulate(om, k["seed"], k["rep_begin"] * 2 * ram, n, want_near=True)
    _same_symbols(f"null simulator {name}", got, wo, near)


@pytest.mark.parametrize("name,k", ms.CHAIN, ids=[n for n, _ in ms.CHAIN])
def test_lds_table_simulator(name, k):
    """75 000 sites with everything even is the threshold of the LDS-table kernel; six classes are the largest node block of its two-piece shape"""
    import torch
    c, eng = ms.case(name), _eng(name)
    T, nrep, ram = len(c["lot"]), k["rep_end"] - k["rep_begin"], k["rep_ram"]
    n = nrep * 2 * ram
    assert n >= 75_000 and n % 2 == 0 and (k["rep_begin"] * 2 * ram) % 2 == 0
    buf = torch.empty(n * T, dtype=torch.uint8, device="cuda:0")
    eng.null_simulate_dev(k["seed"], k["rep_begin"], k["rep_end"], ram, buf)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nrep, 2, T, ram).transpose(2, 0, 1, 3).reshape(T, n)
    plain, _ = eng.simulate(k["seed"], k["rep_begin"] * 2 * ram, n)
    assert np.array_equal(got, plain)
    wo, _, near = oracle.simulate(_om(name), k["seed"], k["rep_begin"] * 2 * ram, n, want_near=True)
    _same_symbols(f"LDS simulator {name}", got, wo, near)


# ---------------------------------------------------------------------------------------------- 5. continuous simulator
@pytest.mark.parametrize("name", ms.CONTINUOUS_CASES)
def test_continuous_simulator_and_its_null(name):
    c, eng, om = ms.case(name), _eng(name), _om(name)
    k = ms.CONTINUOUS
    for alpha, pinv in k["rates"]:
        a, r = eng.simulate_continuous(k["seed"], k["g0"], k["n"], alpha, pinv)
        ao, ro, near = oracle.simulate_continuous(om, k["seed"], k["g0"], k["n"], alpha, pinv, want_near=True)
        _close(f"continuous rates {name} {alpha}", r, ro, 1e-12, 1e-300)
        _same_symbols(f"continuous {name} {alpha}", a, ao, near)
    k = ms.CONTINUOUS_NULL
    T, nrep, ram = len(c["lot"]), k["rep_end"] - k["rep_begin"], k["rep_ram"]
    g = eng.null_intra_continuous(0, k["seed"], k["rep_begin"], k["rep_end"], ram, k["alpha"], k["p_inv"])
    aln, _, near = oracle.simulate_continuous(om, k["seed"], k["rep_begin"] * 2 * ram, nrep * 2 * ram, k["alpha"], k["p_inv"],
                                              want_near=True)
    assert not ms.fragile(near).any()
    sup = np.ascontiguousarray(aln.reshape(T, nrep, 2, ram).transpose(1, 2, 0, 3))
    _check_null(f"continuous null {name}", g, oracle.null_intra(om, 0, k["seed"], k["rep_begin"], k["rep_end"], ram, supplied=sup))


# ---------------------------------------------------------------------------------------------- 6. null of one data set
@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COMPENSATION], ids=["correlation", "compensation"])
@pytest.mark.parametrize("name", ms.NULL_CASES)
def test_null_of_one_data_set(name, kind):
    """rep_ram = 50: blocks of 64 straddle replicates.  The fused null with the pattern table on and off, and the unfused
    simulate -> map -> score sequence (the two-data-set null with both sides equal), all against the oracle"""
    c, eng, om = ms.case(name), _eng(name), _om(name)
    seed, nrep, ram = ms.NULL["seed"], ms.NULL["nrep"], ms.NULL["rep_ram"]
    _no_fragile(c, seed, 0, nrep * 2 * ram)
    o = oracle.null_intra(om, kind, seed, 0, nrep, ram)
    try:
        eng.set_null_patterns(True)
        on = eng.null_intra(kind, seed, 0, nrep, ram)
        eng.set_null_patterns(False)
        off = eng.null_intra(kind, seed, 0, nrep, ram)
    finally:
        eng.set_null_patterns(None)
    _check_null(f"null patterns on {name} {kind}", on, o)
    _check_null(f"null patterns off {name} {kind}", off, o)
    for key in on:
        assert np.array_equal(on[key], off[key], equal_nan=True), key
    _check_null(f"null unfused {name} {kind}", eng.null_inter(eng, kind, seed, 0, nrep, ram), o)
    tail = eng.null_intra(kind, seed, 1, nrep, ram)           # sharding: replicates [1, 3) alone
    default = eng.null_intra(kind, seed, 0, nrep, ram)
    for key in tail:
        assert np.array_equal(tail[key], default[key][ram:], equal_nan=True), key
    _no_fragile(c, 5, 0, nrep * 2 * ram)
    sup = np.stack([np.stack([oracle.simulate(om, 5, (r * 2 + h) * ram, ram)[0] for h in range(2)]) for r in range(nrep)])
    _check_null(f"null supplied {name} {kind}", eng.null_intra(kind, 0, 0, nrep, ram, supplied=sup),
                oracle.null_intra(om, kind, 0, 0, nrep, ram, supplied=sup))


# ---------------------------------------------------------------------------------------------- 7. null of two data sets
@pytest.mark.parametrize("name", ms.NULL_CASES)
def test_null_of_two_data_sets_with_different_sets(name):
    k = ms.NULL_INTER
    for v in (0, 1):
        _no_fragile(ms.case(name, v), k["seed"], k["rep_begin"] * 2 * k["rep_ram"], (k["rep_end"] - k["rep_begin"]) * 2 * k["rep_ram"])
    for kind in (engine.STAT_CORRELATION, engine.STAT_COMPENSATION):
        g = _eng(name).null_inter(_eng(name, 1), kind, k["seed"], k["rep_begin"], k["rep_end"], k["rep_ram"])
        o = oracle.null_inter(_om(name), _om(name, 1), kind, k["seed"], k["rep_begin"], k["rep_end"], k["rep_ram"])
        _check_null(f"null inter {name} {kind}", g, o)


# ---------------------------------------------------------------------------------------------- 8. composed analyses
def test_cluster_null_under_a_set():
    c, k = ms.long_case(), ms.CLUSTER
    eng, om = ms.engine_of(c), ms.oracle_of(c)
    n, r0, r1 = k["nsites"], k["rep_begin"], k["rep_end"]
    _no_fragile(c, k["seed"], r0 * n, (r1 - r0) * n)
    for r in range(r0, r1):
        a = oracle.simulate(om, k["seed"], r * n, n)[0]
        assert np.unique(a, axis=1).shape[1] == n, "test precondition: simulated columns must be distinct"
    g = eng.cluster_null(oc.DIST_CORRELATION, oc.LINK_COMPLETE, k["seed"], r0, r1, n)
    o = oc.cluster_null(om, oc.DIST_CORRELATION, oc.LINK_COMPLETE, k["seed"], r0, r1, n)
    for r in range(r1 - r0):
        assert np.array_equal(g["merge"][r], o[r]["merge"]) and np.array_equal(g["size"][r], o[r]["size"])
        assert np.allclose(g["dmax"][r], o[r]["dmax"], rtol=1e-6, atol=1e-12)
        assert np.allclose(g["stat"][r], o[r]["stat"], rtol=1e-6, atol=1e-9)
        assert np.allclose(g["nmin"][r], o[r]["nmin"], rtol=1e-6, atol=0)


def test_candidate_groups_under_a_set():
    c, eng, om = ms.case("p20x4"), _eng("p20x4"), _om("p20x4")
    k = ms.CANDIDATES
    aln = oracle.simulate(om, 11, 10 ** 6, 60)[0]
    mp = oracle.map_sites(om, aln)
    groups = [[3, 17], [5, 8, 40]]
    windows = [[(mp["norm"][i] - 0.3, mp["norm"][i] + 0.3) for i in g] for g in groups]
    observed = eng.group_stats(engine.STAT_CORRELATION, mp["counts"], groups)
    args = dict(min_sim=25, rep_ram=k["rep_ram"], max_trials=4, seed=k["seed"])
    g = eng.candidate_groups(engine.STAT_CORRELATION, windows, [1, 1], observed, **args)
    o = ocand.candidate_groups(om, oracle.ST_CORRELATION, windows, [1, 1], observed, **args)
    assert o["batches"] <= 16                               # the range whose fragile share and power the CPU tests bound
    _no_fragile(c, k["seed"], 0, int(o["batches"]) * k["rep_ram"])
    assert np.array_equal(g["n2"], o["n2"]) and g["trials"] == o["trials"] and g["batches"] == o["batches"]
    assert np.all(np.abs(g["n1"].astype(np.int64) - o["n1"]) <= o["near_ties"])
    assert np.all(g["n2"] <= 25) and g["batches"] >= 1
    assert np.allclose(g["pvalue"], (o["n1"] + 1.0) / (o["n2"] + 1.0))


def test_mica_parametric_null_under_a_set():
    c, eng, om = ms.case("p20x4"), _eng("p20x4"), _om("p20x4")
    k = ms.MICA
    nrep, ram = k["nrep"], k["rep_ram"]
    _no_fragile(c, k["seed"], 0, nrep * 2 * ram)
    pn = eng.mica_parametric_null(k["seed"], nrep, ram)
    for rep in range(nrep):
        a1 = oracle.simulate(om, k["seed"], (rep * 2) * ram, ram)[0]
        a2 = oracle.simulate(om, k["seed"], (rep * 2 + 1) * ram, ram)[0]
        o = oracle.mi_columns(a1, a2, c["S"])
        _close(f"mica MI replicate {rep}", pn["mi"][rep * ram:(rep + 1) * ram], np.diag(o["mi"]), 1e-6, 1e-12)
        _close(f"mica joint entropy replicate {rep}", pn["hjoint"][rep * ram:(rep + 1) * ram], np.diag(o["hjoint"]), 1e-6, 1e-12)
