"""-m gpu: the HIP path behind the C-ABI against the oracle on the same seeded inputs.

Tolerances: substitution vectors, likelihoods, norms, statistics 1e-6 relative (north_star); rate classes, norm
classes, Nsim, simulated states bit-exact.  Statistics that are differences of nearly equal numbers (correlation
near 0, compensation near 0) additionally get an absolute floor of 1e-12, stated where used.  The all-kinds and the
fixture-vector pair statistics are held to the derived bounds of tests/pair_stat_cases.py instead."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, protein_models as pm, synthetic
import pair_stat_cases as pc
from conftest import make_case, rel_close

pytestmark = pytest.mark.gpu


def _engine(case, **kw):
    return engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"],
                         **kw)


def _omodel(case, **kw):
    return oracle.Model(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"],
                        **kw)


def _check_map(r, o):
    rel_close(r["counts"], o["counts"], 1e-6, 1e-300)
    rel_close(r["logL"], o["logL"], 1e-9)
    rel_close(r["post_rate"], o["post_rate"], 1e-9)
    rel_close(r["norm"], o["norm"], 1e-6)
    assert np.array_equal(r["rate_class"], o["rate_class"])


def test_transition_matrices_match_oracle_eigensystem():
    case = make_case(8, 4, 20, 11)
    eng = _engine(case)
    P = eng.transition_matrices()
    assert np.allclose(P.sum(-1), 1.0, atol=1e-12)
    import scipy.linalg
    for c in (0, 3):
        for b in (0, 5):
            ref = scipy.linalg.expm(case["Q"] * case["blen"][b] * case["rates"][c])
            assert np.max(np.abs(P[c, b] - ref)) < 1e-12


@pytest.mark.parametrize("nsites", [1, 63, 64, 65, 200])
def test_map_sites_protein_ragged_sizes(nsites):
    case = make_case(12, nsites, 20, 100 + nsites)
    r = _engine(case).map_sites(case["aln"])
    _check_map(r, oracle.map_sites(_omodel(case), case["aln"]))


@pytest.mark.parametrize("ntaxa,nstates", [(3, 20), (4, 20), (5, 20), (3, 4), (4, 4), (6, 4)])
def test_tiny_trees_map_and_null(ntaxa, nstates):
    """smallest trees (a star of three leaves upward): op streams of a handful of entries, no stored vectors at all"""
    case = make_case(ntaxa, 70, nstates, 900 + ntaxa)
    eng, om = _engine(case), _omodel(case)
    _check_map(eng.map_sites(case["aln"]), oracle.map_sites(om, case["aln"]))
    g, o = eng.null_intra(0, 5, 0, 2, 33), oracle.null_intra(om, 0, 5, 0, 2, 33)
    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
    assert np.array_equal(g["rcmin"], o["rcmin"])


def test_large_trees_150_and_600_taxa():
    """600 taxa = 1 197 branches: op stream of ~5 000 entries per class pass, 12 MB of workspace per wave.  Like the
    reference's DR likelihood the engine does not rescale: at 600 taxa site likelihoods underflow to 0 in both
    implementations (log = -inf, counts NaN) and must do so identically; 150 taxa stay finite."""
    case = make_case(150, 40, 20, 4322)
    r = _engine(case).map_sites(case["aln"])
    assert np.isfinite(r["counts"]).all() and np.isfinite(r["logL"]).all()
    _check_map(r, oracle.map_sites(_omodel(case), case["aln"]))
    case = make_case(600, 40, 20, 4321)
    eng, om = _engine(case), _omodel(case)
    with np.errstate(invalid="ignore"):
        _check_map(eng.map_sites(case["aln"]), oracle.map_sites(om, case["aln"]))
    info = eng.info()
    assert info["nbranches"] == 1197 and info["workspace_bytes"] < 80 * 2 ** 30


@pytest.mark.parametrize("seed,nstates", [(1, 20), (2, 20), (3, 4), (4, 4)])
def test_multifurcating_trees_map_and_null(seed, nstates):
    """internal nodes with 2..5 children everywhere (the kernel's general-node path, not only at the root)"""
    from test_traversal_program import _random_multifurcating
    ntaxa = 15 + 7 * seed
    parent, blen, lot = _random_multifurcating(ntaxa, seed)
    mdl = synthetic.protein_model(0.5, 4) if nstates == 20 else synthetic.dna_model(0.5, 4)
    om = oracle.Model(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    eng = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    aln, _ = oracle.simulate(om, 50 + seed, 0, 90)
    _check_map(eng.map_sites(aln), oracle.map_sites(om, aln))
    g, o = eng.null_intra(1, 9, 0, 2, 40), oracle.null_intra(om, 1, 9, 0, 2, 40)
    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)


@pytest.mark.parametrize("seed", range(16))
def test_random_configurations_against_oracle(seed):
    """seeded sweep over tree shape, taxa, sites, alphabet, number of rate classes (1..6: plain, fused-4, fused-5 with
    padding), substitution types and ambiguity"""
    from test_traversal_program import _random_multifurcating
    rng = np.random.default_rng(7000 + seed)
    ntaxa = int(rng.integers(3, 41))
    nstates = 20 if seed % 2 == 0 else 4
    ncat = int(rng.integers(1, 7))
    nsites = int(rng.integers(1, 200))
    if rng.random() < 0.4 and ntaxa >= 4:
        parent, blen, lot = _random_multifurcating(ntaxa, seed)
    else:
        parent, blen, lot = synthetic.random_tree(ntaxa, 7000 + seed)
    mdl = synthetic.protein_model(float(rng.uniform(0.3, 2.0)), ncat) if nstates == 20 else \
        synthetic.dna_model(float(rng.uniform(0.3, 2.0)), ncat)
    Bk = None
    if rng.random() < 0.4:       # two weighted substitution types
        W = rng.uniform(-1, 1, size=(2, nstates, nstates))
        Bk = np.stack([synthetic.weighted_register(mdl["Q"], W[0]), synthetic.weighted_register(mdl["Q"], W[1])])
    kw = dict(Bk=Bk) if Bk is not None else {}
    om = oracle.Model(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], nonneg=Bk is None, **kw)
    eng = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], clamp_negative=Bk is None, **kw)
    aln, _ = oracle.simulate(om, 99 + seed, 0, nsites)
    masks = None
    if rng.random() < 0.5:       # sprinkle one ambiguity id
        masks = oracle.default_masks(nstates)
        masks[nstates] = (1 << int(rng.integers(0, nstates))) | (1 << int(rng.integers(0, nstates)))
        aln = aln.copy()
        aln[rng.random(aln.shape) < 0.05] = nstates
    r = eng.map_sites(aln, masks=None if masks is None else masks[: nstates + 1])
    _check_map(r, oracle.map_sites(om, aln, masks))
    kind = int(rng.integers(0, 6))
    g, o = eng.null_intra(kind, 3 + seed, 0, 2, 37), oracle.null_intra(om, kind, 3 + seed, 0, 2, 37)
    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
    assert np.array_equal(g["rcmin"], o["rcmin"])


def test_map_sites_large_alignment_takes_the_fused_class_loop():
    """below 512 (site block, class) tasks the observed mapping runs one class per wave-task + a finalize kernel; a
    9 000-site alignment exercises the other path (all classes in one wave), same results required"""
    case = make_case(7, 9000, 20, 77)
    r = _engine(case).map_sites(case["aln"])
    _check_map(r, oracle.map_sites(_omodel(case), case["aln"]))


def test_map_sites_dna_five_classes_multifurcating_root():
    case = make_case(33, 300, 4, 7, alpha=0.8, ncat=5)
    r = _engine(case).map_sites(case["aln"])
    _check_map(r, oracle.map_sites(_omodel(case), case["aln"]))
    assert (r["counts"] >= 0).all()


# the reference's fixtures print six digits: half a unit of the sixth is 5e-6.  With the table the reference's build held
# (protein_models.jtt92_bpp2x, fitted on Myo_unif / Myo_naive / Myo.infos only) every fixture is met at that precision;
# the literature table (the product default) differs from it in the sixth decimal and meets them at 1e-4 / 5e-6.
_MYO_TABLES = [("jtt92_bpp2x", 1e-5, 2e-6, 6e-6), ("jtt92", 2e-4, 5e-6, 2e-5)]


@pytest.mark.parametrize("table,max_rel,med_rel,infos_rel", _MYO_TABLES)
def test_map_sites_myoglobin_golden_with_ambiguity(myo, table, max_rel, med_rel, infos_rel):
    """100 taxa, X/B/Z symbols, 1e-6 branches: GPU vs oracle at 1e-6, and vs the reference's own fixture."""
    Q, pi = getattr(pm, table)()
    rates, probs = pm.gamma_rates(float(myo["alpha"]), 4)
    eng = engine.Engine(myo["parent"], myo["blen"], myo["leaf_of_taxon"], Q, pi, rates, probs)
    r = eng.map_sites(myo["aln"], masks=myo["masks"])
    o = oracle.map_sites(oracle.Model(myo["parent"], myo["blen"], myo["leaf_of_taxon"], Q, pi, rates, probs), myo["aln"],
                         myo["masks"])
    _check_map(r, o)
    v = myo["vec_unif"].T
    rel = np.abs(r["counts"][:, :, 0] - v) / np.where(v > 0, v, 1)
    assert rel.max() < max_rel and np.median(rel) < med_rel, (rel.max(), np.median(rel))
    assert np.array_equal(r["rate_class"], myo["infos_rc"])
    assert np.max(np.abs(r["logL"] - myo["infos_logl"]) / np.abs(myo["infos_logl"])) < infos_rel
    assert np.max(np.abs(r["post_rate"] - myo["infos_pr"]) / myo["infos_pr"]) < infos_rel


@pytest.mark.parametrize("table,max_rel,med_rel,infos_rel", _MYO_TABLES)
def test_map_sites_myoglobin_other_fixtures_on_the_device(myo, table, max_rel, med_rel, infos_rel):
    """The HIP path itself (not only the CPU oracle) against the reference's other committed mappings: Myo_naive.vec,
    Myo_unif_grantham.vec, Myo_naive_grantham.vec, and Myo_decomp.vec / Myo_decomp_grantham.vec on the branches longer than
    1e-5 (on the 1e-6 branches the reference's difference quotient cancels: it is 0.65 % off its own Myo_unif.vec there)
    (examples/Proteins/Benchmark/CoMap)."""
    from oracle import np_oracle as npo
    Q, pi = getattr(pm, table)()
    rates, probs = pm.gamma_rates(float(myo["alpha"]), 4)
    W = pm.grantham_distance()
    tree = (myo["parent"], myo["blen"], myo["leaf_of_taxon"])
    long_branches = myo["blen"][: myo["vec_unif"].shape[0]] > 1e-5

    def check(eng, fixture, branches=slice(None)):
        r = eng.map_sites(myo["aln"], masks=myo["masks"])
        v = myo[fixture].T[:, branches]
        rel = np.abs(r["counts"][:, :, 0][:, branches] - v) / np.where(np.abs(v) > 0, np.abs(v), 1.0)
        assert rel.max() < max_rel and np.median(rel) < med_rel, (fixture, rel.max(), np.median(rel))

    plain = engine.Engine(*tree, Q, pi, rates, probs)
    check(plain, "vec_decomp", long_branches)
    check(engine.Engine(*tree, Q, pi, rates, probs, count_method=engine.COUNT_NAIVE), "vec_naive")
    B = npo.rate_matrix_register(Q, W)
    weighted = engine.Engine(*tree, Q, pi, rates, probs, Bk=B[None], clamp_negative=False)
    check(weighted, "vec_unif_grantham")
    check(weighted, "vec_decomp_grantham", long_branches)
    check(engine.Engine(*tree, Q, pi, rates, probs, count_method=engine.COUNT_NAIVE, naive_weights=W, clamp_negative=False),
          "vec_naive_grantham")


@pytest.mark.parametrize("nstates", [20, 4])
def test_continuous_rate_simulator_matches_oracle(nstates):
    """simulations.continuous = yes (CoMap.cpp:146, 213): device vs the oracle's restatement -- same rates (the Gamma
    quantile runs on the device), same alignments; and a null distribution under continuous rates"""
    case = make_case(17, 4, nstates, 31)
    eng, om = _engine(case), _omodel(case)
    for alpha, pinv in ((0.5, 0.0), (1.7, 0.2)):
        a, r = eng.simulate_continuous(77, 1000, 600, alpha, pinv)
        ao, ro = oracle.simulate_continuous(om, 77, 1000, 600, alpha, pinv)
        rel_close(r, ro, 1e-12, 1e-300)
        assert (a != ao).mean() < 1e-4          # identical but for draws within an ulp of a boundary of the cumulative row
    g = eng.null_intra_continuous(0, 5, 2, 4, 64, 0.5, 0.1)
    aln, _ = oracle.simulate_continuous(om, 5, 2 * 2 * 64, 2 * 2 * 64, 0.5, 0.1)
    sup = np.ascontiguousarray(aln.reshape(17, 2, 2, 64).transpose(1, 2, 0, 3))
    o = oracle.null_intra(om, 0, 5, 2, 4, 64, supplied=sup)
    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
    assert np.array_equal(g["rcmin"], o["rcmin"])


def test_map_sites_two_types_weighted_and_naive():
    case = make_case(10, 70, 20, 21)
    Q = case["Q"]
    W = pm.grantham_distance()
    B0 = synthetic.weighted_register(Q)
    ts = np.triu(np.ones((20, 20)), 1)
    ts = ts + ts.T
    ts[:, ::2] = 0                      # an arbitrary two-type register: type 0 = into odd states, type 1 = the rest
    Bk = np.stack([B0 * ts, B0 * (1 - ts)])
    r = _engine(case, Bk=Bk).map_sites(case["aln"])
    o = oracle.map_sites(_omodel(case, Bk=Bk), case["aln"])
    _check_map(r, o)
    tot = _engine(case).map_sites(case["aln"])
    rel_close(r["counts"].sum(-1), tot["counts"][:, :, 0], 1e-9)       # linearity over types
    Bw = synthetic.weighted_register(Q, W - W.mean())                    # signed weights: no clamping
    rw = _engine(case, Bk=Bw[None], clamp_negative=False).map_sites(case["aln"])
    ow = oracle.map_sites(_omodel(case, Bk=Bw[None], nonneg=False), case["aln"])
    rel_close(rw["counts"], ow["counts"], 1e-6, 1e-9)
    rn = _engine(case, count_method=engine.COUNT_NAIVE, naive_weights=W).map_sites(case["aln"])
    on = oracle.map_sites(_omodel(case, method=oracle.METHOD_NAIVE, naive_W=W), case["aln"])
    rel_close(rn["counts"], on["counts"], 1e-6, 1e-300)


def test_simulator_bit_exact_and_distribution():
    case = make_case(16, 4, 20, 5)
    eng, om = _engine(case), _omodel(case)
    a, c = eng.simulate(seed=987654321, g0=12345, n=3000)
    ao, co = oracle.simulate(om, 987654321, 12345, 3000)
    assert np.array_equal(c, co)
    assert np.array_equal(a, ao)
    freq = np.bincount(a.ravel(), minlength=20) / a.size
    assert np.max(np.abs(freq - case["pi"])) < 0.02
    a2, _ = eng.simulate(seed=987654321, g0=12345 + 1000, n=10)
    assert np.array_equal(a2, a[:, 1000:1010])            # counter-based: any sub-range reproduces


def test_euclidian_distance_is_exact_for_near_identical_vectors():
    """Distance.h:157-171 from the differences (a Gram form would lose every digit here)"""
    case = make_case(10, 40, 20, 33)
    eng, om = _engine(case), _omodel(case)
    counts = oracle.map_sites(om, case["aln"])["counts"]
    counts[1] = counts[0] * (1 + 1e-9)                 # two almost identical sites
    counts[2] = counts[0]
    g, o = eng.pair_stats(7, counts), oracle.pair_stats_intra(7, counts)
    rel_close(g, o, 1e-6, 1e-300)
    assert g[0, 2] == 0.0 and 0 < g[0, 1] < 1e-7
    rel_close(eng.pair_stats(7, counts[:15], counts[15:]), oracle.pair_stats_inter(7, counts[:15], counts[15:]), 1e-6, 1e-300)


@pytest.mark.parametrize("kind", range(6))
def test_pair_stats_all_kinds_intra_and_inter(kind):
    case = make_case(14, 150, 20, 31)
    eng = _engine(case)
    counts = eng.map_sites(case["aln"])["counts"]
    if kind in (2, 5):
        counts = counts * 3.0          # make ">= 1" / ">= 0.99" events common
    # engine and oracle are each within the derived bound of the exact value (tests/pair_stat_cases.py; the oracle is
    # held to it by tests/test_pair_stat_fixture.py), so they are within twice the bound of one another
    g = eng.pair_stats(kind, counts)
    o = oracle.pair_stats_intra(kind, counts)
    pc.check_two(g, o, pc.counts_bounds(f"k{kind}", counts), f"kind {kind} intra")
    g2 = eng.pair_stats(kind, counts[:40], counts[40:150])
    o2 = oracle.pair_stats_inter(kind, counts[:40], counts[40:150])
    pc.check_two(g2, o2, pc.counts_bounds(f"k{kind}", counts[:40], counts[40:150]), f"kind {kind} inter")
    iu = np.triu_indices(150, 1)
    if kind == 0:
        assert np.nanmax(np.abs(g[iu])) <= 1 + 1e-12


def test_corrected_correlation_statistic_all_paths():
    """Statistics.h:176-204 with the mean vector of CoMap.cpp:350-359: all-pairs, inter with two vectors, the fused null"""
    case = make_case(11, 70, 20, 91)
    eng, om = _engine(case), _omodel(case)
    counts = oracle.map_sites(om, case["aln"])["counts"]
    mv = counts.sum(axis=2).mean(axis=0)                       # mean total substitution vector [B]
    mv2 = mv * 0.5 + 0.01
    p1, p2 = np.concatenate([mv, mv]), np.concatenate([mv, mv2])
    g = eng.pair_stats(6, counts, mean_vectors=mv)
    rel_close(g, oracle.pair_stats_intra(6, counts, p1), 1e-6, 1e-12)
    gi = eng.pair_stats(6, counts[:30], counts[30:], mean_vectors=np.stack([mv, mv2]))
    rel_close(gi, oracle.pair_stats_inter(6, counts[:30], counts[30:], p2), 1e-6, 1e-12)
    assert np.nanmax(np.abs(g - eng.pair_stats(0, counts))) > 1e-3      # it is not the plain correlation
    gn = eng.null_intra(6, 13, 0, 2, 50, mean_vectors=mv)
    on = oracle.null_intra(om, 6, 13, 0, 2, 50, params=p1)
    rel_close(gn["stat"], on["stat"], 1e-6, 1e-12)
    with pytest.raises(engine.CmxError):
        eng.pair_stats(6, counts)


def test_pair_stats_on_reference_fixture_vectors(myo):
    """Feed the reference's own Myo_unif.vec (197 x 129) through the Gram kernel: all 8256 correlations."""
    case = dict(parent=myo["parent"], blen=myo["blen"], lot=myo["leaf_of_taxon"])
    Q, pi = pm.jtt92()
    rates, probs = pm.gamma_rates(float(myo["alpha"]), 4)
    eng = engine.Engine(myo["parent"], myo["blen"], myo["leaf_of_taxon"], Q, pi, rates, probs)
    counts = myo["vec_unif"].T[:, :, None].copy()
    for kind in (0, 3, 4):
        pc.check_two(eng.pair_stats(kind, counts), oracle.pair_stats_intra(kind, counts), pc.counts_bounds(f"k{kind}", counts),
                     f"kind {kind}")


def test_null_intra_supplied_and_simulated_match_oracle():
    case = make_case(10, 8, 20, 41)
    eng, om = _engine(case), _omodel(case)
    nrep, rep_ram = 3, 50                                   # 150 null pairs; blocks straddle replicates (50 % 64 != 0)
    o = oracle.null_intra(om, 0, 777, 0, nrep, rep_ram)
    g = eng.null_intra(0, 777, 0, nrep, rep_ram)
    rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
    rel_close(g["prmin"], o["prmin"], 1e-9)
    rel_close(g["nmin"], o["nmin"], 1e-6)
    assert np.array_equal(g["rcmin"], o["rcmin"])
    # sharding invariance: replicates [1,3) alone reproduce the tail of the full run (bit for bit)
    g2 = eng.null_intra(0, 777, 1, 3, rep_ram)
    assert np.array_equal(g2["stat"], g["stat"][rep_ram:])
    assert np.array_equal(g2["nmin"], g["nmin"][rep_ram:])
    # externally supplied alignments (deterministic cross-implementation path)
    sup = np.stack([np.stack([oracle.simulate(om, 5, (r * 2 + h) * rep_ram, rep_ram)[0] for h in range(2)])
                    for r in range(nrep)])
    for kind in (0, 1, 5):
        os_ = oracle.null_intra(om, kind, 0, 0, nrep, rep_ram, supplied=sup)
        gs = eng.null_intra(kind, 0, 0, nrep, rep_ram, supplied=sup)
        rel_close(gs["stat"], os_["stat"], 1e-6, 1e-12)


def test_null_inter_two_data_sets_match_oracle():
    """getNullDistributionInterDR (AnalysisTools.cpp:662-735): same tree topology, different branch lengths and rate
    distributions for the two data sets."""
    c1 = make_case(10, 8, 20, 61)
    c2 = dict(c1)
    rng = np.random.default_rng(3)
    c2["blen"] = c1["blen"] * rng.uniform(0.5, 1.5, size=len(c1["blen"]))
    mdl2 = synthetic.protein_model(0.9, 3)
    c2.update(rates=mdl2["rates"], probs=mdl2["probs"])
    e1, e2, o1, o2 = _engine(c1), _engine(c2), _omodel(c1), _omodel(c2)
    nrep, rep_ram = 2, 70
    for kind in (0, 1):
        g = e1.null_inter(e2, kind, 4242, 1, 1 + nrep, rep_ram)
        o = oracle.null_inter(o1, o2, kind, 4242, 1, 1 + nrep, rep_ram)
        rel_close(g["stat"], o["stat"], 1e-6, 1e-12)
        rel_close(g["prmin"], o["prmin"], 1e-9)
        rel_close(g["nmin"], o["nmin"], 1e-6)
        assert np.array_equal(g["rcmin"], o["rcmin"])


def test_map_sites_dna_iupac_ambiguity_rows():
    """ambiguity ids are extra rows of the leaf operators: 11 IUPAC codes + gap for nucleotides"""
    case = make_case(9, 130, 4, 71)
    masks = np.array([1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15, 15], dtype=np.uint32)   # A C G T R Y S W K M B D H V N -
    aln = case["aln"].copy()
    rng = np.random.default_rng(5)
    hit = rng.random(aln.shape) < 0.15
    aln[hit] = rng.integers(4, 16, size=int(hit.sum()), dtype=np.uint8)
    r = _engine(case).map_sites(aln, masks=masks)
    _check_map(r, oracle.map_sites(_omodel(case), aln, masks))
    # a second call without a table falls back to "every code >= S is fully ambiguous"
    r0 = _engine(case).map_sites(np.where(aln >= 4, 14, aln).astype(np.uint8))
    _check_map(r0, oracle.map_sites(_omodel(case), np.where(aln >= 4, 14, aln).astype(np.uint8)))
    with pytest.raises(engine.CmxError):     # more ambiguity ids than the operators carry rows for
        _engine(case).map_sites(aln, masks=np.concatenate([masks, [15]]).astype(np.uint32))


def test_pvalues_bit_exact_counts_and_na_rule():
    case = make_case(10, 90, 20, 51)
    eng, om = _engine(case), _omodel(case)
    m = eng.map_sites(case["aln"])
    stat = eng.pair_stats(0, m["counts"])
    null = eng.null_intra(0, 99, 0, 40, 64)
    pv, ns = eng.intra_pvalues(stat, m["norm"], 10, null["stat"], null["nmin"])
    po, no = oracle.intra_pvalues(stat, m["norm"], 10, null["stat"], null["nmin"])
    assert np.array_equal(ns, no)
    assert np.array_equal(np.isnan(pv), np.isnan(po))
    assert np.array_equal(pv[~np.isnan(pv)], po[~np.isnan(po)])          # same integers -> same doubles
    imax = int(np.argmax(m["norm"]))                                      # Domain upper bound is exclusive:
    others = [j for j in range(90) if j != imax and m["norm"][j] == m["norm"][imax]]
    assert not others
    iu = np.triu_indices(90, 1)
    assert (ns[iu] > 0).all()                                             # min(norm_i, norm_j) < max norm always here
    pv0, ns0 = eng.intra_pvalues(stat, m["norm"], 10, np.zeros(0), np.zeros(0))
    assert (ns0 == 0).all() and np.all(pv0[iu] == 1.0)                   # (0 - 0 + 1)/(0 + 1)


@pytest.mark.parametrize("A,T,n1,n2", [(20, 40, 37, 21), (20, 256, 9, 70), (4, 33, 18, 18)])
def test_mi_columns_mfma_path_resolved_and_mixed_columns(A, T, n1, n2):
    """fully resolved columns go through the one-hot MFMA Gram, columns with ambiguous symbols through the LDS-table
    kernel; tile overhangs (n % 4 != 0) and T % 16 != 0 are exercised"""
    rng = np.random.default_rng(A * 1000 + T)
    a1 = rng.integers(0, A, size=(T, n1)).astype(np.uint8)
    a2 = rng.integers(0, max(2, A // 3), size=(T, n2)).astype(np.uint8)
    a2[:, 0] = a2[0, 0]                                   # a constant column: H = 0, MI = 0
    a1[rng.integers(0, T, 3), rng.integers(0, n1, 3)] = A + 1    # three columns of a1 become ambiguous
    eng = engine.Engine()
    g = eng.mi_columns(a1, a2, A)
    o = oracle.mi_columns(a1, a2, A)
    rel_close(g["mi"], o["mi"], 1e-6, 1e-12)
    rel_close(g["hjoint"], o["hjoint"], 1e-6, 1e-12)
    rel_close(g["h1"], o["h1"], 1e-9, 1e-12)
    gi = eng.mi_columns(a2, None, A)
    oi = oracle.mi_columns(a2, a2, A)
    iu = np.triu_indices(n2, 1)
    rel_close(gi["mi"][iu], oi["mi"][iu], 1e-6, 1e-12)
    assert np.isnan(gi["mi"][np.tril_indices(n2)]).all()


def test_mi_columns_configuration5_shape_identities():
    """BASELINE configs[4] shape (T = 256 taxa, protein), reduced column counts; size-independent properties:
    MI = H1 + H2 - Hjoint with the entropies of the independent column kernel, MI >= 0, MI(i, i') symmetric"""
    rng = np.random.default_rng(20260103)
    T, n1, n2 = 256, 600, 500
    base = rng.integers(0, 20, size=(T, 1))
    a1 = np.where(rng.random((T, n1)) < 0.7, base, rng.integers(0, 20, size=(T, n1))).astype(np.uint8)
    a2 = np.where(rng.random((T, n2)) < 0.5, base, rng.integers(0, 20, size=(T, n2))).astype(np.uint8)
    eng = engine.Engine()
    g = eng.mi_columns(a1, a2, 20)
    ident = g["h1"][:, None] + g["h2"][None, :] - g["hjoint"]
    assert np.max(np.abs(g["mi"] - ident)) < 1e-11
    assert g["mi"].min() > -1e-12
    gt = eng.mi_columns(a2, a1, 20)
    assert np.max(np.abs(gt["mi"] - g["mi"].T)) < 1e-12
    sub = oracle.mi_columns(a1[:, :8], a2[:, :8], 20)
    rel_close(g["mi"][:8, :8], sub["mi"], 1e-6, 1e-12)


def test_compacted_rows_equal_the_reference_pair_loop():
    """cmx_intra_rows == CoETools.cpp:672-724 (filters, (i, j) order, NA rule) applied on the host to the dense matrices"""
    from comap_amd import formats
    case = make_case(10, 150, 20, 81)
    eng = _engine(case)
    m = eng.map_sites(case["aln"])
    st = eng.pair_stats(0, m["counts"])
    nl = eng.null_intra(0, 11, 0, 30, 64)
    pv, ns = eng.intra_pvalues(st, m["norm"], 6, nl["stat"], nl["nmin"])
    coords = np.arange(150) + 1
    for f in (engine.PairFilters(), engine.PairFilters(min_rate_class=1, max_rate_class_diff=1, min_rate=0.3,
                                                       max_rate_diff=1.5, min_statistic=0.2)):
        rows, count = eng.intra_rows(0, m["counts"], m["rate_class"], m["post_rate"], m["norm"], nl["stat"], nl["nmin"], 6, f)
        assert count == len(rows)
        ref = formats.to_text(formats.write_intra_stats, coords, st, m["rate_class"], m["post_rate"], m["norm"], pv, ns,
                              f.min_rate_class, f.min_rate, f.max_rate_class_diff, f.max_rate_diff, f.min_statistic)
        pvm, nsm = np.full((150, 150), np.nan), np.zeros((150, 150), dtype=np.int32)
        stm = np.full((150, 150), np.nan)
        stm[rows["i"], rows["j"]] = rows["stat"]
        pvm[rows["i"], rows["j"]] = rows["pvalue"]
        nsm[rows["i"], rows["j"]] = rows["nsim"]
        # writing the compacted rows (already filtered, already ordered) gives the same text
        lines = ["Group\tStat\tRCmin\tPRmin\tNmin\tPValue\tNsim"]
        for r in rows:
            p = ["NA", "0"] if np.isnan(r["pvalue"]) else [formats.fmt(r["pvalue"]), str(r["nsim"])]
            lines.append("\t".join(["[%d;%d]" % (coords[r["i"]], coords[r["j"]]), formats.fmt(r["stat"]), str(r["rc_min"]),
                                    formats.fmt(r["pr_min"]), formats.fmt(r["n_min"])] + p))
        assert "\n".join(lines) + "\n" == ref
    # capacity smaller than the row count: count still reports all rows
    few, total = eng.intra_rows(0, m["counts"], m["rate_class"], m["post_rate"], m["norm"], capacity=10)
    assert len(few) == 10 and total == 150 * 149 // 2 and np.isnan(few["pvalue"]).all()


def test_mica_bootstrap_nulls_match_oracle():
    """cmx_mi_pairs under Mica's two bootstrap nulls (Mica.cpp:399-548) against the oracle's column MI"""
    from comap_amd import mica
    rng = np.random.default_rng(9)
    T, n = 48, 60
    aln = rng.integers(0, 20, size=(T, n)).astype(np.uint8)
    aln[rng.random(aln.shape) < 0.03] = 21
    eng = engine.Engine()
    full = oracle.mi_columns(aln, aln, 20)
    nb = mica.bootstrap_null(eng, aln, full["h1"], seed=5, nrep_cpu=3, nrep_ram=37)
    rel_close(nb["mi"], full["mi"][nb["index1"], nb["index2"]], 1e-6, 1e-12)
    rel_close(nb["hjoint"], full["hjoint"][nb["index1"], nb["index2"]], 1e-6, 1e-12)
    assert np.array_equal(nb["hmin"], np.minimum(full["h1"][nb["index1"]], full["h1"][nb["index2"]]))
    assert (nb["index1"] == nb["index2"]).any() or True     # a site may be paired with itself, as in the reference
    # parametric: simulate under a model, score (j, j)
    case = make_case(12, 4, 20, 15)
    em, om = _engine(case), _omodel(case)
    pn = mica.parametric_null(em, seed=77, nrep_cpu=2, nrep_ram=50)
    for rep in range(2):
        a1, _ = oracle.simulate(om, 77, (rep * 2) * 50, 50)
        a2, _ = oracle.simulate(om, 77, (rep * 2 + 1) * 50, 50)
        o = oracle.mi_columns(a1, a2, 20)
        rel_close(pn["mi"][rep * 50:(rep + 1) * 50], np.diag(o["mi"]), 1e-6, 1e-12)
        rel_close(pn["hjoint"][rep * 50:(rep + 1) * 50], np.diag(o["hjoint"]), 1e-6, 1e-12)
    # with the model norms (use_model, Mica.cpp:505-530): Nmin of the two simulated sites of a pair
    pm_ = mica.parametric_null(em, seed=77, nrep_cpu=2, nrep_ram=50, with_norms=True)
    assert np.array_equal(pm_["mi"], pn["mi"])
    for rep in range(2):
        a1, _ = oracle.simulate(om, 77, (rep * 2) * 50, 50)
        a2, _ = oracle.simulate(om, 77, (rep * 2 + 1) * 50, 50)
        n1, n2 = oracle.map_sites(om, a1)["norm"], oracle.map_sites(om, a2)["norm"]
        rel_close(pm_["nmin"][rep * 50:(rep + 1) * 50], np.minimum(n1, n2), 1e-6, 1e-12)


@pytest.mark.parametrize("with_model", [False, True])
def test_mica_zscore_null_and_output_table(with_model):
    """null.method = z-score (Mica.cpp:549-607) and the rows of Mica's output file (:634-690): average MI, APC, RCW,
    Hmin / Nmin, Bs.p.value, against the oracle's column MI and p-value restatement"""
    from comap_amd import formats, mica
    rng = np.random.default_rng(21)
    T, n, ncls = 40, 37, 4
    base = rng.integers(0, 20, size=(T, 1))
    aln = np.where(rng.random((T, n)) < 0.5, base, rng.integers(0, 20, size=(T, n))).astype(np.uint8)
    aln[:, 5] = 3                                            # a constant column: entropy 0, MI 0
    eng = engine.Engine()
    o = oracle.mi_columns(aln, aln, 20)
    norms = rng.uniform(0.0, 3.0, size=n) if with_model else None
    key = norms if with_model else o["h1"]
    r0 = mica.analysis(eng, aln, norms=norms)
    avg, full = oracle.mica_average_mi(o["mi"])
    rel_close(r0["average_mi"], avg, 1e-6, 1e-12)
    assert abs(r0["full_average_mi"] - full) <= 1e-6 * full
    for which, name in enumerate(("MI", "MIp", "MIc")):
        ns, nk = mica.zscore_null(eng, r0["mi"], r0["entropy"], name, norms=norms)
        os_, ok = oracle.mica_zscore_null(which, o["mi"], key)
        assert ns.shape == (n * (n - 1) // 2,)
        iu0 = np.triu_indices(n, 1)
        fin = np.isfinite(os_) & (iu0[0] != 5) & (iu0[1] != 5)   # MIc divides by the constant column's zero average MI
        rel_close(ns[fin], os_[fin], 1e-6, 1e-12)
        rel_close(nk, ok, 1e-6, 0.0)
    ns, nk = mica.zscore_null(eng, r0["mi"], r0["entropy"], "MI", norms=norms)
    res = mica.analysis(eng, aln, norms=norms, null=(ns, nk), nclasses=ncls)
    po, no = oracle.intra_pvalues(res["mi"], key if with_model else res["entropy"], ncls, ns, nk)
    iu = np.triu_indices(n, 1)
    assert np.array_equal(res["nsim"][iu], no[iu])
    assert np.array_equal(res["pvalue"][iu], po[iu], equal_nan=True)
    txt = formats.to_text(formats.write_mica, np.arange(1, n + 1), res)
    lines = txt.split("\n")
    assert lines[0] == "Group\tMI\tAPC\tRCW\tHjoint\tHmin" + ("\tNmin" if with_model else "") + "\tBs.p.value\tBs.nb"
    assert len(lines) == n * (n - 1) // 2 + 2 and lines[1].startswith("[1;2]\t")
    f = lines[1].split("\t")
    assert f[2] == formats.fmt(r0["average_mi"][0] * r0["average_mi"][1] / r0["full_average_mi"])
    assert f[3] == formats.fmt(r0["average_mi"][0] * r0["average_mi"][1] / 2.0)


def test_mi_columns_matches_oracle_with_ambiguity():
    rng = np.random.default_rng(3)
    T, n1, n2 = 40, 37, 21
    a1 = rng.integers(0, 20, size=(T, n1)).astype(np.uint8)
    a2 = rng.integers(0, 6, size=(T, n2)).astype(np.uint8)
    a1[rng.random(a1.shape) < 0.05] = 22                  # 'X'
    a2[rng.random(a2.shape) < 0.05] = 20                  # 'B' = {D, N}
    masks = oracle.default_masks(20)
    masks[20] = (1 << 3) | (1 << 2)
    eng = engine.Engine()
    g = eng.mi_columns(a1, a2, 20, masks)
    o = oracle.mi_columns(a1, a2, 20, masks)
    rel_close(g["mi"], o["mi"], 1e-6, 1e-12)
    rel_close(g["hjoint"], o["hjoint"], 1e-6, 1e-12)
    rel_close(g["h1"], o["h1"], 1e-9, 1e-12)
    rel_close(g["h2"], o["h2"], 1e-9, 1e-12)
    gi = eng.mi_columns(a2, None, 20, masks)
    oi = oracle.mi_columns(a2, a2, 20, masks)
    iu = np.triu_indices(n2, 1)
    rel_close(gi["mi"][iu], oi["mi"][iu], 1e-6, 1e-12)


@pytest.mark.parametrize("A,T,n,max_perm", [(20, 30, 14, 200), (4, 64, 9, 1000), (20, 65, 7, 64), (20, 257, 6, 130), (4, 7, 5, 63)])
def test_mica_permutation_test_matches_oracle(A, T, n, max_perm):
    """miTest (Mica.cpp:93-118): p-value and number of permutations per pair, bit for bit (counter RNG + fixed-point
    comparison), across batch boundaries of 64 permutations and for constant columns"""
    rng = np.random.default_rng(A * 1000 + T)
    base = rng.integers(0, A, size=(T, 1))
    aln = np.where(rng.random((T, n)) < 0.55, base, rng.integers(0, A, size=(T, n))).astype(np.uint8)
    aln[:, 2] = 1                                        # constant column: p = 1, 0 permutations
    eng = engine.Engine()
    pv, npm = eng.mica_permutation_test(aln, max_perm, 99, nalpha=A)
    po, no = oracle.mica_permutation_test(aln, A, max_perm, 99)
    assert np.array_equal(npm, no) and np.array_equal(pv, po)
    iu = np.triu_indices(n, 1)
    const = (iu[0] == 2) | (iu[1] == 2)
    assert np.all(npm[const] == 0) and np.all(pv[const] == 1.0)
    assert np.all(npm[~const] >= 5) and np.all(npm <= max_perm)
    stopped = npm < max_perm
    assert np.allclose(pv[stopped & ~const], 6.0 / (npm[stopped & ~const] + 1.0))


def test_mica_permutation_test_is_calibrated():
    """independent columns: p-values roughly uniform; coupled columns: small p"""
    rng = np.random.default_rng(1)
    T, n = 100, 40
    aln = rng.integers(0, 4, size=(T, n)).astype(np.uint8)
    aln[:, 1] = (aln[:, 0] + (rng.random(T) < 0.15)) % 4     # column 1 follows column 0
    eng = engine.Engine()
    pv, npm = eng.mica_permutation_test(aln, 1000, 3, nalpha=4)
    assert pv[0] < 0.01 and npm[0] == 1000                   # pair (0, 1)
    rest = pv[n - 1:]                                        # pairs not involving column 0... (row 0 is the first n-1 pairs)
    assert 0.3 < np.median(rest) < 0.8 and (rest < 0.05).mean() < 0.12


def _with_unknowns(rng, A, T, n, ncodes, frac):
    """coupled columns with gaps / ambiguity codes sprinkled in; some columns stay fully resolved"""
    base = rng.integers(0, A, size=(T, 1))
    aln = np.where(rng.random((T, n)) < 0.55, base, rng.integers(0, A, size=(T, n))).astype(np.uint8)
    hit = rng.random((T, n)) < frac
    hit[:, :3] = False                                       # resolved columns: their mutual pairs take the resolved path
    aln[hit] = rng.integers(A, A + ncodes, size=int(hit.sum()))
    return aln


@pytest.mark.parametrize("A,T,n,max_perm,partial", [(4, 40, 10, 300, False), (20, 33, 9, 200, False), (4, 64, 9, 500, True),
                                                     (20, 130, 8, 140, True), (4, 7, 6, 63, True)])
def test_mica_permutation_test_with_unknowns_matches_oracle(A, T, n, max_perm, partial):
    """Mica.cpp:93-118 with SiteTools::*(.., resolveUnknowns = true): gaps / unknowns (and, with a mask table, partial
    ambiguity codes) spread over their compatible states.  p-value and number of permutations per pair equal the
    oracle's exactly; pairs of resolved columns are the same as without any unknown in the alignment."""
    rng = np.random.default_rng(A * 77 + T)
    if partial:
        ncodes = 5
        masks = oracle.default_masks(A)[:A + ncodes].copy()
        for c in range(A, A + ncodes - 1):                   # the last code stays "all states" (a gap)
            k = int(rng.integers(1 if c == A else 2, 4))     # one alias of a single state among them
            masks[c] = sum(1 << int(x) for x in rng.choice(A, size=k, replace=False))
    else:
        ncodes, masks = 2, None                              # two unknown codes (gap, X): the same extended code
    aln = _with_unknowns(rng, A, T, n, ncodes, 0.2)
    aln[:, 4] = np.where(aln[:, 4] < A, 1, aln[:, 4])        # constant besides its unknowns: p = 1, 0 permutations
    aln[:, 5] = A + ncodes - 1                               # nothing but gaps
    eng = engine.Engine()
    pv, npm = eng.mica_permutation_test(aln, max_perm, 41, nalpha=A, masks=masks)
    po, no = oracle.mica_permutation_test(aln, A, max_perm, 41, masks=masks)
    assert np.array_equal(npm, no) and np.array_equal(pv, po)
    iu = np.triu_indices(n, 1)
    const = np.isin(iu[0], (4, 5)) | np.isin(iu[1], (4, 5))
    if not partial:
        assert np.all(npm[const] == 0) and np.all(pv[const] == 1.0)
    # pairs (0, 1) and (0, 2) carry the pair numbers 0 and 1 whatever n is: resolved columns, so the same shuffles and the
    # same answer as in an alignment without any unknown
    p3, n3 = eng.mica_permutation_test(aln[:, :3], max_perm, 41, nalpha=A)
    assert np.array_equal(pv[:2], p3[:2]) and np.array_equal(npm[:2], n3[:2])


def test_mica_permutation_test_unknowns_many_taxa_and_limits():
    """T = 600 with gaps: one wave per workgroup; a mask table whose partial codes do not fit is refused loudly"""
    rng = np.random.default_rng(5)
    eng = engine.Engine()
    aln = _with_unknowns(rng, 4, 600, 6, 1, 0.1)
    pv, npm = eng.mica_permutation_test(aln, 70, 9, nalpha=4)
    po, no = oracle.mica_permutation_test(aln, 4, 70, 9)
    assert np.array_equal(npm, no) and np.array_equal(pv, po)
    masks = oracle.default_masks(20)[:40].copy()
    masks[33] = 0b11
    with pytest.raises(engine.CmxError, match="< 31"):
        eng.mica_permutation_test(_with_unknowns(rng, 20, 20, 5, 2, 0.1), 10, 1, nalpha=20, masks=masks)
    masks[33] = 0
    with pytest.raises(engine.CmxError, match="no state"):
        eng.mica_permutation_test(_with_unknowns(rng, 20, 20, 5, 2, 0.1), 10, 1, nalpha=20, masks=masks)


def _nh_case(nstates, seed):
    """a rooted tree with three generators spread over its branches (nonhomogeneous = general, CoETools.cpp:184-200)"""
    from oracle import np_oracle as npo
    rng = np.random.default_rng(seed)
    parent, blen, lot = synthetic.random_tree(9, seed)
    mk = synthetic.protein_model if nstates == 20 else synthetic.dna_model
    base = mk(0.6, 4 if nstates == 4 else 3)      # 4 classes: the class-fused nucleotide layout
    Qs, pis = [], []
    for m in range(3):
        pi = rng.dirichlet(np.full(nstates, 8.0))
        R = np.asarray(base["Q"]) / np.asarray(base["pi"])[None, :]      # exchangeabilities of the base generator
        R = (R + R.T) / 2
        Q = R * pi[None, :]
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
        Q /= -(pi * np.diag(Q)).sum()
        Qs.append(Q)
        pis.append(pi)
    mob = rng.integers(0, 3, size=len(parent))
    root = rng.dirichlet(np.full(nstates, 5.0))
    Bks = [[npo.rate_matrix_register(q)] for q in Qs]
    return dict(parent=parent, blen=blen, lot=lot, Qs=np.array(Qs), pis=np.array(pis), mob=mob, root=root, Bks=Bks,
                rates=base["rates"], probs=base["probs"])


@pytest.mark.parametrize("nstates", [20, 4])
def test_non_homogeneous_model_set(nstates):
    """one generator per branch + root frequency set (DRNonHomogeneousTreeLikelihood, CoETools.cpp:126-206): mapping
    against the numpy restatement; the simulator and the null against the model-set oracle"""
    from oracle import np_oracle as npo
    c = _nh_case(nstates, 17 + nstates)
    rng = np.random.default_rng(3)
    N = 70
    aln = rng.integers(0, nstates, size=(len(c["lot"]), N)).astype(np.uint8)
    eng = engine.Engine(c["parent"], c["blen"], c["lot"], c["Qs"], c["pis"], c["rates"], c["probs"], model_of_branch=c["mob"],
                        root_freqs=c["root"])
    r = eng.map_sites(aln)
    o = npo.map_sites(c["parent"], c["blen"], c["lot"], aln, oracle.default_masks(nstates), list(c["Qs"]), list(c["pis"]),
                      np.asarray(c["rates"]), np.asarray(c["probs"]), c["Bks"], model_of_branch=c["mob"], root_freqs=c["root"])
    rel_close(r["counts"], o["counts"], 1e-6, 1e-12)
    rel_close(r["logL"], o["logL"], 1e-6, 0.0)
    rel_close(r["post_rate"], o["post_rate"], 1e-6, 0.0)
    assert np.array_equal(r["rate_class"], o["rate_class"])
    # the same data under the homogeneous model of generator 0 must differ: the set is really used
    hom = engine.Engine(c["parent"], c["blen"], c["lot"], c["Qs"][0], c["pis"][0], c["rates"], c["probs"]).map_sites(aln)
    assert np.abs(hom["logL"] - r["logL"]).max() > 1e-3
    # transition matrices per branch come from the branch's generator
    P = eng.transition_matrices()
    for b in (0, 3, len(c["parent"]) - 2):
        lam, V, Vi = npo.eigen_reversible(c["Qs"][c["mob"][b]], c["pis"][c["mob"][b]])
        rel_close(P[1, b], npo.transition_matrix(lam, V, Vi, c["blen"][b] * c["rates"][1]), 1e-9, 1e-13)
    # simulator and null against the model-set oracle (tests/test_gpu_model_sets.py holds every other path against it):
    # byte-identical but for sites with a draw within 1e-9 of a boundary of its cumulative row
    om = oracle.ModelSet(c["parent"], c["blen"], c["lot"], c["Qs"], c["pis"], c["rates"], c["probs"], c["mob"], c["root"])
    sim, cls = eng.simulate(5, 0, 40000)
    so, co, near = oracle.simulate(om, 5, 0, 40000, want_near=True)
    keep = near >= oracle.FRAGILE
    assert keep.mean() >= 1 - 1e-3 and keep[:4 * 64].all()
    assert np.array_equal(sim[:, keep], so[:, keep]) and np.array_equal(cls[keep], co[keep])
    null, onull = eng.null_intra(engine.STAT_CORRELATION, 5, 0, 2, 64), oracle.null_intra(om, oracle.ST_CORRELATION, 5, 0, 2, 64)
    rel_close(null["stat"], onull["stat"], 1e-6, 1e-12)
    rel_close(null["prmin"], onull["prmin"], 1e-9)
    rel_close(null["nmin"], onull["nmin"], 1e-6)
    assert np.array_equal(null["rcmin"], onull["rcmin"])


def test_non_homogeneous_argument_errors():
    c = _nh_case(4, 1)
    bad = c["mob"].copy()
    bad[2] = 7
    with pytest.raises(engine.CmxError, match="out of range"):
        engine.Engine(c["parent"], c["blen"], c["lot"], c["Qs"], c["pis"], c["rates"], c["probs"], model_of_branch=bad,
                      root_freqs=c["root"])


def test_mica_permutation_test_many_taxa():
    """T = 1025 and T = 2047 (the limit): one wave per workgroup, the private column copies fill the LDS"""
    rng = np.random.default_rng(12)
    eng = engine.Engine()
    for T in (1025, 2047):
        aln = rng.integers(0, 4, size=(T, 4)).astype(np.uint8)
        aln[:, 1] = np.where(rng.random(T) < 0.9, aln[:, 0], aln[:, 1])
        pv, npm = eng.mica_permutation_test(aln, 70, 5, nalpha=4)
        po, no = oracle.mica_permutation_test(aln, 4, 70, 5)
        assert np.array_equal(npm, no) and np.array_equal(pv, po)
    with pytest.raises(engine.CmxError, match="ntaxa"):
        eng.mica_permutation_test(rng.integers(0, 4, size=(2048, 3)).astype(np.uint8), 10, 1, nalpha=4)


def test_label_substitution_count_is_the_naive_count_with_label_weights():
    """nijt = Label: N(x, y) = label of (x, y), 1 .. S(S-1) row by row, through the naive path"""
    case = make_case(8, 60, 4, 23)
    W = engine.label_substitution_weights(4)
    assert W[0, 1] == 1 and W[0, 3] == 3 and W[1, 0] == 4 and W[3, 2] == 12 and np.all(np.diag(W) == 0)
    r = _engine(case, count_method=engine.COUNT_NAIVE, naive_weights=W).map_sites(case["aln"])
    o = oracle.map_sites(_omodel(case, method=oracle.METHOD_NAIVE, naive_W=W), case["aln"])
    rel_close(r["counts"], o["counts"], 1e-6, 1e-12)


@pytest.mark.parametrize("A,T", [(20, 96), (4, 77), (20, 256)])
def test_mi_columns_with_gaps_everywhere(A, T):
    """unknowns (gap / X / N: compatible with every state) stay on the matrix cores as pseudo-state A and are spread
    over the states in the epilogue (weight 1/A); partial ambiguity codes still go to the LDS-table kernel.  Gaps in
    both columns of a pair, gap-only rows, intra and cross layouts, tile overhangs"""
    rng = np.random.default_rng(A + T)
    n1, n2 = 23, 18
    a1 = rng.integers(0, A, size=(T, n1)).astype(np.uint8)
    a2 = rng.integers(0, max(2, A // 2), size=(T, n2)).astype(np.uint8)
    a1[rng.random(a1.shape) < 0.15] = A          # unknown, default mask = every state
    a2[rng.random(a2.shape) < 0.30] = A + 3      # another unknown code
    a2[:, 1] = A                                 # a column of gaps only
    a1[:, 2] = np.where(rng.random(T) < 0.5, a1[:, 2], A)
    masks = oracle.default_masks(A)
    eng = engine.Engine()
    g = eng.mi_columns(a1, a2, A)
    o = oracle.mi_columns(a1, a2, A)
    rel_close(g["mi"], o["mi"], 1e-6, 1e-10)
    rel_close(g["hjoint"], o["hjoint"], 1e-6, 1e-10)
    gi = eng.mi_columns(a1, None, A)
    oi = oracle.mi_columns(a1, a1, A)
    iu = np.triu_indices(n1, 1)
    rel_close(gi["mi"][iu], oi["mi"][iu], 1e-6, 1e-10)
    rel_close(gi["hjoint"][iu], oi["hjoint"][iu], 1e-6, 1e-10)
    # a partial ambiguity code (two states) next to the gaps: that column takes the LDS-table kernel, the rest does not change
    m2 = masks.copy()
    m2[A + 1] = 0b11
    a3 = a1.copy()
    a3[rng.integers(0, T, 5), 4] = A + 1
    g3 = eng.mi_columns(a3, a2, A, masks=m2[: A + 4])
    o3 = oracle.mi_columns(a3, a2, A, m2)
    rel_close(g3["mi"], o3["mi"], 1e-6, 1e-10)
    keep = np.arange(n1) != 4
    assert np.array_equal(g3["mi"][keep], g["mi"][keep])


@pytest.mark.parametrize("S,ntaxa,nsites,ncat", [(20, 9, 70, 4), (4, 12, 90, 4), (4, 6, 40, 2)])
def test_noavg_mapping_matches_oracle(S, ntaxa, nsites, ncat):
    """nijt.average = no, nijt.joint = yes (computeSubstitutionVectorsNoAveraging, CoETools.cpp:401): counts = the table
    entry N^k(x*, y*; t_b) of the most probable pair of ancestral states; the oracle's restatement is pinned to that
    definition by brute force (tests/test_oracle_noavg.py).  Entries whose two best pairs are closer than 1e-9 relative
    may be decided differently by rounding and are skipped; likelihoods etc. stay those of the averaged call."""
    case = make_case(ntaxa, nsites, S, 300 + S)
    case["aln"][2, ::7] = S                                   # some unknowns at a leaf
    om = oracle.Model(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    o = oracle.map_sites_noavg(om, case["aln"])
    avg = oracle.map_sites(om, case["aln"])
    eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    eng.set_mapping_options(average=False, joint=True)
    g = eng.map_sites(case["aln"])
    clear = o["margin"] > 1e-9
    assert clear.mean() > 0.97
    got, want = g["counts"][clear], o["counts"][clear]
    assert np.allclose(got, want, rtol=1e-6, atol=1e-12), np.abs(got - want).max()
    full = clear.all(axis=1)
    rel_close(g["norm"][full], o["norm"][full], 1e-6, 1e-12)
    rel_close(g["logL"], avg["logL"], 1e-9)
    assert np.array_equal(g["rate_class"], avg["rate_class"])
    # back to the default: the averaged mapping again
    eng.set_mapping_options(True, True)
    rel_close(eng.map_sites(case["aln"])["counts"], avg["counts"], 1e-6, 1e-300)


@pytest.mark.parametrize("S,ntaxa,nsites,ncat", [(20, 9, 70, 4), (4, 12, 90, 4), (4, 6, 40, 2)])
def test_marginal_mappings_match_oracle(S, ntaxa, nsites, ncat):
    """nijt.joint = no (computeSubstitutionVectorsMarginal / ...NoAveragingMarginal, CoETools.cpp:399-405): the product
    of the two ends' posteriors per state and rate weights N(x, y; r_c t_b); or N(x*, y*; t_b) at the two ends' marginal
    ancestral states.  The oracle's restatement is pinned to those definitions by brute force
    (tests/test_oracle_marginal.py); parity against the reference itself is unpinned."""
    case = make_case(ntaxa, nsites, S, 400 + S, ncat=ncat)
    case["aln"][2, ::7] = S                                   # some unknowns at a leaf
    om = _omodel(case)
    avg = oracle.map_sites(om, case["aln"])
    eng = _engine(case)
    # average = yes, joint = no
    eng.set_mapping_options(average=True, joint=False)
    g, o = eng.map_sites(case["aln"]), oracle.map_sites_marginal(om, case["aln"], True)
    rel_close(g["counts"], o["counts"], 1e-6, 1e-14)
    rel_close(g["norm"], o["norm"], 1e-6, 1e-14)
    rel_close(g["logL"], avg["logL"], 1e-9)
    assert np.array_equal(g["rate_class"], avg["rate_class"])
    # average = no, joint = no: entries of N(t_b) at the marginal ancestral states; a state decided by less than 1e-9
    # relative may fall the other way
    eng.set_mapping_options(False, False)
    g0, o0 = eng.map_sites(case["aln"]), oracle.map_sites_marginal(om, case["aln"], False)
    parent = np.asarray(case["parent"])
    clear = (o0["margin"][:, :-1] > 1e-9) & (o0["margin"][:, parent[:-1]] > 1e-9)     # node and father both clear
    assert clear.mean() > 0.97
    assert np.allclose(g0["counts"][clear], o0["counts"][clear], rtol=1e-6, atol=1e-12)
    # the null follows the option: simulate -> map (variant) -> score
    eng.set_mapping_options(True, False)
    nl = eng.null_intra(engine.STAT_CORRELATION, 31, 0, 2, 24)
    for r in range(2):
        a0, _ = eng.simulate(31, (r * 2 + 0) * 24, 24)
        a1, _ = eng.simulate(31, (r * 2 + 1) * 24, 24)
        m0, m1 = eng.map_sites(a0), eng.map_sites(a1)
        st = np.array([oracle.stat_pair(0, m0["counts"][j], m1["counts"][j]) for j in range(24)])
        rel_close(nl["stat"][r * 24:(r + 1) * 24], st, 1e-9, 1e-12)
    eng.set_mapping_options(True, True)
    rel_close(eng.map_sites(case["aln"])["counts"], avg["counts"], 1e-6, 1e-300)


def test_variant_mapping_on_a_side_stream_beside_the_null():
    """with nijt.average = no the observed mapping (public entry point, side stream) and the null (engine's own
    pipeline, main stream) may run at once -- each keeps its own scratch -- and give what they give one after the other"""
    import torch
    case = make_case(10, 300, 20, 55)
    eng = _engine(case)
    eng.set_mapping_options(False, True)
    dev = torch.device("cuda:0")
    T, n = case["aln"].shape
    BK = eng.B * eng.K
    d_aln = torch.from_numpy(case["aln"]).to(dev)
    ram, nrep = 200, 3

    def run(overlap):
        counts = torch.zeros(BK, n, dtype=torch.float64, device=dev)
        norm = torch.zeros(n, dtype=torch.float64, device=dev)
        stat = torch.zeros(nrep * ram, dtype=torch.float64, device=dev)
        nmin = torch.zeros(nrep * ram, dtype=torch.float64, device=dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        if overlap:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                eng.map_sites_dev(d_aln, counts=counts, norm=norm)
            eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, nrep, ram, stat, nmin=nmin)
            torch.cuda.current_stream().wait_stream(side)
        else:
            eng.map_sites_dev(d_aln, counts=counts, norm=norm)
            torch.cuda.synchronize()
            eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, nrep, ram, stat, nmin=nmin)
        torch.cuda.synchronize()
        return counts.cpu().numpy(), norm.cpu().numpy(), stat.cpu().numpy(), nmin.cpu().numpy()

    seq = run(False)
    for _ in range(3):
        ovl = run(True)
        for a, b in zip(seq, ovl):
            assert np.array_equal(a, b, equal_nan=True)


def test_noavg_null_is_simulate_map_score():
    """AnalysisTools.cpp:598-610 with nijt.average = no: replicate r scores site j of its first simulated batch against
    site j of the second, both mapped without averaging -- rebuilt here from the engine's own simulator and mapping and
    the oracle's statistic"""
    case = make_case(8, 10, 20, 77)
    eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    eng.set_mapping_options(False, True)
    rep_begin, rep_end, ram, seed = 1, 3, 40, 909
    nl = eng.null_intra(engine.STAT_CORRELATION, seed, rep_begin, rep_end, ram)
    for r in range(rep_begin, rep_end):
        a0, _ = eng.simulate(seed, (r * 2 + 0) * ram, ram)
        a1, _ = eng.simulate(seed, (r * 2 + 1) * ram, ram)
        m0, m1 = eng.map_sites(a0), eng.map_sites(a1)
        st = np.array([oracle.stat_pair(0, m0["counts"][j], m1["counts"][j]) for j in range(ram)])
        sl = slice((r - rep_begin) * ram, (r - rep_begin + 1) * ram)
        rel_close(nl["stat"][sl], st, 1e-9, 1e-12)
        rel_close(nl["nmin"][sl], np.minimum(m0["norm"], m1["norm"]), 1e-12)
        assert np.array_equal(nl["rcmin"][sl], np.minimum(m0["rate_class"], m1["rate_class"]))


def test_label_counts_without_averaging_feed_the_mi_statistic():
    """the reference's MI statistic as it actually runs (CoETools.cpp:577-588): nijt = Label needs nijt.average = no, the
    substitution vector of a site is then the label of the most probable substitution on every branch -- integers -- and
    DiscreteMutualInformationStatistic bins them with the bounds -0.5, 0.5, ..., S(S-1) + 0.5"""
    case = make_case(10, 50, 4, 31)
    W = engine.label_substitution_weights(4)
    eng = _engine(case, count_method=engine.COUNT_NAIVE, naive_weights=W)
    eng.set_mapping_options(False, True)
    r = eng.map_sites(case["aln"])
    o = oracle.map_sites_noavg(_omodel(case, method=oracle.METHOD_NAIVE, naive_W=W), case["aln"])
    clear = o["margin"] > 1e-9
    assert np.array_equal(r["counts"][clear], o["counts"][clear])
    lab = r["counts"][clear]
    assert np.all(lab == np.round(lab)) and lab.min() >= 0 and lab.max() <= 12
    x, y = o["argmax"][clear] // 4, o["argmax"][clear] % 4
    assert np.array_equal(lab[:, 0], W[x, y])


def test_null_simulator_kernels_and_passes_agree_with_the_plain_simulator(tmp_path):
    """cmx_null_simulate_dev lays the replicates' alignments out as [replicate][batch][taxon][rep_ram] with the draws of
    cmx_simulate at g = ((rep * 2 + batch) * rep_ram + j) -- for both of its kernels (tables in LDS above 2 M sites,
    gathers below) -- and a null computed in several passes (alignment buffer capped) equals the one-pass null."""
    import os, subprocess, sys, textwrap
    import torch
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    case = make_case(8, 10, 20, 5)
    eng = _engine(case)
    dev = torch.device("cuda:0")
    T = len(case["lot"])
    case6 = make_case(8, 10, 20, 6, ncat=6)                     # six classes: a node block of 15 360 B, the largest of the two-piece shape
    for e, rb, re, ram in ((eng, 3, 5, 700), (eng, 0, 2, 600_000), (_engine(case6), 1, 3, 550_001)):
        # 2 800 sites (gather kernel); 2.4 M and 2.2 M sites (LDS-table kernel, one batch of 1 024 sites per workgroup)
        n = (re - rb) * 2 * ram
        buf = torch.empty(n * T, dtype=torch.uint8, device=dev)
        e.null_simulate_dev(77, rb, re, ram, buf)
        torch.cuda.synchronize()
        got = buf.cpu().numpy().reshape(re - rb, 2, T, ram)
        want, _ = e.simulate(77, rb * 2 * ram, n)                # [T, n], column s <-> g = rb * 2 * ram + s
        want = want.reshape(T, re - rb, 2, ram).transpose(1, 2, 0, 3)
        assert np.array_equal(got, want)
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        import torch
        sys.path.insert(0, %r + '/tests')
        from conftest import make_case
        from comap_amd import engine
        case = make_case(8, 10, 20, 5)
        eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
        nl = eng.null_intra(engine.STAT_CORRELATION, 5, 2, 9, 50)
        np.save(sys.argv[1], np.stack([nl["stat"], nl["nmin"], nl["prmin"], nl["rcmin"].astype(float)]))
    """ % (ROOT, ROOT))
    outs = []
    for cap in (None, str(3 * 2 * T * 50)):                      # one pass; passes of three replicates
        env = dict(os.environ)
        if cap:
            env["CMX_NULL_PASS_BYTES"] = cap
        f = tmp_path / ("null_%s.npy" % (cap or "all"))
        subprocess.check_call([sys.executable, "-c", code, str(f)], env=env, cwd=ROOT)
        outs.append(np.load(f))
    assert np.array_equal(outs[0], outs[1], equal_nan=True)


def test_device_resident_handovers_equal_the_host_paths():
    """the continuous-rate null (simulator -> mapping) and Mica's parametric bootstrap (simulator -> MI of
    the (j, j) pairs -> norms) no longer cross PCIe between their stages; same bits as the paths through host memory"""
    from comap_amd import mica
    case = make_case(9, 10, 20, 41)
    eng = _engine(case)
    a = eng.null_intra_continuous(engine.STAT_CORRELATION, 5, 2, 5, 64, 0.5, 0.1)
    b = eng.null_intra_continuous_via_host(engine.STAT_CORRELATION, 5, 2, 5, 64, 0.5, 0.1)
    for k in ("stat", "nmin", "prmin", "rcmin"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for norms in (False, True):
        p = mica.parametric_null(eng, seed=77, nrep_cpu=3, nrep_ram=50, with_norms=norms)
        q = mica.parametric_null_via_host(eng, seed=77, nrep_cpu=3, nrep_ram=50, with_norms=norms)
        assert p.keys() == q.keys()
        for k in p:
            assert np.array_equal(p[k], q[k]), k


def _inter_rows_restated(stat, m1, m2, f):
    """CoETools::computeInterStats' pair loop (CoETools.cpp:786-828) restated on a dense statistic matrix"""
    out = []
    n1, n2 = stat.shape
    for i in range(n1):
        ci, ri = int(m1["rate_class"][i]), m1["post_rate"][i]
        if ci < f.min_rate_class1 or ri < f.min_rate1:
            continue
        js = [i] if f.independent_comparisons else range(n2)
        for j in js:
            cj, rj = int(m2["rate_class"][j]), m2["post_rate"][j]
            if cj < f.min_rate_class2 or rj < f.min_rate2:
                continue
            if f.max_rate_class_diff >= 0 and abs(cj - ci) > f.max_rate_class_diff:
                continue
            if f.max_rate_diff >= 0 and abs(rj - ri) > f.max_rate_diff:
                continue
            st = stat[i, j]
            if abs(st) < f.min_statistic:
                continue
            nj = m2["norm"][min(i, n2 - 1)] if f.reference_norm_quirk else m2["norm"][j]     # :803 reads norms2[i]
            out.append((i, j, st, min(ci, cj), min(ri, rj), min(m1["norm"][i], nj)))
    return out


@pytest.mark.parametrize("kind", [engine.STAT_CORRELATION, engine.STAT_COMPENSATION, engine.STAT_DISCRETE_MI_BOUNDS])
def test_inter_rows_on_the_device_match_the_reference_loop(kind):
    """the inter-gene pair loop (filters of CoETools.cpp:786-812, independant comparisons, compaction) runs
    on the device; the rows equal the reference's loop restated over the oracle's statistic, pair for pair"""
    case = make_case(12, 150, 20, 88)
    case2 = dict(case)
    case2["blen"] = case["blen"] * 1.4
    e1, e2 = _engine(case), _engine(case2)
    m1 = e1.map_sites(case["aln"])
    m2 = e2.map_sites(case["aln"][:, ::-1][:, :150 if kind != engine.STAT_CORRELATION else 97].copy())
    thr = [0.0, 0.02, 0.2, 1.0, 100.0] if kind == engine.STAT_DISCRETE_MI_BOUNDS else 0.99
    okind = oracle.ST_DISCRETE_MI if kind == engine.STAT_DISCRETE_MI_BOUNDS else kind
    op = np.concatenate([[len(thr)], thr]) if kind == engine.STAT_DISCRETE_MI_BOUNDS else None
    dense = oracle.pair_stats_inter(okind, m1["counts"], m2["counts"], params=op)
    n2 = len(m2["norm"])
    cases = [engine.InterFilters(),
             engine.InterFilters(min_rate_class1=1, min_rate_class2=2, max_rate_class_diff=1, min_rate1=0.2, min_rate2=0.1,
                                 max_rate_diff=1.5, min_statistic=0.05),
             engine.InterFilters(reference_norm_quirk=True, min_statistic=0.1)]
    if n2 == 150:
        cases.append(engine.InterFilters(independent_comparisons=True, min_rate_class1=1))
    for f in cases:
        rows, count = e1.inter_rows(kind, m1, m2, f, threshold=thr)
        want = _inter_rows_restated(dense, m1, m2, f)
        assert count == len(want) == len(rows) and count > 0
        assert [(int(r["i"]), int(r["j"])) for r in rows] == [(w[0], w[1]) for w in want]
        rel_close(rows["stat"], [w[2] for w in want], 1e-6, 1e-12)
        assert np.array_equal(rows["rc_min"], [w[3] for w in want])
        rel_close(rows["pr_min"], [w[4] for w in want], 1e-12)
        rel_close(rows["n_min"], [w[5] for w in want], 1e-12)
        assert np.isnan(rows["pvalue"]).all() and (rows["nsim"] == 0).all()
    with pytest.raises(engine.CmxError, match="same length"):
        e1.inter_rows(kind, m1, {k: v[:60] for k, v in m2.items()}, engine.InterFilters(independent_comparisons=True), threshold=thr)


@pytest.mark.parametrize("T,n1,n2", [(40, 50, 77), (100, 37, 205), (200, 61, 100), (256, 130, 260), (300, 40, 50), (257, 61, 40), (512, 50, 77),
                                     (600, 30, 25)])
def test_mica_four_wave_kernels_mixed_blocks_against_oracle(T, n1, n2):
    """The protein path up to 512 taxa (cmx_mica4.hip: plain and weighted instantiation, operand registers for 2 / 4 / 8 /
    16 k-steps, the last at one workgroup per CU) and above (eight-wave kernel): column counts that are no multiple of the 12 x 3 tile, runs longer than one
    chunk of tiles (n2 = 205, 260), columns with unknowns scattered so that blocks and tiles mix clean and gapped
    columns, some columns all unknown, one column with a partial ambiguity code; rectangle and intra layout."""
    rng = np.random.default_rng(T + n1)
    A = 20
    masks = oracle.default_masks(A).copy()
    masks[A + 1] = 0b101                                    # partial ambiguity: two states
    base = rng.integers(0, A, size=(T, 1))

    def draw(n, p):
        a = np.where(rng.random((T, n)) < p, base, rng.integers(0, A, size=(T, n))).astype(np.uint8)
        gapped = rng.random(n) < 0.3
        a[(rng.random((T, n)) < 0.2) & gapped[None, :]] = A   # unknowns in 30 % of the columns
        a[:, n // 2] = A                                       # a column of unknowns only
        return a

    a1, a2 = draw(n1, 0.6), draw(n2, 0.4)
    a1[rng.integers(0, T, 3), 7] = A + 1
    eng = engine.Engine()
    g = eng.mi_columns(a1, a2, A, masks=masks[: A + 2])
    o = oracle.mi_columns(a1, a2, A, masks)
    rel_close(g["mi"], o["mi"], 1e-6, 1e-10)
    rel_close(g["hjoint"], o["hjoint"], 1e-6, 1e-10)
    gi = eng.mi_columns(a2, None, A, masks=masks[: A + 2])
    oi = oracle.mi_columns(a2, a2, A, masks)
    iu = np.triu_indices(n2, 1)
    rel_close(gi["mi"][iu], oi["mi"][iu], 1e-6, 1e-10)
    rel_close(gi["hjoint"][iu], oi["hjoint"][iu], 1e-6, 1e-10)
    assert np.isnan(gi["mi"][np.tril_indices(n2)]).all() and np.isnan(gi["hjoint"][np.tril_indices(n2)]).all()


@pytest.mark.parametrize("T,blocks", [(256, 20), (512, 20), (512, 40)])
def test_mica_weighted_kernel_queue_of_large_cells_beyond_one_wave(T, blocks):
    """The weighted instantiation looks cells below 4 096 / 400 = 10.24 taxa up in LDS and queues the larger ones per wave
    for one gather when the tile's sums are reduced.  Here every pair of columns has twenty cells of 12 or 13 taxa (the
    columns are the same partition of the 256 taxa into twenty blocks, states permuted per column) and every column two
    unknowns: a wave's nine pairs queue 180 cells per tile, three rounds of its 64 lanes (the bound is 225).  With 512 taxa
    (sixteen k-steps, queue of 464) twenty cells of 25 or 26 taxa, or -- forty blocks, the first column's state by block
    modulo 20, the second's by block / 2 -- FORTY cells of 12 or 13 taxa per pair: 360 queued cells per wave and tile."""
    rng = np.random.default_rng(5)
    A, n1, n2 = 20, 26, 11
    block = np.arange(T) * blocks // T

    def draw(n, key):
        a = np.stack([rng.permutation(A).astype(np.uint8)[key] for _ in range(n)], axis=1)
        for c in range(n):
            a[rng.choice(T, 2, replace=False), c] = A
        return np.ascontiguousarray(a)

    a1, a2 = draw(n1, block % A), draw(n2, block * A // blocks)
    eng = engine.Engine()
    g = eng.mi_columns(a1, a2, A)
    o = oracle.mi_columns(a1, a2, A, oracle.default_masks(A))
    rel_close(g["mi"], o["mi"], 1e-6, 1e-10)
    rel_close(g["hjoint"], o["hjoint"], 1e-6, 1e-10)
    # (blocks = 20: nearly the full ln 20; 40: each state of one column meets two of the other, ln 20 - ln 2)
    assert o["mi"].min() > (2.5 if blocks == 20 else 1.9)
    g2 = eng.mi_columns(a1, a2, A)
    assert np.array_equal(g["mi"], g2["mi"]) and np.array_equal(g["hjoint"], g2["hjoint"])   # same bits run to run


def test_pvalues_binned_lookup_is_the_linear_count():
    """The p-value lookup finds the bin of the statistic (equal-width bins between the class's 1/64 and 63/64 quantiles,
    one per eight sorted null values) and searches inside it; the count must be the reference's linear scan with strict
    '<' (CoETools.cpp:712-717) for classes whose sizes are no multiple of the bin size, classes too small for bins, an
    empty class, heavy ties, statistics below and above every null value -- in the dense call and in the pass that
    writes the compacted rows."""
    rng = np.random.default_rng(77)
    n, ncls, nnull = 120, 7, 200_003
    norms = np.concatenate([rng.uniform(0.0, 5.0, n - 1), [5.0]])
    width = 5.0 / ncls
    null_nmin = rng.uniform(0.0, 5.0, nnull)
    null_nmin[(null_nmin >= 2 * width) & (null_nmin < 3 * width)] = 0.1 * width     # class 2 stays empty
    small = np.flatnonzero((null_nmin >= 4 * width) & (null_nmin < 5 * width))
    null_nmin[small[37:]] = 5 * width + 0.01                                         # class 4 keeps 37 values
    null_stat = np.round(rng.normal(0.0, 0.3, nnull), 3)                             # three decimals: ties everywhere
    null_stat[rng.integers(0, nnull, 50)] = np.nan                                   # dropped from their class
    stat = np.round(rng.normal(0.0, 0.35, (n, n)), 3)
    stat = np.triu(stat, 1) + np.triu(stat, 1).T
    stat[0, 1] = stat[1, 0] = -9.0
    stat[0, 2] = stat[2, 0] = 9.0
    eng = engine.Engine()
    pv, ns = eng.intra_pvalues(stat, norms, ncls, null_stat, null_nmin)
    opv, ons = oracle.intra_pvalues(stat, norms, ncls, null_stat, null_nmin)
    iu = np.triu_indices(n, 1)
    assert np.array_equal(ns[iu], ons[iu])
    assert np.array_equal(pv[iu], opv[iu], equal_nan=True)
    assert set(np.unique(ons[iu])) >= {0, 37}
    # the row writer (cmx_intra_rows_range_dev) looks the same values up itself, for the pairs it writes
    import torch
    from test_gpu_fullsize import _rows_range
    case = make_case(9, n, 20, 5)
    e2 = _engine(case)
    m = e2.map_sites(case["aln"])
    scale = float(m["norm"].max()) / 5.0
    dev = torch.device("cuda:0")
    cbm = torch.from_numpy(np.ascontiguousarray(m["counts"].reshape(n, -1).T)).to(dev)
    rc, pr, nm = (torch.from_numpy(m[k]).to(dev) for k in ("rate_class", "post_rate", "norm"))
    rows = _rows_range(e2, cbm, rc, pr, nm, torch.from_numpy(null_stat).to(dev), torch.from_numpy(null_nmin * scale).to(dev), ncls,
                       engine.STAT_CORRELATION, 0, n)
    assert len(rows) == n * (n - 1) // 2
    st = e2.pair_stats(engine.STAT_CORRELATION, m["counts"])
    opv2, ons2 = oracle.intra_pvalues(st, m["norm"], ncls, null_stat, null_nmin * scale)
    assert np.array_equal(rows["nsim"], ons2[iu]) and np.array_equal(rows["pvalue"], opv2[iu], equal_nan=True)


@pytest.mark.parametrize("dist", ["continuous", "outliers", "few_values", "constant", "two_clusters"])
def test_pvalues_binned_lookup_on_awkward_null_distributions(dist):
    """The bins are cut in the statistic's value, so the shapes that stress them: a continuous null (every bin a
    handful of values), infinite and huge outliers (the tails fall into the first and last bin), a statistic that takes
    six values (most bins empty, a few hold a sixth of the class), a constant null (no bins at all), two far clusters
    (one thread fills the empty bins between them).  Always the linear count of the oracle."""
    rng = np.random.default_rng(len(dist))
    n, ncls, nnull = 90, 4, 150_001
    norms = np.concatenate([rng.uniform(0.0, 3.0, n - 1), [3.0]])
    null_nmin = rng.uniform(0.0, 3.0, nnull)
    stat = rng.normal(0.0, 0.4, (n, n))
    if dist == "continuous":
        null_stat = rng.normal(0.0, 0.3, nnull)
    elif dist == "outliers":
        null_stat = rng.normal(0.0, 0.3, nnull)
        null_stat[rng.integers(0, nnull, 40)] = np.inf
        null_stat[rng.integers(0, nnull, 40)] = -np.inf
        null_stat[rng.integers(0, nnull, 40)] = 1.0e308
        null_stat[rng.integers(0, nnull, 40)] = -1.0e308
        stat[3, 4] = np.inf
        stat[5, 6] = -np.inf
        stat[7, 8] = 1.0e308
    elif dist == "few_values":
        null_stat = rng.integers(0, 6, nnull).astype(np.float64)
        stat = rng.integers(-1, 8, (n, n)).astype(np.float64)
        stat[::3] += 0.5
    elif dist == "constant":
        null_stat = np.full(nnull, 0.25)
        stat[2, 3] = 0.25
    else:
        null_stat = np.where(rng.random(nnull) < 0.5, rng.normal(-50.0, 0.01, nnull), rng.normal(70.0, 0.01, nnull))
        stat = np.where(rng.random((n, n)) < 0.5, rng.normal(-50.0, 0.02, (n, n)), rng.normal(70.0, 0.02, (n, n)))
        stat[1, 2] = 0.0
    stat = np.triu(stat, 1) + np.triu(stat, 1).T
    # the statistic equal to a null value, and one ulp either side of it
    v = null_stat[np.isfinite(null_stat)][:20]
    stat[0, 1:21] = v
    stat[1, 2:22] = np.nextafter(v, np.inf)
    stat[2, 3:23] = np.nextafter(v, -np.inf)
    stat = np.triu(stat, 1) + np.triu(stat, 1).T
    eng = engine.Engine()
    pv, ns = eng.intra_pvalues(stat, norms, ncls, null_stat, null_nmin)
    opv, ons = oracle.intra_pvalues(stat, norms, ncls, null_stat, null_nmin)
    iu = np.triu_indices(n, 1)
    assert np.array_equal(ns[iu], ons[iu])
    assert np.array_equal(pv[iu], opv[iu], equal_nan=True)


@pytest.mark.parametrize("T,n1,n2", [(40, 70, 33), (100, 130, 300), (256, 200, 129), (300, 40, 50)])
def test_mica_four_wave_nucleotide_kernel_against_oracle(T, n1, n2):
    """Nucleotides up to 256 taxa (cmx_mica4.hip, mica_dna4_kernel: sixteen columns per 64-row block, the weighted table
    whole in LDS, one instantiation for columns with and without unknowns) and above (one-column-per-tile kernel): column
    counts that are no multiple of the 64 x 16 tile, several runs, unknowns in a third of the columns, a column of unknowns
    only, a column with a partial ambiguity code (R = A or G); rectangle and intra layout."""
    rng = np.random.default_rng(T + n2)
    A = 4
    masks = oracle.default_masks(A).copy()
    masks[A + 1] = 0b0101                                    # R: two states
    base = rng.integers(0, A, size=(T, 1))

    def draw(n, p):
        a = np.where(rng.random((T, n)) < p, base, rng.integers(0, A, size=(T, n))).astype(np.uint8)
        gapped = rng.random(n) < 0.33
        a[(rng.random((T, n)) < 0.2) & gapped[None, :]] = A
        a[:, n // 2] = A
        return a

    a1, a2 = draw(n1, 0.6), draw(n2, 0.4)
    a1[rng.integers(0, T, 3), 5] = A + 1
    eng = engine.Engine()
    g = eng.mi_columns(a1, a2, A, masks=masks[: A + 2])
    o = oracle.mi_columns(a1, a2, A, masks)
    rel_close(g["mi"], o["mi"], 1e-6, 1e-10)
    rel_close(g["hjoint"], o["hjoint"], 1e-6, 1e-10)
    gi = eng.mi_columns(a2, None, A, masks=masks[: A + 2])
    oi = oracle.mi_columns(a2, a2, A, masks)
    iu = np.triu_indices(n2, 1)
    rel_close(gi["mi"][iu], oi["mi"][iu], 1e-6, 1e-10)
    rel_close(gi["hjoint"][iu], oi["hjoint"][iu], 1e-6, 1e-10)
    assert np.isnan(gi["mi"][np.tril_indices(n2)]).all() and np.isnan(gi["hjoint"][np.tril_indices(n2)]).all()


def test_mi_columns_one_context_serves_every_path_in_turn_and_back():
    """One model-less context through the five paths of the column stage and back to the first: four-wave protein (40
    taxa), eight-wave protein (600), four-wave nucleotide (40), one-column-per-tile nucleotide (300), LDS tables only (2 048
    taxa, 5 x 4 columns).  Each visit is a rectangle call and an intra call; the unknowns are in the second alignment only on
    one visit and in the first only on the next, and each alignment has one column with a partial ambiguity code.  The
    context's scratch buffers keep their names from path to path and only grow, so a path that reads a buffer another path
    sized or filled shows here: every result is the oracle's and, bit for bit, that of the same call on a fresh context."""
    visits = [(20, 40, 30, 25), (20, 600, 30, 25), (4, 40, 30, 25), (4, 300, 30, 25), (4, 2048, 5, 4), (20, 40, 30, 25)]
    eng = engine.Engine()
    for k, (A, T, n1, n2) in enumerate(visits):
        rng = np.random.default_rng(1000 + k)
        masks = oracle.default_masks(A).copy()
        masks[A + 1] = 0b101                                    # partial ambiguity: two states
        base = rng.integers(0, A, size=(T, 1))

        def draw(n, p, unknowns):
            a = np.where(rng.random((T, n)) < p, base, rng.integers(0, A, size=(T, n))).astype(np.uint8)
            if unknowns:
                gapped = rng.random(n) < 0.3
                gapped[0] = True
                a[(rng.random((T, n)) < 0.2) & gapped[None, :]] = A
                a[:, n // 2] = A                                   # a column of unknowns only
            return a

        a1, a2 = draw(n1, 0.6, k % 2 == 1), draw(n2, 0.4, k % 2 == 0)
        a1[rng.integers(0, T, 3), n1 // 4] = A + 1
        a2[rng.integers(0, T, 3), n2 - 1] = A + 1
        for x, y in ((a1, a2), (a2, None)):
            g = eng.mi_columns(x, y, A, masks=masks[: A + 2])
            f = engine.Engine().mi_columns(x, y, A, masks=masks[: A + 2])
            o = oracle.mi_columns(x, x if y is None else y, A, masks)
            for key in ("mi", "hjoint"):
                if y is None:
                    iu = np.triu_indices(x.shape[1], 1)
                    rel_close(g[key][iu], o[key][iu], 1e-6, 1e-10)
                    assert np.isnan(g[key][np.tril_indices(x.shape[1])]).all()
                else:
                    rel_close(g[key], o[key], 1e-6, 1e-10)
                assert np.array_equal(g[key], f[key], equal_nan=True), (k, key, y is None)


@pytest.mark.parametrize("dim,n1,n2", [(5, 7, 4), (125, 70, 33), (64, 130, 130), (2, 3, 3)])
def test_analysis_tools_vector_matrices(dim, n1, n2):
    """AnalysisTools::compute{ScalarProduct,Cosinus,Correlation,Covariance}Matrix (CoMap/AnalysisTools.cpp:102-339) on the
    Gram kernel (cmx_vector_matrix) against the definitions (VectorTools::scalar / cos / cor / cov, unbiased), for the
    one-set forms (symmetric, the reference's diagonal), the two-set forms and independantComparisons; a model-less
    context serves"""
    rng = np.random.default_rng(dim * 1000 + n1)
    a, b = rng.normal(size=(n1, dim)), rng.normal(loc=0.3, size=(n2, dim))
    eng = engine.Engine()

    def ref(kind, x, y):
        if kind == engine.STAT_SCALAR_PRODUCT:
            return x @ y.T
        if kind == engine.STAT_COSINUS:
            return (x @ y.T) / np.outer(np.linalg.norm(x, axis=1), np.linalg.norm(y, axis=1))
        xc, yc = x - x.mean(1, keepdims=True), y - y.mean(1, keepdims=True)
        cov = (xc @ yc.T) / (dim - 1)
        if kind == engine.STAT_COVARIANCE:
            return cov
        return cov / np.outer(np.sqrt((xc ** 2).sum(1) / (dim - 1)), np.sqrt((yc ** 2).sum(1) / (dim - 1)))

    for kind in (engine.STAT_SCALAR_PRODUCT, engine.STAT_COSINUS, engine.STAT_CORRELATION, engine.STAT_COVARIANCE):
        one = eng.vector_matrix(kind, a)
        r = ref(kind, a, a)
        if kind in (engine.STAT_COSINUS, engine.STAT_CORRELATION):
            assert np.all(np.diag(one) == 1.0)                      # matrix[i][i] = 1 (AnalysisTools.cpp:178, 236)
        assert np.array_equal(one, one.T)                           # matrix[i][j] = matrix[j][i]
        rel_close(one, r, 1e-9, 1e-12)
        two = eng.vector_matrix(kind, a, b)
        rel_close(two, ref(kind, a, b), 1e-9, 1e-12)
        if n1 == n2:
            ind = eng.vector_matrix(kind, a, b, independent=True)
            assert np.all(ind[~np.eye(n1, dtype=bool)] == 0.0)      # only j = i is computed (AnalysisTools.cpp:150-157)
            rel_close(np.diag(ind), np.diag(ref(kind, a, b)), 1e-9, 1e-12)
        else:
            with pytest.raises(engine.CmxError, match="independant comparisons"):
                eng.vector_matrix(kind, a, b, independent=True)
    # the scalar product is a pair statistic like the others (the raw Gram of the type-0 counts)
    case = make_case(9, 40, 20, 3)
    e2 = _engine(case)
    m = e2.map_sites(case["aln"])
    st = e2.pair_stats(engine.STAT_SCALAR_PRODUCT, m["counts"])
    iu = np.triu_indices(40, 1)
    rel_close(st[iu], (m["counts"][:, :, 0] @ m["counts"][:, :, 0].T)[iu], 1e-9, 1e-300)
