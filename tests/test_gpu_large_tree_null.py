"""-m gpu: everything that builds a null distribution, on trees beyond 64 leaves (tests/large_tree_cases.py), against the
oracle and path against path.

Bars, the ones the same comparison has on small trees (test_against_the_oracle_with_many_cherries,
test_random_configurations_against_oracle): stat rel_close(1e-6, 1e-12), nmin and prmin rel_close(1e-6), rcmin equal.
Between the paths of one engine, and between the engines with and without the cherry message table: the same bytes in
every output.

What only a larger tree reaches, and the case that reaches it:
* null_pattern_moments_kernel holds a column in registers up to kMomentRows = 128 branches and calls pattern_moments above:
  u65 (B = 127) and r65 (128) take the first arm, u66 (129) and every larger tree the second; Correlation and Covariance
  are scored from its moments and must be the per-site path's bytes -- on the null's own draws and on supplied alignments
  with 171 distinct columns among 222, where the table's tiles hold real duplicates at B = 129, 196, 197, 254, 258, 259;
* null_pattern_key_kernel (ram 53 and 37) and null_pattern_key4_kernel (ram 48) pack a column in 16-taxon pieces and the
  flag kernel compares them: five pieces with 2 taxa in the last (T = 66), nine with 3 (T = 131), eight full ones (T = 128),
  seven with 4 (T = 100, myo), nine with 2 and with 12 (T = 130, 140); null_pattern_count() must be the number of distinct
  columns, which a piece left out of the hash or the comparison would lower;
* the null-mode walks kModeNull, kModeNullMsg, kModeNullPatterns and kModeNullPatternsMsg over a resolved stream, a wait
  plan, an LDS-slot plan and stored workspace vectors of a tree of up to 260 nodes: every (table, patterns) combination;
  the message table holds 60 or more cherries on bal128 (14 in the tests of small trees);
* the class-fused nucleotide walks (16 and 20 device states, cherry tables; six classes as two passes of 20) and the
  unfused 4-state one (two classes) at 131 and 128 leaves, per site and forced onto the pattern path;
* the unfused null (simulate_kernel with rep_ram and gstep -> map -> diagonal pairs: MI with bounds, branch weights), the
  inter-gene null and the continuous-rate null on 260 nodes.

Measured on one MI355X, the largest error / bar (1.0 = at the bar) and the pair comparisons per path; the module prints the
table anew when it has run (pytest -s):

    path                          stat      nmin      prmin     pairs
    protein patterns, table on    4.3e-04   1.2e-06   1.6e-09   12810
    protein per site, table on    4.3e-04   1.2e-06   1.6e-09   12810
    protein patterns, table off   4.3e-04   1.2e-06   1.6e-09   12810
    protein per site, table off   4.3e-04   1.2e-06   1.6e-09   12810
    16 fused states               3.9e-06   1.5e-08   9.0e-10   1464
    20 fused states               3.8e-04   1.9e-08   1.2e-09   2928
    4 states unfused              2.3e-07   2.9e-09   2.5e-10   1464
    unfused null, MI(bounds)      1.0e-06   3.2e-07   1.1e-09   66
    unfused null, weights         8.3e-06   3.2e-07   1.1e-09   132
    inter                         2.0e-05   1.9e-07   8.4e-10   140
    continuous                    4.2e-07   3.2e-07   6.0e-10   66
    under the scratch guard       1.0e-04   2.2e-07   1.1e-09   1080

(the four protein rows are equal because the four paths give the same bytes; every path agreed in every byte, no bug found)

Not here: 50-digit references at this size (minutes per 20-state case), trees that underflow without scaling."""
import numpy as np
import pytest

import large_tree_cases as ltc
import oracle
import weighted_reference as wr
from comap_amd import engine
from conftest import rel_close

pytestmark = pytest.mark.gpu

OUT = ("stat", "nmin", "prmin", "rcmin")
BARS = (("stat", 1e-6, 1e-12), ("nmin", 1e-6, 0.0), ("prmin", 1e-6, 0.0))
FIGURES = {}       # path -> [largest error over the bar of stat, nmin, prmin; pairs compared]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n    %-28s  %-8s  %-8s  %-8s  %s" % ("path", "stat", "nmin", "prmin", "pairs"))
    for path, f in FIGURES.items():
        print("    %-28s  %.1e   %.1e   %.1e   %d" % (path, f[0], f[1], f[2], f[3]))


def _hold(path, got, ref):
    """the bars of the module's docstring; the figures are recorded before anything is asserted"""
    fig = FIGURES.setdefault(path, [0.0, 0.0, 0.0, 0])
    for i, (key, rtol, atol) in enumerate(BARS):
        g, r = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        ok = ~(np.isnan(g) | np.isnan(r))
        err, tol = np.abs(g[ok] - r[ok]), rtol * np.abs(r[ok]) + atol
        over = np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))
        fig[i] = max(fig[i], float(over.max()) if over.size else 0.0)
    fig[3] += len(ref["stat"])
    for key, rtol, atol in BARS:
        rel_close(got[key], ref[key], rtol, atol)
    assert got["rcmin"].dtype == np.int32 and np.array_equal(got["rcmin"], ref["rcmin"])


def _same_bytes(a, b, what):
    for key in OUT:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (what, key, int((a[key] != b[key]).sum()))


def _null(eng, case, inp, kind, patterns):
    """the case's null of that input on one path; asserts that the path ran: the columns mapped are the distinct ones with
    patterns on and every site of every pair with them off"""
    nrep, ram = ltc.shape_of(inp)
    eng.set_null_patterns(patterns)
    try:
        if inp == ltc.FORCED:
            r = eng.null_intra(kind, 0, 0, nrep, ram, supplied=ltc.alignments(case, inp))
        else:
            r = eng.null_intra(kind, ltc.null_seed(case), 0, nrep, ram)
        n = eng.null_pattern_count()
    finally:
        eng.set_null_patterns(None)
    want = ltc.distinct(ltc.alignments(case, inp)) if patterns else 2 * nrep * ram
    assert n == want, (case, inp, kind, patterns, n, want)
    if inp == ltc.FORCED and patterns:
        assert n == ltc.FORCED_PATTERNS == 171
    return r


def _tables(case, on, off):
    tree = case.split("-")[0]
    a, b = on.cherry_msg_info(), off.cherry_msg_info()
    assert b["tables"] == b["gathers"] == b["table_bytes"] == 0
    # (no tree holds more disjoint pairs of leaves than half its taxa, whatever nodes binarising adds)
    assert a["tables"] <= on.T // 2 and a["table_bytes"] == on.C * a["tables"] * 400 * 192 <= a["max_bytes"]
    assert a["gathers"] == 2 * a["tables"]
    if tree == "bal128":
        assert a["tables"] >= 60
    if tree in ("u65", "r65", "u66", "u131", "cat130"):
        assert a["tables"] >= 1
    return a["tables"]


@pytest.mark.parametrize("inp", ltc.INPUTS)
@pytest.mark.parametrize("case", ltc.PROTEIN_CASES + ltc.OTHER_PROTEIN_CASES)
def test_protein_null_with_and_without_table_and_patterns(case, inp):
    """every (table, patterns) combination: the same bytes in every output, and the oracle's values"""
    on, off = ltc.engine_of(case, True), ltc.engine_of(case, False)
    assert on.B == ltc.SIZES[case.split("-")[0]][0] and on.info()["device_states"] == 20
    _tables(case, on, off)
    for kind in ltc.null_kinds(case):
        ref = ltc.reference(case, inp, kind)
        res = {(table, patterns): _null(eng, case, inp, kind, patterns)
               for table, eng in ((True, on), (False, off)) for patterns in (True, False)}
        for (table, patterns), r in res.items():
            _same_bytes(res[(True, True)], r, (case, inp, kind, "table" if table else "no table", "patterns" if patterns else "per site"))
            _hold("protein %s, table %s" % ("patterns" if patterns else "per site", "on" if table else "off"), r, ref)


@pytest.mark.parametrize("inp", ltc.INPUTS)
@pytest.mark.parametrize("case", ltc.DNA_CASES)
def test_dna_null_per_site_and_forced_onto_patterns(case, inp):
    """16 and 20 class-fused device states with cherry tables; six classes, which the walk takes five at a time (two passes
    of 20 device states, the second padded); two classes, the unfused 4 states"""
    ncat = int(case.split("-")[1][1:])
    eng = ltc.engine_of(case)
    info = eng.info()
    fused = {4: 4, 5: 5, 6: 5, 2: 1}[ncat]                  # classes per pass (cmx_host_model.h: fuse)
    assert info["device_states"] == 4 * fused and info["device_classes"] == -(-ncat // fused)
    if ncat in (4, 5):
        assert info["device_states"] == 4 * ncat and info["cherry_tables"] > 0
    path = "%d fused states" % (4 * fused) if fused > 1 else "4 states unfused"
    for kind in ltc.null_kinds(case):
        ref = ltc.reference(case, inp, kind)
        per_site, patterns = _null(eng, case, inp, kind, False), _null(eng, case, inp, kind, True)
        _same_bytes(per_site, patterns, (case, inp, kind))
        _hold(path, patterns, ref)
    if inp != ltc.FORCED:        # left to itself a nucleotide model maps every site of every pair
        nrep, ram = ltc.shape_of(inp)
        default = eng.null_intra(0, ltc.null_seed(case), 0, nrep, ram)
        assert eng.null_pattern_count() == 2 * nrep * ram
        _same_bytes(default, _null(eng, case, inp, 0, False), (case, inp, "default"))


def _unfused_ref(stat):
    ref = ltc.unfused_mapped()
    return dict(stat=stat, nmin=ref["nmin"], prmin=ref["prmin"], rcmin=ref["rcmin"])


def test_unfused_null_mi_with_bounds():
    """simulate_kernel (rep_ram, gstep) -> map_sites -> the class words' MI and the diagonal kernel's minima"""
    eng, k = ltc.engine_of(ltc.UNFUSED_CASE), ltc.UNFUSED
    got = eng.null_intra(engine.STAT_DISCRETE_MI_BOUNDS, k["seed"], 0, k["nrep"], k["ram"], threshold=ltc.MI_BOUNDS)
    assert eng.null_pattern_count() == 2 * k["nrep"] * k["ram"]
    _hold("unfused null, MI(bounds)", got, _unfused_ref(ltc.stat_of(ltc.unfused_mapped(), oracle.ST_DISCRETE_MI, ltc.mi_params())))


def test_unfused_null_weighted_correlation():
    """uniform weights: the weighted Correlation is the unweighted one (w = 1 / B drops out of cov / sqrt(var var)), so
    oracle.null_intra's; other weights: the restatement of weighted_reference.pair_brute on the oracle's counts"""
    eng, k = ltc.engine_of(ltc.UNFUSED_CASE), ltc.UNFUSED
    ref = ltc.unfused_mapped()
    a, b = ref["counts"]
    try:
        eng.set_statistic_weights(np.ones(eng.B))
        got = eng.null_intra(engine.STAT_CORRELATION, k["seed"], 0, k["nrep"], k["ram"])
        assert eng.null_pattern_count() == 2 * k["nrep"] * k["ram"]
        _hold("unfused null, weights", got, _unfused_ref(ltc.stat_of(ref, oracle.ST_CORRELATION)))
        w = ltc.branch_weights(eng.B)
        eng.set_statistic_weights(w)
        got = eng.null_intra(engine.STAT_CORRELATION, k["seed"], 0, k["nrep"], k["ram"])
        wn = wr.normalise(w)
        st = np.array([wr.pair_brute(wr.CORRELATION, a[q], b[q], wn) for q in range(len(a))])
        _hold("unfused null, weights", got, _unfused_ref(st))
        plain = ltc.stat_of(ref, oracle.ST_CORRELATION)
        assert np.abs(st - plain).max() > 1e-3             # (these weights change the statistic)
    finally:
        eng.set_statistic_weights(None)


def test_inter_gene_null():
    """the second data set: the same tree with every branch 1.3 times as long, as tests/test_oracle_model_sets.py has it"""
    k = ltc.INTER
    e1, e2 = ltc.engine_of(ltc.UNFUSED_CASE), ltc.engine_of(ltc.UNFUSED_CASE, blen_scale=k["blen_scale"])
    o1, o2 = ltc.oracle_of(ltc.UNFUSED_CASE), ltc.oracle_of(ltc.UNFUSED_CASE, k["blen_scale"])
    for kind in (oracle.ST_CORRELATION, oracle.ST_COMPENSATION):
        got = e1.null_inter(e2, kind, k["seed"], k["rep_begin"], k["rep_end"], k["ram"])
        _hold("inter", got, oracle.null_inter(o1, o2, kind, k["seed"], k["rep_begin"], k["rep_end"], k["ram"]))


def test_continuous_rate_null():
    """oracle.simulate_continuous fed to the oracle's null as supplied alignments (test_continuous_rate_simulator_matches_oracle);
    and the device-resident null is the one assembled through host memory, bit for bit"""
    eng, om, k = ltc.engine_of(ltc.UNFUSED_CASE), ltc.oracle_of(ltc.UNFUSED_CASE), ltc.CONTINUOUS
    args = (engine.STAT_CORRELATION, k["seed"], k["rep_begin"], k["rep_end"], k["ram"], k["alpha"], k["p_inv"])
    got = eng.null_intra_continuous(*args)
    _same_bytes(got, eng.null_intra_continuous_via_host(*args), "via host")
    ref = ltc.compose(om, om, ltc.continuous_alignments())
    _hold("continuous", got, dict(stat=ltc.stat_of(ref, oracle.ST_CORRELATION), nmin=ref["nmin"], prmin=ref["prmin"], rcmin=ref["rcmin"]))


@pytest.mark.parametrize("case", ["u131-p4", "bal128-d4"])
def test_under_the_scratch_guard(case):
    """a canary behind every scratch buffer of a fresh engine: the pattern table, the packed columns and the per-pattern
    scalars of 259 branches and 131 taxa; the class-fused walk's buffers at 128"""
    was = engine.scratch_guard(True)
    try:
        engine.scratch_guard_failures(clear=True)
        eng = ltc.new_engine(case)
        for inp in ("3x53", ltc.FORCED):
            for kind in (0, 1):
                ref = ltc.reference(case, inp, kind)
                per_site, patterns = _null(eng, case, inp, kind, False), _null(eng, case, inp, kind, True)
                _same_bytes(per_site, patterns, (case, inp, kind))
                _hold("under the scratch guard", patterns, ref)
        eng.synchronize()
        eng.scratch_check()
        eng.close()
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
    finally:
        engine.scratch_guard(was)
