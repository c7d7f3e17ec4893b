"""Mica's column mutual information for 4 and 20 states against tests/golden/mica_counts.npz (the definition at 50 digits from
exact counts: tests/golden/make_mica_count_fixture.py, cases in tests/mica_count_cases.py).  No GPU.

Held to the fixture, as the largest ABSOLUTE error over a case's rectangle, its first side against itself and its listed pairs:

  * tab: the matrix-core kernels' documented counts-table form restated in fp64 numpy (mica_count_cases.table_form):
    MI = ln T + (sum f2[m] - S1 - S2) / T, Hjoint = ln T - sum f2[m] / T, tables of c ln c, sums in plain order;
    every pair without a partial ambiguity code;
  * def: the LDS-table kernel's form (mica_count_cases.definition_form: fractional counts, a logarithm per cell) -- what the
    device evaluates for the pairs of a column with a partial code, for every pair above 2 047 taxa and for listed pairs
    (mi_pairs_kernel).  A different but legitimate form, so it has its own columns, measured over those pairs.  Its tables
    are filled as the device fills them, 1 / (k1 k2) added taxon by taxon: two thousand adds of 1 / 400 drift by 1e-13,
    three times what the logarithms cost (with exact tables def:hj stays at 4e-14);
  * h: column_entropy_kernel's form (mica_count_cases.entropy_form);
  * oracle.mi_columns (C, fp64) and mica_wide_reference.mi_columns / mi_pairs (numpy; no mask table: the columns without a
    partial code): definition forms with their own order of operations, held to the def bound (h: the h bound); the
    oracle, which also adds every weight into both marginals, to its a-priori rounding bound where that is larger
    (oracle_accumulation).

Every bound asserted -- here and in tests/test_gpu_mica_count_edges.py, which reads this table -- is absolute and is
10 x the value measured here (x86-64 glibc), not less than 1e-13 and not more than 1e-11.  The margin covers the device's log
(1 - 2 ulp against glibc's) and another order of summation.  `python tests/test_mica_count_edges.py` prints the table anew;
test_forms_meet_the_fixture holds a new measurement to 10 x the committed one.

MEASURED
  case                  tab:mi    tab:hj    def:mi    def:hj         h
  a20-t1               3.1e-14   3.1e-14   3.3e-16   3.1e-14   0.0e+00
  a20-t2               3.2e-14   3.3e-14   6.1e-15   4.7e-14   4.4e-16
  a20-t33              1.7e-14   1.7e-14   6.2e-15   4.0e-14   1.3e-15
  a20-t64              1.2e-14   1.4e-14   3.6e-15   5.2e-14   2.2e-15
  a20-t65              1.2e-14   1.4e-14   5.8e-15   3.6e-14   3.1e-15
  a20-t128             1.2e-14   1.2e-14   4.9e-15   4.3e-14   4.0e-15
  a20-t129             1.2e-14   1.2e-14   6.2e-15   4.9e-14   5.8e-15
  a20-t256             2.3e-14   2.1e-14   4.9e-15   4.7e-14   8.4e-15
  a20-t257             2.2e-14   2.2e-14   4.9e-15   5.2e-14   8.0e-15
  a20-t400             2.4e-14   2.4e-14   1.1e-14   5.3e-14   1.6e-14
  a20-t512             2.3e-14   2.3e-14   1.4e-14   1.1e-13   1.8e-14
  a20-t513             2.3e-14   2.2e-14   1.3e-14   1.1e-13   1.9e-14
  a20-t2000            4.0e-14   3.9e-14   3.6e-14   1.4e-13   7.1e-14
  a20-t2047            3.7e-14   3.8e-14   3.6e-14   1.2e-13   7.1e-14
  a20-t2048            3.6e-14   3.8e-14   3.6e-14   1.2e-13   7.2e-14
  a20-t2049            3.8e-14   3.8e-14   3.6e-14   1.2e-13   7.3e-14
  a20-t33-one          2.2e-16   0.0e+00   4.4e-16   4.4e-16   1.3e-15
  a20-t33-two          1.8e-15   1.3e-15   1.6e-15   6.2e-15   1.3e-15
  a20-t300-one         1.9e-15   8.9e-16   3.3e-16   8.9e-16   1.3e-15
  a20-t300-two         4.0e-15   3.6e-15   3.3e-16   1.2e-14   1.3e-15
  a4-t1                0.0e+00   0.0e+00   2.7e-51   0.0e+00   0.0e+00
  a4-t2                6.7e-16   4.4e-16   8.3e-17   4.4e-16   0.0e+00
  a4-t33               1.1e-15   8.9e-16   2.2e-16   8.9e-16   2.2e-16
  a4-t64               2.0e-15   1.3e-15   2.2e-16   1.3e-15   2.2e-16
  a4-t65               2.1e-15   1.3e-15   2.2e-16   8.9e-16   2.2e-16
  a4-t128              1.9e-15   1.8e-15   2.2e-16   1.3e-15   2.2e-16
  a4-t129              2.1e-15   2.0e-15   2.2e-16   1.3e-15   2.2e-16
  a4-t256              3.1e-15   1.8e-15   8.3e-17   8.9e-16   2.2e-16
  a4-t257              2.5e-15   2.0e-15   2.2e-16   1.3e-15   2.2e-16
  a4-t512              2.4e-15   1.8e-15   4.4e-16   8.9e-16   2.2e-16
  a4-t2047             3.6e-15   2.4e-15   4.4e-16   8.9e-16   2.2e-16
  a4-t2048             3.2e-15   2.2e-15   2.2e-16   1.3e-15   2.2e-16
  a4-t2049             2.8e-15   2.7e-15   2.2e-16   1.3e-15   2.2e-16
  a4-t33-one           5.6e-17   0.0e+00   0.0e+00   0.0e+00   2.2e-16
  a4-t33-two           2.8e-16   4.4e-16   1.1e-16   4.4e-16   2.2e-16
  a4-t300-one          8.9e-16   8.9e-16   2.8e-17   4.4e-16   0.0e+00
  a4-t300-two          1.6e-15   2.2e-15   3.5e-17   4.4e-16   0.0e+00
  a20-t256-queue       2.1e-14   2.1e-14   1.3e-15   1.6e-14   8.9e-16
  a20-t512-queue       1.8e-14   1.9e-14   8.9e-16   2.0e-14   8.9e-16
  a20-t2047-dump16     7.3e-14   6.9e-14   3.6e-14   1.2e-13   7.1e-14
"""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":          # run as a script (below): the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
import mica_count_cases as mc
import mica_wide_reference as wide
from conftest import ROOT

FLOOR, CEILING = 1e-13, 1e-11
COLUMNS = ("tab_mi", "tab_hj", "def_mi", "def_hj", "h")


def bound(measured):
    return min(max(10.0 * measured, FLOOR), CEILING)


def _table():
    rows, on = {}, False
    for line in __doc__.splitlines():
        if line.strip() == "MEASURED":
            on = True
        elif on and not line.strip():
            break
        elif on and not line.lstrip().startswith("case"):
            f = line.split()
            rows[f[0]] = dict(zip(COLUMNS, (float(v) for v in f[1:])))
    return rows


def bounds(name):
    """{column: the bound asserted for this case}"""
    return {k: bound(v) for k, v in _table()[name].items()}


def load_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "mica_counts.npz"))


@pytest.fixture(scope="module")
def fix():
    return load_fixture()


def _err(a, ref):
    keep = ~np.isnan(a)
    return float(np.max(np.abs(a[keep] - ref[keep]))) if keep.any() else 0.0


def measure(c, r):
    """the five figures of a case"""
    A, a1, a2, i1, i2 = c["A"], c["a1"], c["a2"], c["i1"], c["i2"]
    out = {}
    rect, intra = mc.table_form(a1, a2, A), mc.table_form(a1, a1, A)
    for q, k in (("mi", "mi"), ("hj", "hjoint")):
        out[f"tab_{q}"] = max(_err(rect[k], r[k]), _err(intra[k], r["i" + k]), _err(rect[k][i1, i2], r["p" + k]),
                              _err(intra[k][i1, i2], r["q" + k]))
    # the definition form where the device evaluates it (filling its tables taxon by taxon is the slow part of this module):
    # every pair above 2 047 taxa; below, the pairs of a column with a partial code and the listed pairs
    p1, p2 = np.nonzero(mc.has_partial(a1, A))[0], np.nonzero(mc.has_partial(a2, A))[0]
    u1, v1 = np.unique(i1, return_inverse=True)
    u2, v2 = np.unique(i2, return_inverse=True)
    if c["T"] > 2047:
        p1, p2 = np.arange(a1.shape[1]), np.arange(0)
    parts = [(a1[:, p1], a2, lambda x: x[p1], ""), (a1, a2[:, p2], lambda x: x[:, p2], ""), (a1[:, p1], a1, lambda x: x[p1], "i"),
             (a1[:, u1], a2[:, u2], lambda x: x[np.ix_(u1, u2)], ""), (a1[:, u1], a1[:, u2], lambda x: x[np.ix_(u1, u2)], "i")]
    out["def_mi"] = out["def_hj"] = 0.0
    for b1, b2, take, pre in parts:
        if b1.shape[1] and b2.shape[1]:
            f = mc.definition_form(b1, b2, A)
            for q, k in (("mi", "mi"), ("hj", "hjoint")):
                out[f"def_{q}"] = max(out[f"def_{q}"], _err(f[k], take(r[pre + k])))
    assert np.array_equal(r["mi"][np.ix_(u1, u2)][v1, v2], r["pmi"]) and np.array_equal(r["imi"][np.ix_(u1, u2)][v1, v2], r["qmi"])
    out["h"] = max(_err(mc.entropy_form(a1, A), r["h1"]), _err(mc.entropy_form(a2, A), r["h2"]))
    return out


@pytest.mark.parametrize("name", mc.CASES)
def test_forms_meet_the_fixture(fix, name):
    c = mc.case(name)
    r = mc.load(fix, name)
    assert r["hash"] == mc.input_hash(c), "the fixture was made from other inputs: python tests/golden/make_mica_count_fixture.py"
    fig, lim = measure(c, r), bounds(name)
    print(name, " ".join(f"{fig[k]:.1e}" for k in COLUMNS))
    for k in COLUMNS:
        assert fig[k] <= lim[k], (k, fig[k], lim[k])


def oracle_accumulation(A, T):
    """orc_mi_columns adds the weight of every (taxon, a, b) into the cell AND into both marginals, so a marginal of a
    column of unknowns is the sum of A T terms (the LDS-table kernel sums its marginals from the finished table: A terms).
    Each add rounds by at most eps / 2 of the running sum; MI = sum p_ab ln(p_ab / (p_a p_b)) moves by at most
    sum p_ab = 1 per unit of relative error in the marginals and by MI + 1 <= ln A + 1 per unit in the cells:
    (2 A T + (ln A + 1) T) eps / 2 <= (A + 2) T eps, a priori.  The oracle is held to this where it is above the def bound
    (measured: 1.4e-13 at 400 taxa against 1.9e-12), never above the ceiling."""
    return min((A + 2) * T * np.finfo(np.float64).eps, CEILING)


@pytest.mark.parametrize("name", mc.CASES)
def test_oracle_and_restatement_meet_the_fixture(fix, name):
    c = mc.case(name)
    r = mc.load(fix, name)
    A, a1, a2, i1, i2 = c["A"], c["a1"], c["a2"], c["i1"], c["i2"]
    lim = bounds(name)
    table = mc.mask_table(A)
    o, oi = oracle.mi_columns(a1, a2, A, table), oracle.mi_columns(a1, a1, A, table)
    fig = dict(mi=max(_err(o["mi"], r["mi"]), _err(oi["mi"], r["imi"])), hj=max(_err(o["hjoint"], r["hjoint"]), _err(oi["hjoint"], r["ihjoint"])),
               h=max(_err(o["h1"], r["h1"]), _err(o["h2"], r["h2"])))
    print(name, "oracle", " ".join(f"{v:.1e}" for v in fig.values()))
    seq = oracle_accumulation(A, c["T"])
    assert fig["mi"] <= max(lim["def_mi"], seq) and fig["hj"] <= max(lim["def_hj"], seq) and fig["h"] <= max(lim["h"], seq), fig
    # the numpy restatement knows no mask table: the columns without a partial code
    k1, k2 = np.nonzero(~mc.has_partial(a1, A))[0], np.nonzero(~mc.has_partial(a2, A))[0]
    w, wi = wide.mi_columns(a1[:, k1], a2[:, k2], A), wide.mi_columns(a1[:, k1], None, A)
    fig = dict(mi=max(_err(w["mi"], r["mi"][np.ix_(k1, k2)]), _err(wi["mi"], r["imi"][np.ix_(k1, k1)])),
               hj=max(_err(w["hjoint"], r["hjoint"][np.ix_(k1, k2)]), _err(wi["hjoint"], r["ihjoint"][np.ix_(k1, k1)])),
               h=max(_err(w["h1"], r["h1"][k1]), _err(w["h2"], r["h2"][k2]), _err(wide.entropy(a1[:, k1], A), r["h1"][k1])))
    ok = ~(mc.has_partial(a1, A)[i1] | mc.has_partial(a2, A)[i2])
    if ok.any():
        p = wide.mi_pairs(a1, i1[ok], i2[ok], A, a2)
        fig["mi"], fig["hj"] = max(fig["mi"], _err(p["mi"], r["pmi"][ok])), max(fig["hj"], _err(p["hjoint"], r["phjoint"][ok]))
    print(name, "restatement", " ".join(f"{v:.1e}" for v in fig.values()))
    assert fig["mi"] <= lim["def_mi"] and fig["hj"] <= lim["def_hj"] and fig["h"] <= lim["h"], fig


# ------------------------------------------------------------------------------------------------ what the cases reach
def path(A, T):
    """mica_path (cmx_mica.hip) for these column counts, and the four-wave kernels' k-steps (m4_ksteps)"""
    if T > 2047:
        return "tables"
    Tp = (T + 31) // 32 * 32
    ks = 2 if Tp <= 64 else 4 if Tp <= 128 else 8 if Tp <= 256 else 16
    if A == 20:
        return f"four-wave/{ks}" if Tp <= 512 else "eight-wave"
    return f"four-wave/{ks}" if Tp <= 256 else "one-column"


def test_every_row_and_every_boundary_is_a_case():
    rows = {20: ["four-wave/2", "four-wave/4", "four-wave/8", "four-wave/16", "eight-wave", "tables"],
            4: ["four-wave/2", "four-wave/4", "four-wave/8", "one-column", "tables"]}
    edges = {20: [(64, 65), (128, 129), (256, 257), (512, 513), (2047, 2048)], 4: [(64, 65), (128, 129), (256, 257), (2047, 2048)]}
    for A in (20, 4):
        taxa = [mc.case(n)["T"] for n in mc.CASES if n.startswith(f"a{A}-") and mc.case(n)["kind"] == "grid"]
        assert taxa == mc.TAXA[A] and {1, 2, 2049} <= set(taxa)
        assert [p for k, p in enumerate(path(A, T) for T in taxa) if k == 0 or p != path(A, taxa[k - 1])] == rows[A]
        for lo, hi in edges[A]:
            assert lo in taxa and hi in taxa and path(A, lo) != path(A, hi)
        for T in taxa:       # column counts that fill no tile: 12 x 3 (proteins), 64 x 16 (nucleotides), 12 x 6, 8 x 4
            n1, n2 = mc.case(f"a{A}-t{T}")["a1"].shape[1], mc.case(f"a{A}-t{T}")["a2"].shape[1]
            assert 26 <= n1 <= 40 and n1 % 12 and 7 <= n2 <= 20 and n2 % (3 if A == 20 else 16)
    assert path(20, 256) == "four-wave/8" and path(20, 512) == "four-wave/16" and path(20, 2047) == "eight-wave"


def test_grid_columns_are_what_they_are_called(fix):
    for name in mc.CASES:
        c = mc.case(name)
        if c["kind"] != "grid":
            continue
        A, T, r = c["A"], c["T"], mc.load(fix, name)
        k, _ = mc.popcounts(A)
        for side, h in (("1", r["h1"]), ("2", r["h2"])):
            aln, idx = c["a" + side], c["idx" + side]
            unknown = k[aln] == A
            assert (aln[:, idx["const0"]] == 0).all() and (aln[:, idx["constlast"]] == A - 1).all()
            assert unknown[:, idx["allunknown"]].all() and unknown[:, idx["oneunknown"]].sum() == 1
            assert unknown[:, idx["allbutone"]].sum() == T - 1 and np.bincount(aln[:, idx["split"]]).max() == max(T - 1, 1)
            if T >= 33:      # columns that mix states and unknowns, both unknown codes
                assert (unknown.any(axis=0) & ~unknown.all(axis=0)).sum() >= 3 and (aln == mc.FAR).any() and (aln == A).any()
            assert mc.has_partial(aln, A).sum() == 1 and mc.has_partial(aln, A)[idx["partial"]]
            assert abs(h[idx["const0"]]) < 1e-30 and abs(h[idx["allunknown"]] - np.log(A)) < 1e-15
        i0 = c["idx1"]["copy"], c["idx1"]["permuted"]
        j0 = c["idx2"]["copy"], c["idx2"]["permuted"]
        for j in j0:         # a copy and a state-permuted copy: MI = H = Hjoint
            assert abs(r["mi"][0, j] - r["h1"][0]) < 1e-15 and abs(r["hjoint"][0, j] - r["h1"][0]) < 1e-15
        for i in i0:
            assert abs(r["imi"][0, i] - r["h1"][0]) < 1e-15
        for key in ("const0", "constlast", "allunknown"):
            assert np.abs(r["mi"][c["idx1"][key], :]).max() < 1e-30 and np.abs(r["mi"][:, c["idx2"][key]]).max() < 1e-30
        assert ("uniform" in c["idx1"]) == (T in mc.UNIFORM[A])
        if "uniform" in c["idx1"]:
            i, j = c["idx1"]["uniform"], c["idx2"]["uniform"]
            N = mc.pseudo_counts(c["a1"][:, [i]], c["a2"][:, [j]], A)[0, 0]
            assert (N[:A, :A] == T // (A * A)).all() and N[:A, :A].sum() == T
            assert abs(r["mi"][i, j]) < 1e-30 and abs(r["hjoint"][i, j] - 2 * np.log(A)) < 1e-15
    assert [n for n in mc.CASES if "uniform" in mc.case(n)["idx1"]] == ["a20-t400", "a20-t2000", "a4-t256", "a4-t512"]


@pytest.mark.parametrize("T", [256, 512])
def test_queue_case_fills_the_queue_and_splits_f2(T):
    c = mc.case(f"a20-t{T}-queue")
    blocks, cap = mc.QUEUE_BLOCKS[T], {256: 232, 512: 464}[T]          # m4_qcap (cmx_mica4.hip)
    assert path(20, T) == f"four-wave/{8 if T == 256 else 16}" and 9 * blocks == {256: 207, 512: 414}[T] <= cap
    for a1, a2 in ((c["a1"], c["a2"]), (c["a2"], c["a1"])):
        m = mc.weighted_cells(mc.pseudo_counts(a1, a2, 20), 20)
        big = (m >= mc.kMicaLdsF2).sum(axis=(2, 3))
        full = [(b, t) for b, t, weighted in mc.four_wave_layout(a1, a2, 20) if weighted and len(b) == 3 and len(t) == 3
                and (big[np.ix_(b, t)] == blocks).all() and (m[np.ix_(b, t)] % 400 == 0).all()]
        assert full, "no wave whose nine pairs of whole counts queue 23 (46) cells each in a tile of the weighted instantiation"
        assert big.max() == blocks          # and no pair beyond what the queue was sized for
    N = mc.pseudo_counts(c["a1"], c["a2"], 20)
    m = mc.weighted_cells(N, 20)
    for k, (i, j) in enumerate(c["f2_pairs"]):
        assert N[i, j, 0, 0] == 10 and N[i, j, 0, 20] + N[i, j, 20, 0] == 4 and N[i, j, 20, 20] == 15 + k
        assert m[i, j, 0, 0] == mc.F2_CELLS[k] and (i, j) in zip(c["i1"], c["i2"])
    assert mc.F2_CELLS == (4095, 4096, 4097)


def test_dump16_case_holds_the_largest_counts():
    c = mc.case("a20-t2047-dump16")
    A, T = 20, 2047
    assert path(A, T) == "eight-wave"
    N = mc.pseudo_counts(c["a1"], c["a2"], A)
    m = mc.weighted_cells(N, A)
    assert N[0, 0, 0, 0] == T - 1 and N[0, 0, A, A] == 1 and m[0, 0, 0, 0] == 400 * (T - 1) + 1
    assert N[1, 0, 0, 0] == T - 2 and N[1, 0, 0, A] == 1 and N[1, 0, A, 0] == 1 and m[1, 0, 0, 0] == 400 * (T - 2) + 40
    assert N[3, 2, A, A] == T and (m[3, 2] == T).all()
    assert N.max() == T < 1 << 16


# ------------------------------------------------------------------------------------------------ what the bound is for
def _rect_errors(c, r, **kw):
    f = mc.table_form(c["a1"], c["a2"], c["A"], **kw)
    return _err(f["mi"], r["mi"]), _err(f["hjoint"], r["hjoint"])


@pytest.mark.parametrize("A", [20, 4])
def test_the_bound_tells_a_wrong_table_from_a_right_one(fix, A):
    """Three ways in which a count-table kernel can be subtly wrong, each applied to the restated form: a cell of m >= 4 096
    reads f2[m + 1]; the tables of c ln c rounded through fp32; one taxon (the first of the second k-step) dropped from the
    counts.  Each leaves a case outside the bound that the right form meets."""
    names = [f"a{A}-t65", f"a{A}-t256", f"a{A}-t257", f"a{A}-t512"]
    outside = {"neighbour": [], "fp32": [], "taxon": []}
    for name in names:
        c, r, lim = mc.case(name), mc.load(fix, name), bounds(name)
        T = c["T"]
        right = _rect_errors(c, r)
        assert right[0] <= lim["tab_mi"] and right[1] <= lim["tab_hj"]
        keep = np.arange(T) != 32
        wrong = {"neighbour": _rect_errors(c, r, bump=True),
                 "fp32": _rect_errors(c, r, f2=mc.f2_table(A, T).astype(np.float32).astype(np.float64)),
                 "taxon": _rect_errors(dict(c, a1=c["a1"][keep], a2=c["a2"][keep]), r, T=T)}
        for k, (emi, ehj) in wrong.items():
            if emi > lim["tab_mi"] or ehj > lim["tab_hj"]:
                outside[k].append(name)
    print(A, outside)
    assert all(outside.values()), outside
    # the bar of the older tests (rel 1e-6 + abs 1e-10) lets the rounded tables pass
    c, r = mc.case(names[1]), mc.load(fix, names[1])
    emi, _ = _rect_errors(c, r, f2=mc.f2_table(A, c["T"]).astype(np.float32).astype(np.float64))
    assert FLOOR < emi < 1e-6


if __name__ == "__main__":          # the table of the docstring, measured anew
    f = load_fixture()
    print("MEASURED\n  case                  tab:mi    tab:hj    def:mi    def:hj         h")
    for name in mc.CASES:
        fig = measure(mc.case(name), mc.load(f, name))
        print(f"  {name:18s} " + " ".join(f"{fig[k]:9.1e}" for k in COLUMNS))
        sys.stdout.flush()
