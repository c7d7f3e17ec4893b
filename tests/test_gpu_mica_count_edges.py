"""Mica's column mutual information for 4 and 20 states on the device against tests/golden/mica_counts.npz (the definition at
50 digits from exact counts), at the taxon counts where mica_path changes kernels and on the designed tables of
tests/mica_count_cases.py.  Reads the fixture and the case module; the bounds are the table of
tests/test_mica_count_edges.py (absolute, 10 x what the kernels' forms restated in fp64 numpy measure against the fixture on
the CPU, floor 1e-13, ceiling 1e-11), by the form the device evaluates for an entry:

    tab   the matrix-core kernels: pairs without a partial ambiguity code, up to 2 047 taxa
    def   the LDS-table kernel: pairs of a column with a partial code, every pair above 2 047 taxa, listed pairs
    h     the column entropies

Every line printed is  case  kernels  entry  form  largest error  bound."""
import numpy as np
import pytest

import mica_count_cases as mc
import test_mica_count_edges as cpu
from comap_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return engine.Engine()


@pytest.fixture(scope="module")
def fix():
    return cpu.load_fixture()


def _hold(name, what, got, ref, by_def, lim, q):
    """|got - ref| within the bound of the form that serves each entry; q: "mi" / "hj" """
    got, ref, by_def = np.asarray(got), np.asarray(ref), np.broadcast_to(by_def, np.shape(ref))
    assert got.shape == ref.shape and not np.isnan(got).any(), what
    err = np.abs(got - ref)
    kernels = cpu.path(mc.case(name)["A"], mc.case(name)["T"])
    for form, sel in (("tab", ~by_def), ("def", by_def)):
        if sel.any():
            print(f"{name} {kernels} {what}:{q} {form} {err[sel].max():.1e} {lim[f'{form}_{q}']:.1e}")
    assert (err[~by_def] <= lim[f"tab_{q}"]).all() and (err[by_def] <= lim[f"def_{q}"]).all(), (what, q, err.max())


def _hold_h(name, what, got, ref, lim):
    err = np.abs(np.asarray(got) - ref).max()
    print(f"{name} entropy {what} h {err:.1e} {lim['h']:.1e}")
    assert err <= lim["h"], (what, err)


@pytest.mark.parametrize("name", mc.CASES)
def test_columns_and_pairs_meet_the_fixture(eng, fix, name):
    c, r, lim = mc.case(name), mc.load(fix, name), cpu.bounds(name)
    A, T, a1, a2, masks, i1, i2 = c["A"], c["T"], c["a1"], c["a2"], c["masks"], c["i1"], c["i2"]
    n1, n2 = a1.shape[1], a2.shape[1]
    p1, p2 = mc.has_partial(a1, A), mc.has_partial(a2, A)
    tables = T > 2047
    rect_def = tables | p1[:, None] | p2[None, :]
    # the rectangle, twice, and transposed (the sides trade roles: registers against image, twelve columns against three)
    g = eng.mi_columns(a1, a2, A, masks=masks)
    for q, k in (("mi", "mi"), ("hj", "hjoint")):
        _hold(name, "rectangle", g[k], r[k], rect_def, lim, q)
    _hold_h(name, "h1", g["h1"], r["h1"], lim)
    _hold_h(name, "h2", g["h2"], r["h2"], lim)
    again = eng.mi_columns(a1, a2, A, masks=masks)
    for k in ("mi", "hjoint", "h1", "h2"):
        assert g[k].tobytes() == again[k].tobytes(), k
    gt = eng.mi_columns(a2, a1, A, masks=masks)
    for q, k in (("mi", "mi"), ("hj", "hjoint")):
        _hold(name, "transposed", gt[k], r[k].T, rect_def.T, lim, q)
    assert gt["h1"].tobytes() == g["h2"].tobytes() and gt["h2"].tobytes() == g["h1"].tobytes()
    # the first side against itself: j > i filled, NaN on and below the diagonal
    if n1 >= 2:
        gi = eng.mi_columns(a1, None, A, masks=masks)
        iu, il = np.triu_indices(n1, 1), np.tril_indices(n1)
        intra_def = (tables | p1[:, None] | p1[None, :])[iu]
        for q, k in (("mi", "mi"), ("hj", "hjoint")):
            assert np.isnan(gi[k][il]).all(), k
            _hold(name, "intra", gi[k][iu], r["i" + k][iu], intra_def, lim, q)
        assert gi["h1"].tobytes() == g["h1"].tobytes() and gi["h2"].tobytes() == g["h1"].tobytes()
        assert eng.mi_columns(a1, None, A, masks=masks)["mi"].tobytes() == gi["mi"].tobytes()
    # listed pairs (i = j, a pair twice, the designed ones), against the second side and against the first itself
    for second, pre in ((a2, "p"), (None, "q")):
        p = eng.mi_pairs(a1, i1, i2, second, A, masks=masks)
        for q, k in (("mi", "mi"), ("hj", "hjoint")):
            _hold(name, "pairs" if second is not None else "pairs-intra", p[k], r[pre + k], True, lim, q)
        same = eng.mi_pairs(a1, i1, i2, second, A, masks=masks)
        assert p["mi"].tobytes() == same["mi"].tobytes() and p["hjoint"].tobytes() == same["hjoint"].tobytes()
        assert p["mi"][1] == p["mi"][2] and p["hjoint"][1] == p["hjoint"][2]        # the pair listed twice
    # exact values
    idx1, idx2 = c["idx1"], c["idx2"]
    if c["kind"] == "grid":
        for key in ("const0", "constlast", "allunknown"):       # MI = 0 (the partial-code column's entry by the def bound)
            i, j = idx1[key], idx2[key]
            _hold(name, key, g["mi"][i, :], 0.0 * r["mi"][i, :], rect_def[i, :], lim, "mi")
            _hold(name, key, g["mi"][:, j], 0.0 * r["mi"][:, j], rect_def[:, j], lim, "mi")
        H = r["h1"][0]                                          # a copy and a state-permuted copy of column 0: MI = H
        for j in (idx2["copy"], idx2["permuted"]):
            _hold(name, "copy", g["mi"][0, j], H, tables, lim, "mi")
        for i in (idx1["copy"], idx1["permuted"]):
            _hold(name, "copy", gi["mi"][0, i], H, tables, lim, "mi")
        if "uniform" in idx1:                                   # all A^2 cells T / A^2: MI = 0, Hjoint = ln A^2
            i, j = idx1["uniform"], idx2["uniform"]
            _hold(name, "uniform", g["mi"][i, j], 0.0, tables, lim, "mi")
            _hold(name, "uniform", g["hjoint"][i, j], 2.0 * np.log(A), tables, lim, "hj")
    if c["kind"] == "dump16":                                   # all unknown x all unknown: MI = 0, Hjoint = ln 400
        _hold(name, "allunknown", g["mi"][3, 2], 0.0, False, lim, "mi")
        _hold(name, "allunknown", g["hjoint"][3, 2], 2.0 * np.log(A), False, lim, "hj")
