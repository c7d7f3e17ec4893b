"""The null over supplied alignments against 50-digit answers, on the CPU: oracle.null_intra (decomposition, and
uniformization where its series runs) against null_walk_cases.expected for every case of tests/golden/operator_edges.npz and
tests/golden/null_walk_edges.npz with 4 or 20 states; the evidence that the bars of tests/null_walk_cases.py are neither
tighter than the counts' own bar allows nor more than two orders looser; the left-out conditions; and the host plan of the
12-leaf tree's walks.  No GPU.  tests/test_gpu_null_walk_edges.py holds every device path of the null to the same answers at
the same bars.

The rows of the 12-leaf tree's cases (operator_edge_cases.DEEP_CASES), measured as test_operator_edges measures its own:
oracle.map_sites against the fixture, counts as the smallest rtol beside the absolute term, logL and post_rate relative.
Every bound asserted is test_operator_edges.bound() of the row (10 x, floor 1e-13, ceiling 1e-8); the rows give the cases
their e.  `python tests/test_null_walk_reference.py` prints both tables anew (x86-64 glibc).

MEASURED-CASES
  case                          counts:unif  decomp     logL  post_rate
  protein-g4-t12-q1               6.8e-13   6.9e-13   4.0e-14   4.0e-13
  protein-g4-t12-q2               1.1e-10   4.9e-13   4.0e-14   4.1e-13
  protein-g4-t12-q3               1.5e-12   1.5e-12   1.2e-13   1.0e-12
  protein-g4-t12-q4                     -   2.7e-12   1.4e-13   1.6e-12
  protein-ig5-t12-q1              9.5e-13   9.2e-13   7.7e-14   6.7e-13
  protein-ig5-t12-q2              1.1e-10   1.3e-12   7.7e-14   9.5e-13
  jc20-g4-t12-q2                  6.7e-11   4.4e-12   1.4e-13   1.9e-12
  protein_k2-g4-t12-q2            1.1e-10   5.8e-13   4.6e-14   4.8e-13
  protein_signed-g4-t12-q1        1.9e-12   1.9e-12   1.3e-13   8.7e-13
  dna-g4-t12-q1                   9.8e-15   8.4e-15   6.0e-15   1.2e-14
  dna-g4-t12-q2                   8.6e-11   4.2e-14   3.6e-15   3.8e-14
  dna-g4-t12-q3                   3.5e-14   3.4e-14   6.1e-15   2.7e-14
  dna-g4-t12-q4                         -   8.0e-13   8.5e-14   3.9e-13
  dna-ig5-t12-q1                  9.8e-15   9.6e-15   3.9e-15   6.0e-15
  dna-ig5-t12-q2                  8.5e-11   3.3e-14   2.8e-15   2.8e-14
  dna-c1-t12-q1                   8.0e-14   7.8e-14   4.8e-15   0.0e+00
  dna-c1-t12-q2                   1.9e-11   6.7e-14   4.1e-15   0.0e+00
  jc4-g4-t12-q2                   6.7e-11   3.0e-14   3.1e-15   2.7e-14

MEASURED-NULL (error / bar; decomposition, and the largest of the row under uniformization; - = not run)
  case                            nmin    prmin      cor     comp      cos      cov      euc       mi     unif
  dna-g4-t4-p1                  1.2e-05  1.0e-02  1.6e-07  1.5e-07  1.5e-07  3.0e-06  4.0e-06  0.0e+00  1.0e-02
  dna-g4-t4-p2                  1.2e-05  9.6e-03  1.7e-07  1.5e-07  1.5e-07  2.6e-06  4.0e-06  0.0e+00  9.6e-03
  dna-g4-t4-p3                  3.0e-05  2.3e-02  2.7e-07  2.6e-07  3.6e-07  8.3e-06  9.8e-06  0.0e+00  2.3e-02
  dna-g4-t4-p4                  1.6e-02  1.1e-04  0.0e+00  0.0e+00  0.0e+00  0.0e+00  0.0e+00  0.0e+00  2.9e-03
  dna-g4-t4-p5                  9.3e-06  7.6e-03  2.3e-07  1.5e-07  2.0e-07  2.8e-06  3.0e-06  0.0e+00  7.6e-03
  dna-g4-t4-p6                  2.1e-05  2.1e-02  7.5e-08  1.5e-07  7.4e-08  5.7e-06  1.6e-06  0.0e+00  7.9e-02
  dna-g4-t4-p7                  6.7e-04  9.6e-02  6.8e-08  1.5e-07  7.4e-08  2.1e-04  6.0e-05  0.0e+00        -
  dna-g4-t4-p8                  1.1e-05  1.2e-02  1.2e-07  1.5e-07  7.4e-08  3.3e-06  2.3e-06  0.0e+00  6.0e-02
  dna-ig5-t5-p1                 1.2e-05  9.1e-03  9.4e-07  3.0e-07  7.0e-07  3.2e-06  3.7e-06  0.0e+00  9.1e-03
  dna-ig5-t5-p2                 1.7e-05  1.4e-02  1.6e-07  2.2e-07  1.9e-07  4.4e-06  5.6e-06  0.0e+00  1.4e-02
  dna-ig5-t5-p6                 2.6e-05  2.6e-02  9.4e-08  1.5e-07  7.4e-08  7.3e-06  5.7e-06  0.0e+00  8.3e-02
  dna-ig5-t5-p7                 7.6e-04  1.0e-01  8.6e-08  1.9e-07  7.4e-08  2.3e-04  1.3e-04  0.0e+00        -
  dna-c1-t4-p1                  5.4e-06  0.0e+00  6.3e-07  2.2e-07  4.4e-07  1.5e-06  1.7e-06  0.0e+00  5.9e-06
  dna-c1-t4-p3                  8.4e-06  0.0e+00  6.1e-07  2.6e-07  5.4e-07  2.6e-06  2.7e-06  0.0e+00  8.4e-06
  dna-c1-t4-p6                  6.7e-07  0.0e+00  9.1e-08  1.5e-07  7.4e-08  2.3e-07  1.1e-07  0.0e+00  1.9e-02
  jc4-g4-t4-p1                  1.0e-05  7.0e-03  6.9e-07  2.2e-07  4.3e-07  2.9e-06  3.2e-06  0.0e+00  7.0e-03
  jc4-g4-t4-p6                  1.9e-05  1.9e-02  7.5e-08  1.5e-07  7.4e-08  5.2e-06  1.4e-06  0.0e+00  6.0e-02
  jcp4-g4-t4-p1                 2.9e-05  2.4e-02  2.7e-07  1.5e-07  1.7e-07  6.1e-06  9.5e-06  0.0e+00  2.4e-02
  jcp4-g4-t4-p6                 1.6e-05  1.6e-02  7.5e-08  1.5e-07  7.4e-08  4.3e-06  1.3e-06  0.0e+00  6.0e-02
  protein-g4-t5-p1              2.2e-04  1.0e-01  4.5e-06  3.4e-06  3.5e-06  6.7e-05  7.5e-05  0.0e+00  1.0e-01
  protein-g4-t5-p2              2.6e-04  1.0e-01  7.3e-06  4.5e-06  5.3e-06  7.9e-05  8.6e-05  0.0e+00  1.0e-01
  protein-g4-t5-p3              8.3e-05  7.1e-02  1.4e-06  1.5e-06  1.2e-06  2.5e-05  2.8e-05  0.0e+00  7.1e-02
  protein-g4-t5-p4              8.0e-03  8.9e-04  0.0e+00  0.0e+00  0.0e+00  0.0e+00  0.0e+00  0.0e+00  8.9e-04
  protein-g4-t5-p5              5.8e-04  1.0e-01  2.2e-06  7.1e-06  1.6e-06  1.7e-04  1.9e-04  0.0e+00  1.0e-01
  protein-g4-t5-p6              5.3e-05  4.9e-02  1.1e-07  1.5e-07  7.4e-08  1.5e-05  1.4e-05  0.0e+00  1.1e-01
  protein-g4-t5-p7              3.9e-04  1.0e-01  1.2e-07  1.5e-07  7.4e-08  1.2e-04  8.2e-05  0.0e+00        -
  protein-g4-t5-p8              8.7e-05  7.6e-02  1.0e-07  1.5e-07  9.2e-08  2.7e-05  2.3e-05  0.0e+00  9.4e-02
  protein-ig5-t4-p2             2.8e-04  1.0e-01  7.2e-07  5.8e-06  5.7e-07  8.4e-05  9.3e-05  0.0e+00  1.0e-01
  protein-ig5-t4-p6             2.2e-04  1.0e-01  7.5e-08  1.5e-07  7.4e-08  6.0e-05  7.3e-05  0.0e+00  1.0e-01
  protein-c1-t4-p7              4.7e-06  0.0e+00  8.4e-08  1.5e-07  7.4e-08  1.5e-06  2.7e-07  0.0e+00        -
  jc20-g4-t4-p1                 2.5e-03  1.0e-01  9.4e-05  4.6e-05  7.5e-05  6.8e-04  8.4e-04  0.0e+00  1.0e-01
  jc20-g4-t4-p6                 4.3e-04  1.0e-01  9.1e-08  1.1e-07  7.4e-08  1.2e-04  1.1e-04  0.0e+00  1.0e-01
  jcp20-g4-t4-p1                2.9e-03  9.9e-02  3.4e-05  2.5e-05  2.4e-05  8.7e-04  9.5e-04  0.0e+00  9.9e-02
  jcp20-g4-t4-p6                8.0e-04  1.0e-01  7.6e-08  1.5e-07  1.1e-07  2.2e-04  2.1e-04  0.0e+00  1.0e-01
  protein_k2-g4-t4-p6           6.3e-05  5.9e-02  7.5e-08  1.5e-07  9.2e-08  1.7e-05  1.6e-05  0.0e+00  1.0e-01
  protein_signed-g4-t4-p1       1.9e-04  6.1e-02  1.5e-06  1.1e-05  1.4e-06  5.8e-05  6.3e-05  0.0e+00  6.1e-02
  protein_signed-g4-t4-p6       3.6e-05  7.7e-02  5.8e-06  1.0e-05  8.0e-06  1.2e-05  8.5e-06  0.0e+00  7.7e-02
  protein-g4-t12-q1             5.6e-04  1.0e-01  1.2e-05  1.5e-05  1.1e-05  1.8e-04  1.6e-04  0.0e+00  1.0e-01
  protein-g4-t12-q2             4.0e-04  1.0e-01  1.1e-07  1.5e-07  9.2e-08  1.3e-04  9.9e-05  0.0e+00  1.1e-01
  protein-g4-t12-q3             1.5e-03  1.0e-01  5.1e-06  3.9e-05  4.4e-06  4.9e-04  5.1e-04  0.0e+00  1.0e-01
  protein-g4-t12-q4             1.6e-03  1.0e-01  1.8e-07  1.5e-07  7.4e-08  5.2e-04  4.0e-04  0.0e+00        -
  protein-ig5-t12-q1            9.5e-04  1.0e-01  1.9e-06  2.9e-05  1.5e-06  3.1e-04  3.2e-04  0.0e+00  1.0e-01
  protein-ig5-t12-q2            9.5e-04  1.0e-01  1.1e-07  1.5e-07  9.2e-08  3.0e-04  3.2e-04  0.0e+00  1.1e-01
  jc20-g4-t12-q2                1.9e-03  1.0e-01  1.2e-07  1.5e-07  7.4e-08  6.0e-04  4.7e-04  0.0e+00  1.0e-01
  protein_k2-g4-t12-q2          4.7e-04  1.0e-01  1.4e-07  1.5e-07  7.4e-08  1.5e-04  1.3e-04  0.0e+00  1.1e-01
  protein_signed-g4-t12-q1      1.7e-03  1.0e-01  3.4e-05  5.5e-05  3.5e-05  5.4e-04  5.5e-04  0.0e+00  1.0e-01
  dna-g4-t12-q1                 1.0e-05  1.2e-02  6.5e-07  2.2e-07  5.4e-07  1.9e-06  3.5e-06  0.0e+00  1.2e-02
  dna-g4-t12-q2                 3.8e-05  3.8e-02  1.1e-07  1.9e-07  7.4e-08  1.2e-05  1.2e-05  0.0e+00  8.6e-02
  dna-g4-t12-q3                 3.9e-05  2.7e-02  1.3e-07  8.5e-07  1.7e-07  1.2e-05  1.3e-05  0.0e+00  2.7e-02
  dna-g4-t12-q4                 3.9e-04  1.0e-01  2.2e-07  1.1e-07  7.4e-08  1.3e-04  1.2e-04  0.0e+00        -
  dna-ig5-t12-q1                7.7e-06  6.0e-03  2.7e-07  3.0e-07  2.9e-07  2.5e-06  2.6e-06  0.0e+00  6.0e-03
  dna-ig5-t12-q2                2.7e-05  2.8e-02  1.4e-07  1.5e-07  7.4e-08  8.6e-06  8.5e-06  0.0e+00  8.5e-02
  dna-c1-t12-q1                 3.5e-05  0.0e+00  1.8e-06  1.1e-06  2.2e-06  1.1e-05  6.3e-06  0.0e+00  3.6e-05
  dna-c1-t12-q2                 1.1e-06  0.0e+00  1.1e-07  1.5e-07  5.6e-08  2.8e-07  5.0e-08  0.0e+00  1.9e-02
  jc4-g4-t12-q2                 2.7e-05  2.7e-02  1.2e-07  1.5e-07  7.4e-08  8.5e-06  6.4e-06  0.0e+00  6.7e-02
"""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

if __name__ == "__main__":          # run as a script (below): the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
import null_walk_cases as nw
import operator_edge_cases as oe
import pair_stat_cases as pc
import test_operator_edges as cpu
from comap_amd import engine
from conftest import ROOT

NULL_COLUMNS = ("nmin", "prmin", 0, 1, 3, 4, 7, 5)       # the columns of MEASURED-NULL (Cosubstitution: equal or not)
ALL_CASES = list(oe.CASES) + list(oe.DEEP_CASES)
WALK_CASES = [n for n in ALL_CASES if oe.Inputs(n).S in (4, 20)]


def _table(title):
    """rows of this module's docstring table whose heading starts with `title`: {first column: [floats]} ('-': None)"""
    rows, on = {}, False
    for line in __doc__.splitlines():
        if line.strip().startswith(title):
            on = True
        elif on and not line.strip():
            break
        elif on and not line.lstrip().startswith("case"):
            f = line.split()
            rows[f[0]] = [None if v == "-" else float(v) for v in f[1:]]
    return rows


@lru_cache(maxsize=None)
def rows():
    """MEASURED-CASES of every case of both fixtures"""
    return {**cpu._table("MEASURED-CASES"), **_table("MEASURED-CASES")}


@lru_cache(maxsize=None)
def fixtures():
    return np.load(os.path.join(ROOT, "tests", "golden", "operator_edges.npz")), nw.deep_fixture()


@lru_cache(maxsize=None)
def case(name):
    return oe.load(fixtures()[name in oe.DEEP_CASES], name)


@lru_cache(maxsize=None)
def pairs(name):
    c = case(name)
    return nw.supplied_pairs(c["aln"], len(c["pi"]))


@lru_cache(maxsize=None)
def expected(name, kind):
    _, i0, i1 = pairs(name)
    return nw.expected(case(name), i0, i1, kind, row=rows()[name])


def _unif_runs(name):
    return cpu._unif_runs(name)


def null_figures(name, method, row=None):
    """oracle.null_intra over the supplied pairs of the case under `method` -> {column of MEASURED-NULL: error / bar}"""
    c = case(name)
    sup, i0, i1 = pairs(name)
    m = oracle.Model(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"], Bk=oe.register_of(c),
                     method=method, nonneg=bool(c["clamp"]))
    out = {"nmin": 0.0, "prmin": 0.0}
    for kind in nw.KINDS:
        exp = expected(name, kind) if row is None else nw.expected(c, i0, i1, kind, row=row)
        with np.errstate(all="ignore"):
            got = oracle.null_intra(m, kind, 0, 0, 3, sup.shape[3], supplied=sup, params=oracle.stat_params(kind, nw.MI_THRESHOLD))
        fig = nw.figures(got, exp, name)
        assert fig["rcmin"] == 0.0, (name, kind)
        assert nw.leaves_out(name, kind) or fig["left_out"] == 0, (name, kind)
        assert fig["compared"] > 0 or not nw.compares_stat(name), (name, kind)
        out["nmin"], out["prmin"] = max(out["nmin"], fig["nmin"]), max(out["prmin"], fig["prmin"])
        out[kind] = fig["stat"]
    return out


# ------------------------------------------------------------------------------------------------ the new fixture
def test_deep_fixture_inputs_are_the_cases():
    fix = fixtures()[1]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "null_walk_edges.npz")) < 400 * 1024
    stored = {"parent", "blen", "lot", "Q", "pi", "rates", "probs", "aln", "classes", "Bk", "clamp", "counts", "logL",
              "post_rate", "rate_class", "class_clear"}
    assert sorted({k.split(".")[0] for k in fix.files}) == sorted(oe.DEEP_CASES)
    for name in oe.DEEP_CASES:
        c, i = oe.load(fix, name), oe.Inputs(name)
        assert set(c) == stored, name                   # no operators, none of the other nijt options
        aln, cls = i.draw()
        assert np.array_equal(c["aln"], aln) and np.array_equal(c["classes"], cls)
        assert np.array_equal(c["blen"], i.blen) and np.array_equal(c["Q"], i.Q) and np.array_equal(c["rates"], i.rates)
        assert np.array_equal(c["parent"], i.parent) and np.array_equal(c["lot"], i.lot)
        assert aln.shape == (12, oe.DEEP_NSITES) and (aln < i.S).all()
        assert c["counts"].shape == (oe.DEEP_NSITES, 21, 1 if i.Bk is None else len(i.Bk))
        assert np.isfinite(c["logL"]).all() and np.isfinite(c["counts"]).all()
        assert (c["counts"][:, i.blen[:-1] == 0.0] == 0.0).all()
        assert 0.05 <= oe.TREES["t12"][1][:-1].min() and oe.TREES["t12"][1][:-1].max() <= 0.4


DEEP_PARAMS = [(n, m) for n in oe.DEEP_CASES for m in cpu.METHODS if m == "decomp" or _unif_runs(n)]
assert [n for n in oe.DEEP_CASES if not _unif_runs(n)] == [n for n in oe.DEEP_CASES if n.endswith("q4")]


@pytest.mark.parametrize("name,method", DEEP_PARAMS)
def test_oracle_mapping_meets_the_deep_fixture(name, method):
    row = _table("MEASURED-CASES")[name]
    counts, logl, prate, classes = cpu.measure_case(case(name), cpu.METHODS[method])
    print(f"{name} {method}: counts {counts:.1e} logL {logl:.1e} post_rate {prate:.1e}")
    assert counts <= cpu.bound(max(v for v in row[:2] if v is not None)), counts
    assert logl <= cpu.bound(row[2]) and prate <= cpu.bound(row[3])
    assert classes


# ------------------------------------------------------------------------------------------------ the supplied pairs
def test_supplied_pairs_are_what_the_walks_need():
    """66 resolved columns of the 70 (198 pairs: six full 64-site blocks of columns and a partial one, 16-site tiles with a
    partial one), all 45 of the 12-leaf tree's (135 pairs)"""
    for name, n in (("protein-g4-t5-p2", 66), ("dna-g4-t4-p1", 66), ("protein-g4-t12-q1", 45)):
        c = case(name)
        sup, i0, i1 = pairs(name)
        assert sup.shape == (3, 2, len(c["lot"]), n) and sup.dtype == np.uint8 and (sup < len(c["pi"])).all()
        assert len(i0) == len(i1) == 3 * n
        assert np.array_equal(sup[:, 0].transpose(1, 0, 2).reshape(len(c["lot"]), -1), c["aln"][:, i0])
        assert np.array_equal(sup[:, 1].transpose(1, 0, 2).reshape(len(c["lot"]), -1), c["aln"][:, i1])
        res = np.flatnonzero((c["aln"] < len(c["pi"])).all(axis=0))
        assert np.array_equal(i0[:n], res) and np.array_equal(i1[:n], np.roll(res, 1))
        assert np.array_equal(i0[n:2 * n], res[::-1]) and np.array_equal(i1[n:2 * n], np.roll(res[::-1], 7))
        assert np.array_equal(i0[2 * n:], res) and np.array_equal(i1[2 * n:], res)


@pytest.mark.parametrize("name", [n for n in ALL_CASES if nw.compares_stat(n)])
def test_nothing_is_left_out(name):
    """the conditions of null_walk_cases: outside the p4 cases no pair is left out of any kind -- every site vector has a
    norm (centred: kappa <= 3) far above its delta, no branch total lies near a threshold"""
    c = case(name)
    for kind in nw.KINDS:
        exp = expected(name, kind)
        if nw.leaves_out(name, kind):       # MI of the signed register: totals that are 0 in exact arithmetic
            assert exp["left_out"].sum() < len(exp["left_out"]), (name, kind)
            continue
        assert exp["left_out"].sum() == 0, (name, kind, int(exp["left_out"].sum()))
        assert (exp["stat_atol"] >= 0).all() and np.isfinite(exp["stat_atol"]).all()
    t = c["counts"][:, :, 0]
    d = t - t.mean(axis=1, keepdims=True)
    assert (np.linalg.norm(t, axis=1) <= 3 * np.linalg.norm(d, axis=1)).all()
    tot = pc.totals(c["counts"])
    for th in (0.99, 1.0, 10000.0):
        assert (np.abs(tot - th) > 1e-6 * th).all()


# ------------------------------------------------------------------------------------------------ the oracle's null
NULL_PARAMS = [(n, m) for n in WALK_CASES for m in cpu.METHODS if m == "decomp" or _unif_runs(n)]


@pytest.mark.parametrize("name,method", NULL_PARAMS)
def test_oracle_null_meets_the_expected_outputs(name, method):
    fig = null_figures(name, cpu.METHODS[method])
    print(name, method, " ".join(f"{fig[k]:.1e}" for k in NULL_COLUMNS), f"cosub {fig[2]:.0f}")
    for k, v in fig.items():
        assert v <= 1.0, (name, method, k, v)
    row = _table("MEASURED-NULL")[name]
    if method == "decomp":          # the committed table is what this run gives
        for k, v in zip(NULL_COLUMNS, row):
            assert float(f"{fig[k]:.1e}") == v, (name, k, fig[k], v)


# ------------------------------------------------------------------------------------------------ the bars, from both sides
@pytest.mark.parametrize("name", [n for n in ALL_CASES if nw.compares_stat(n)])
def test_stat_bars_are_what_the_counts_bar_allows(name):
    """counts moved entrywise by the whole of their own bar, +-(e |n| + atol_b) with seeded random signs, twenty times:
    oracle's statistic of every compared pair moves by at most its bar (the bar is no tighter than the counts' bar
    allows) and, for every kind with a bar, on some pair by more than a hundredth of it (no looser than two orders above);
    the threshold kinds do not move at all.  The lower side is asserted on the cases without a saturated branch: a count of
    hundreds on a branch of 120 ... 10000 is nearly the whole vector, a relative perturbation of it nearly a rescaling, which
    the normalised kinds do not see; the bar, a bound in the norm, still is what an error spread over the other branches may
    use (printed figures: 1e-7 ... 6e-3 of the bar there)."""
    c = case(name)
    _, i0, i1 = pairs(name)
    e, atol = nw.counts_bar(rows()[name]), cpu.count_atol(c)
    ref = c["counts"]
    rng = np.random.default_rng(4100 + ALL_CASES.index(name))
    most = {k: 0.0 for k in nw.KINDS}
    for _ in range(20):
        sign = rng.choice([-1.0, 1.0], size=ref.shape)
        moved = ref + sign * (e * np.abs(ref) + atol[None, :, None])
        if c["clamp"]:          # clamped counts are sums of non-negative products in every implementation
            moved = np.maximum(moved, 0.0)
        for kind in nw.KINDS:
            exp = expected(name, kind)
            params = oracle.stat_params(kind, nw.MI_THRESHOLD)
            with np.errstate(all="ignore"):
                got = oracle.pair_stats_inter(kind, moved, moved, params)[i0, i1]
            if kind in nw.THRESHOLDS:
                keep = ~exp["left_out"]
                assert np.array_equal(got[keep], exp["stat"][keep], equal_nan=True), (name, kind)
                continue
            r = np.abs(got - exp["stat"]) / exp["stat_atol"]
            assert np.isfinite(r).all() and r.max() <= 1.0, (name, kind, float(r.max()))
            most[kind] = max(most[kind], float(r.max()))
    print(name, " ".join(f"{nw.KIND_NAMES[k]} {v:.3f}" for k, v in most.items() if k not in nw.THRESHOLDS))
    if c["blen"].max() < 100.0:
        for kind, v in most.items():
            assert kind in nw.THRESHOLDS or v > 0.01, (name, kind, v)


# ------------------------------------------------------------------------------------------------ the 12-leaf tree's walks
def _walk_args(name):
    i = oe.Inputs(name)
    return i.parent, i.blen, i.lot, i.Q, i.pi, i.rates, i.probs, i.Bk


def test_the_deep_tree_walks_store_load_and_gather():
    """host plans only (no GPU): t12 has four inlined cherries, and its walks store and load workspace vectors, some of them
    through the wave's LDS slot; t4 and t5 have two cherries, t4 no stored vector and t5 one, neither an LDS slot"""
    for name in ("protein-g4-t12-q3", "protein-ig5-t12-q1", "protein_k2-g4-t12-q2"):
        w = engine.debug_cherry_msg_walk(*_walk_args(name))
        assert w["tables"] == 4 and w["gathers"] == 8, (name, w)
        assert w["loads"] > 0 and w["stores"] > 0 and w["lds_loads"] > 0, (name, w)
        g = engine.debug_walk(*_walk_args(name))
        assert g["loads"] > 0 and g["stores"] > 0 and g["lds_loads"] > 0, (name, g)
    for name in ("dna-g4-t12-q1", "dna-ig5-t12-q2"):
        g = engine.debug_walk(*_walk_args(name))
        assert g["cherry_tables"] == 4, (name, g)
        assert g["loads"] > 0 and g["stores"] > 0, (name, g)
    for name, stored in (("protein-g4-t5-p2", 1), ("protein-ig5-t4-p2", 0)):      # t5: one vector waits for the third child
        w = engine.debug_cherry_msg_walk(*_walk_args(name))
        assert w["tables"] == 2 and w["loads"] == w["stores"] == stored and w["lds_loads"] == 0, (name, w)
    assert engine.debug_walk(*_walk_args("dna-g4-t4-p2"))["cherry_tables"] == 2
    assert engine.debug_walk(*_walk_args("dna-ig5-t5-p2"))["cherry_tables"] == 2


if __name__ == "__main__":          # the tables of the docstring, measured anew
    print("MEASURED-CASES\n  case                          counts:unif  decomp     logL  post_rate")
    measured = {}
    for name in oe.DEEP_CASES:
        c = case(name)
        u = cpu.measure_case(c, oracle.METHOD_UNIF) if _unif_runs(name) else None
        d = cpu.measure_case(c, oracle.METHOD_DECOMP)
        assert d[3] and (u is None or u[3]), name
        logl, pr = max(d[1], u[1] if u else 0), max(d[2], u[2] if u else 0)
        print(f"  {name:28s} {'-' if u is None else '%.1e' % u[0]:>10s} {d[0]:9.1e} {logl:9.1e} {pr:9.1e}")
        measured[name] = [None if u is None else float("%.1e" % u[0])] + [float("%.1e" % v) for v in (d[0], logl, pr)]
        sys.stdout.flush()
    print("\nMEASURED-NULL (error / bar; decomposition, and the largest of the row under uniformization; - = not run)")
    print("  case                            nmin    prmin      cor     comp      cos      cov      euc       mi     unif")
    allrows = {**cpu._table("MEASURED-CASES"), **measured}
    for name in WALK_CASES:
        d = null_figures(name, oracle.METHOD_DECOMP, row=allrows[name])
        u = max(null_figures(name, oracle.METHOD_UNIF, row=allrows[name]).values()) if _unif_runs(name) else None
        print(f"  {name:28s} " + " ".join(f"{d[k]:8.1e}" for k in NULL_COLUMNS) + f" {'-' if u is None else '%.1e' % u:>8s}")
        assert d[2] == 0.0
        sys.stdout.flush()
