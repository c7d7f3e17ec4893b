"""The CPU restatements of the operators against tests/golden/operator_edges.npz (50-digit known answers at the edges of branch
length and rate: tests/golden/make_operator_edge_fixture.py, cases in tests/operator_edge_cases.py).  No GPU.

What is compared, and how the error is measured:

  * operators (np_oracle.transition_matrix, count_matrix_uniformization, count_matrix_decomposition,
    scaled_reference.operators) per generator: max |A - ref| / max |ref| over the matrix, the largest over the stored times
    (J(0) = 0 must come out as exact zeros);
  * oracle.map_sites per case, METHOD_UNIF and METHOD_DECOMP: logL and post_rate relative; counts as the smallest rtol with
        |count - ref| <= rtol |ref| + A t_b r_top,        A = 8 S eps max(|V| |Vinv B V| |Vinv|)   (operator_rounding)
    The absolute term is the a-priori rounding bound of the branch's operator: the closed form goes through
    V ( . ) Vinv, whose rounding error is absolute in the operator (max |J| ~ t_b r), while a count between equal states on
    a branch of 1e-12 is O(t^2) = 1e-24: fp64 cannot give that entry a relative accuracy.  On a zero-length branch the
    term is 0: the counts are exact zeros.
    Where an entry of P = V e^(L t) Vinv is below P's own rounding (off-diagonals carry +-1e-17 ... 1e-15 of either sign:
    the 1e-100 branch, and at 20 and 61 states the pairs with rates of 1e-5 on a 1e-12 branch) it can come out <= 0, and
    N = J / P with the Bio++ guards (negative -> 0) then dropped J(x, y) from P o N: counts of 1e-12 came out 1e-4 ... 1e-3
    low, counts of 1e-100 up to 100 %.  The joint operator needs no quotient; engine and oracles now keep J(x, y) there
    (P > 0 gives P (J / P) = J whatever P's error), and profiles 4 and 5 meet the same bars as the others.
    The rate class is compared where the fixture's two best classes are more than 1e-9 apart (class_clear; a site whose taxa
    all sit beyond saturated branches has the same likelihood under every fast class).

  * oracle.map_sites_noavg and oracle.map_sites_marginal (the three other nijt.average / nijt.joint options, which read the
    conditional counts N1 and NC entry by entry) on the cases of operator_edge_cases.has_variants(): no time (zero-length
    branches, the rate-zero class: N = 0 exactly) and saturated branches; where states are chosen, on the branches whose two
    best candidates are more than 1e-9 apart in the fixture (variant_figure).

Every bound asserted is 10 x the value measured here (x86-64 glibc), not less than 1e-13 and not more than 1e-8; the table
is read by the tests, so it is the one statement of the bounds (tests/test_gpu_operator_edges.py reads it too).
`python tests/test_operator_edges.py` prints it anew.  Uniformization is left out where its series needs more than 1e4 terms
(mu r_top t > 1e4: every profile 7); the fixture is the reference, so nothing is lost.  Before the saturated form of Phi
(cmx_host_model.cpp, oracle.c, np_oracle.py: d > 680) the decomposition counts of the 150-long branches were 70 ... 78 % low
summed over the sites (every count of the top rate class zero; single entries 90 ... 100 % low), those of the 10000-long
branch 99 ... 100 %: test_old_form_lost_the_saturated_counts keeps the evidence.

MEASURED-CASES
  case                          counts:unif  decomp     logL  post_rate
  dna-g4-t4-p1                    9.8e-15   8.6e-15   2.7e-15   1.0e-14
  dna-g4-t4-p2                    1.3e-14   1.2e-14   2.5e-15   9.6e-15
  dna-g4-t4-p3                    3.0e-14   2.8e-14   5.2e-15   2.3e-14
  dna-g4-t4-p4                    0.0e+00   0.0e+00   3.0e-15   3.3e-16
  dna-g4-t4-p5                    7.9e-15   8.0e-15   2.3e-15   7.6e-15
  dna-g4-t4-p6                    7.9e-11   5.5e-15   5.6e-15   2.1e-14
  dna-g4-t4-p7                          -   9.7e-13   2.3e-13   7.0e-13
  dna-g4-t4-p8                    6.0e-11   6.0e-15   2.7e-15   1.2e-14
  dna-ig5-t5-p1                   1.0e-14   1.2e-14   1.9e-15   9.1e-15
  dna-ig5-t5-p2                   1.6e-14   1.5e-14   2.8e-15   1.4e-14
  dna-ig5-t5-p6                   8.3e-11   9.3e-15   5.7e-15   2.7e-14
  dna-ig5-t5-p7                         -   8.9e-13   1.7e-13   7.6e-13
  dna-c1-t4-p1                    6.5e-15   7.5e-15   2.0e-15   0.0e+00
  dna-c1-t4-p3                    1.2e-14   1.0e-14   2.1e-15   0.0e+00
  dna-c1-t4-p6                    1.9e-11   2.6e-15   4.1e-15   0.0e+00
  jc4-g4-t4-p1                    9.0e-15   9.0e-15   1.8e-15   7.0e-15
  jc4-g4-t4-p6                    6.0e-11   8.5e-15   4.9e-15   1.9e-14
  jcp4-g4-t4-p1                   2.8e-14   2.8e-14   4.0e-15   2.4e-14
  jcp4-g4-t4-p6                   6.0e-11   5.9e-15   4.2e-15   1.6e-14
  protein-g4-t5-p1                2.3e-13   2.1e-13   2.4e-14   1.7e-13
  protein-g4-t5-p2                3.3e-13   3.0e-13   2.6e-14   2.1e-13
  protein-g4-t5-p3                9.2e-14   9.1e-14   1.5e-14   7.5e-14
  protein-g4-t5-p4                0.0e+00   0.0e+00   1.2e-14   8.9e-16
  protein-g4-t5-p5                5.9e-13   5.7e-13   6.0e-14   4.3e-13
  protein-g4-t5-p6                1.1e-10   4.8e-14   7.4e-15   5.5e-14
  protein-g4-t5-p7                      -   6.1e-13   7.7e-14   3.9e-13
  protein-g4-t5-p8                9.4e-11   1.3e-13   1.5e-14   1.2e-13
  protein-ig5-t4-p2               2.8e-13   2.6e-13   2.6e-14   2.2e-13
  protein-ig5-t4-p6               1.0e-10   2.7e-13   2.5e-14   2.2e-13
  protein-c1-t4-p7                      -   1.2e-12   1.1e-13   0.0e+00
  jc20-g4-t4-p1                   2.6e-12   2.6e-12   2.7e-13   1.9e-12
  jc20-g4-t4-p6                   6.1e-11   5.2e-13   3.1e-14   4.3e-13
  jcp20-g4-t4-p1                  2.8e-12   2.9e-12   2.8e-13   2.1e-12
  jcp20-g4-t4-p6                  6.1e-11   9.9e-13   6.9e-14   8.0e-13
  protein_k2-g4-t4-p6             1.0e-10   6.4e-14   9.1e-15   5.9e-14
  protein_signed-g4-t4-p1         6.3e-13   6.4e-13   3.6e-14   2.2e-13
  protein_signed-g4-t4-p6         4.9e-11   6.1e-14   5.9e-15   7.7e-14
  s7-g4-t5-p1                     2.0e-14   2.2e-14   4.4e-15   2.0e-14
  s7-g4-t5-p3                     4.2e-14   4.3e-14   4.9e-15   4.2e-14
  s7-g4-t5-p6                     1.1e-10   2.2e-14   4.1e-15   1.8e-14
  s7-g4-t5-p7                           -   1.4e-13   4.1e-14   1.8e-13
  s7-ig5-t4-p2                    1.2e-14   1.3e-14   3.2e-15   1.3e-14
  s61-g4-t4-p1                    1.4e-12   1.4e-12   1.1e-13   1.0e-12
  s61-g4-t4-p4                    0.0e+00   0.0e+00   1.6e-14   1.9e-15
  s61-g4-t4-p6                    8.9e-11   6.3e-13   3.5e-14   5.2e-13
  s61-g4-t4-p8                    6.7e-11   3.3e-13   2.3e-14   2.5e-13

MEASURED-VARIANTS (decomposition; largest over the cases of each generator and rate set)
  cases                a0j1     a1j0     a0j0
  dna-g4              1.1e-14  1.5e-12  1.1e-14
  dna-ig5             6.6e-15  1.3e-12  6.6e-15
  dna-c1              6.5e-15  1.8e-14  7.4e-15
  jc4-g4              3.7e-15  9.1e-14  3.7e-15
  jcp4-g4             6.8e-15  5.2e-14  6.8e-15
  protein-g4          1.0e-12  1.3e-12  1.0e-12
  protein-ig5         1.4e-13  7.6e-13  1.4e-13
  protein-c1          1.2e-12  1.2e-12  1.2e-12
  jc20-g4             1.1e-12  4.5e-12  1.8e-12
  jcp20-g4            1.0e-12  7.3e-12  1.0e-12
  protein_k2-g4       3.7e-14  3.3e-12  3.7e-14
  protein_signed-g4   6.7e-14  1.6e-11  9.0e-14
  s7-g4               3.5e-14  2.6e-13  3.5e-14
  s7-ig5              9.1e-15  1.1e-13  9.1e-15

MEASURED-OPERATORS
  generator         np:P   unif J  decomp J     sr:P  sr:P o NC
  dna             1.2e-11  8.0e-10  1.2e-11  1.9e-13  8.1e-11
  jc4             2.4e-12  6.3e-10  2.4e-12  3.7e-14  8.5e-11
  jcp4            9.6e-12  6.7e-10  9.6e-12  1.4e-13  8.5e-11
  protein         9.9e-12  8.2e-10  9.9e-12  1.5e-13  1.0e-10
  protein_signed  9.9e-12  8.0e-10  1.0e-11  1.5e-13  8.0e-11
  jc20            2.2e-12  6.4e-10  2.2e-12  3.3e-14  8.5e-11
  jcp20           8.0e-14  6.8e-10  8.0e-14  2.6e-15  8.5e-11
  s7              6.2e-12  9.7e-10  6.2e-12  9.4e-14  1.1e-10
"""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":          # run as a script (below): the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
from oracle import np_oracle as npo
import operator_edge_cases as oe
import scaled_reference as sr
from conftest import ROOT

FLOOR, CEILING = 1e-13, 1e-8
UNIF_MAX_TERMS = 1e4
METHODS = {"unif": oracle.METHOD_UNIF, "decomp": oracle.METHOD_DECOMP}


def bound(measured):
    return min(max(10.0 * measured, FLOOR), CEILING)


def _table(title):
    """rows of the docstring table under `title`: {first column: [floats]} ('-' = not measured)"""
    rows, on = {}, False
    for line in __doc__.splitlines():
        if line.strip() == title:
            on = True
        elif on and not line.strip():
            break
        elif on and not line.lstrip().startswith("case") and not line.lstrip().startswith("generator"):
            f = line.split()
            rows[f[0]] = [None if v == "-" else float(v) for v in f[1:]]
    return rows


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(ROOT, "tests", "golden", "operator_edges.npz"))


def operator_rounding(Q, pi, Bk=None):
    """A = 8 S eps max(|V| |Vinv B_k V| |Vinv|): the a-priori bound of the rounding error of an entry of
    J / t = V [ (Vinv B V) o Phi / t ] Vinv, |Phi / t| <= 1: S eps for each of the four products of length S behind it
    (two for Vinv B V, two around Phi) and for each of V, Vinv, the eigenvalues and Phi itself.  A property of the
    generator, not of any code under test: 2e-14 (S = 4), 9e-14 (JTT), 2e-13 (S = 61)."""
    lam, V, Vinv = npo.eigen_reversible(Q, pi)
    regs = [npo.rate_matrix_register(Q)] if Bk is None else list(Bk)
    G = max(float(np.max(np.abs(V) @ np.abs(Vinv @ B @ V) @ np.abs(Vinv))) for B in regs)
    return 8 * len(pi) * np.finfo(np.float64).eps * G


def count_atol(c):
    """[B] the absolute term of the counts' tolerance, A t_b r_top"""
    return operator_rounding(c["Q"], c["pi"], oe.register_of(c)) * c["blen"][:-1] * c["rates"].max()


def needed_rtol(counts, c):
    """the smallest rtol with |counts - ref| <= rtol |ref| + count_atol; inf where a reference zero is missed"""
    ref = c["counts"]
    over = np.abs(counts - ref) - count_atol(c)[None, :, None]
    if np.isnan(counts).any() or (over[ref == 0] > 0).any():
        return np.inf
    nz = ref != 0
    return float(np.max(np.maximum(over[nz], 0) / np.abs(ref[nz]))) if nz.any() else 0.0


def unif_terms(c):
    return np.abs(np.diag(c["Q"])).max() * c["rates"].max() * c["blen"].max()


def map_case(c, method):
    m = oracle.Model(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"], Bk=oe.register_of(c),
                     method=method, nonneg=bool(c["clamp"]))
    return oracle.map_sites(m, c["aln"])


def measure_case(c, method):
    """-> (counts, logL, post_rate) figures and whether the clear rate classes agree"""
    with np.errstate(all="ignore"):
        r = map_case(c, method)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))  # noqa: E731
    ok = np.array_equal(r["rate_class"][c["class_clear"]], c["rate_class"][c["class_clear"]])
    return needed_rtol(r["counts"], c), rel(r["logL"], c["logL"]), rel(r["post_rate"], c["post_rate"]), ok


def _unif_runs(name):
    i = oe.Inputs(name)
    return np.abs(np.diag(i.Q)).max() * i.rates.max() * i.blen.max() <= UNIF_MAX_TERMS


# uniformization is left out where its series needs more than 1e4 terms: the 10000-long branch of every profile 7
CASE_PARAMS = [(n, m) for n in oe.CASES for m in METHODS if m == "decomp" or _unif_runs(n)]
assert [n for n in oe.CASES if not _unif_runs(n)] == [n for n in oe.CASES if n.endswith("p7")]


@pytest.mark.parametrize("name,method", CASE_PARAMS)
def test_oracle_mapping_meets_the_fixture(fix, name, method):
    c = oe.load(fix, name)
    row = _table("MEASURED-CASES")[name]
    counts, logl, prate, classes = measure_case(c, METHODS[method])
    print(f"{name} {method}: counts {counts:.1e} logL {logl:.1e} post_rate {prate:.1e}")
    # one bound for both methods: the fixed decomposition form must meet what uniformization meets
    measured = [v for v in row[:2] if v is not None]
    assert counts <= bound(max(measured)), counts
    assert logl <= bound(row[2]) and prate <= bound(row[3])
    assert classes


# ------------------------------------------------------------------------------------------------ the three other options
VARIANTS = {"a0j1": (False, True), "a1j0": (True, False), "a0j0": (False, False)}      # (nijt.average, nijt.joint)
VARIANT_CASES = [n for n in oe.CASES if oe.has_variants(n)]


def variant_figure(counts, c, key):
    """a mapping under another nijt option against the fixture's: the largest relative error over the branches whose choice
    of states is clear (the fixture's two best candidates more than 1e-9 apart; every branch where nothing is chosen).
    Reference zeros (no time: N = 0) must be met exactly; the absolute term is the averaged counts'.  inf if NaN."""
    ref = c["counts_" + key]
    clear = np.ones(ref.shape[:2], dtype=bool) if key == "a1j0" else c["margin_" + key] > 1e-9
    assert clear.mean() > 0.5
    a, r = counts[clear], ref[clear]
    over = np.abs(a - r) - np.broadcast_to(count_atol(c)[None, :, None], ref.shape)[clear]
    if np.isnan(a).any() or (over[r == 0] > 0).any():
        return np.inf
    return float(np.max(np.maximum(over[r != 0], 0) / np.abs(r[r != 0]))) if (r != 0).any() else 0.0


def map_variant(c, key, method=oracle.METHOD_DECOMP):
    m = oracle.Model(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"], Bk=oe.register_of(c),
                     method=method, nonneg=bool(c["clamp"]))
    with np.errstate(all="ignore"):
        if key == "a0j1":
            return oracle.map_sites_noavg(m, c["aln"])["counts"]
        return oracle.map_sites_marginal(m, c["aln"], average=key == "a1j0")["counts"]


VARIANT_BOUND = 1.6e-10     # 10 x the largest figure measured over all cases and options, 1.6e-11 (MEASURED-VARIANTS)


@pytest.mark.parametrize("key", list(VARIANTS))
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_oracle_variant_mappings_meet_the_fixture(fix, name, key):
    """nijt.average / nijt.joint through N1 and NC (conditional counts at no time and on saturated branches), decomposition"""
    c = oe.load(fix, name)
    fig = variant_figure(map_variant(c, key), c, key)
    print(f"{name} {key}: {fig:.1e}")
    assert fig <= VARIANT_BOUND


def _operator_figures(fix, gen):
    """-> [np P, np unif J, np decomp J, scaled_reference P, scaled_reference PN (the joint operator P o NC)]"""
    Q, pi, Bk, clamp = oe.generator(gen)
    regs = [npo.rate_matrix_register(Q)] if Bk is None else list(Bk)
    ts, Pref, Jref = fix[f"ops.{gen}.t"], fix[f"ops.{gen}.P"], fix[f"ops.{gen}.J"]
    eig = npo.eigen_reversible(Q, pi)
    mu = np.abs(np.diag(Q)).max()

    def err(a, ref):
        if not ref.any():
            return 0.0 if not a.any() else np.inf
        return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))

    fig = np.zeros(5)
    with np.errstate(all="ignore"):
        for i, t in enumerate(ts):
            fig[0] = max(fig[0], err(npo.transition_matrix(*eig, t), Pref[i]))
            for k, B in enumerate(regs):
                fig[1] = max(fig[1], err(npo.count_matrix_uniformization(Q, B, t), Jref[i, k]))
                fig[2] = max(fig[2], err(npo.count_matrix_decomposition(*eig, B, t), Jref[i, k]))
        few = [i for i, t in enumerate(ts) if mu * t <= UNIF_MAX_TERMS]
        star = np.full(len(few) + 1, len(few), dtype=np.int32)
        star[-1] = -1
        ops = sr.operators(star, np.append(ts[few], 0.0), Q, pi, np.array([1.0]), Bk=regs, nonneg=clamp)
        for j, i in enumerate(few):
            fig[3] = max(fig[3], err(ops["P"][0, j], Pref[i]))
            for k in range(len(regs)):
                fig[4] = max(fig[4], err(ops["PN"][0, j, k], Jref[i, k]))
                assert np.array_equal(ops["NC"][0, j], ops["N1"][j])
    return fig


@pytest.mark.parametrize("gen", oe.OPERATOR_MODELS)
def test_numpy_operators_meet_the_fixture(fix, gen):
    row = _table("MEASURED-OPERATORS")[gen]
    fig = _operator_figures(fix, gen)
    print(gen, " ".join(f"{v:.1e}" for v in fig))
    for v, m in zip(fig, row):
        assert v <= bound(m), (fig, row)


def _phi_old(lam, t):
    """Phi as it was evaluated before the saturated form"""
    d = (lam[:, None] - lam[None, :]) * t
    e = np.exp(lam * t)
    with np.errstate(all="ignore"):
        return d, np.where(np.abs(d) < 1e-14, t * e[:, None], t * e[None, :] * np.expm1(d) / d)


@pytest.mark.parametrize("name", [n for n in oe.CASES if n.endswith("p8")])
def test_profile_8_keeps_its_bits(fix, name):
    """t = 120: every d is below the switch, and the count operators are byte for byte what the old expression gave.  The old
    expression is oracle.c's and the engine's (_phi_old restates it in numpy), not np_oracle's former plain quotient, whose
    bits moved at every t; the engine's own bits are compared between builds (scripts/compare_host_model.py)."""
    c = oe.load(fix, name)
    lam, V, Vinv = npo.eigen_reversible(c["Q"], c["pi"])
    B = npo.rate_matrix_register(c["Q"])
    for t in np.unique(np.outer(c["rates"], c["blen"])):
        d, phi = _phi_old(lam, t)
        assert d.max() < 680.0 and np.isfinite(phi).all()
        old = V @ ((Vinv @ B @ V) * phi) @ Vinv
        assert old.tobytes() == npo.count_matrix_decomposition(lam, V, Vinv, B, t).tobytes()


@pytest.mark.parametrize("name", [n for n in oe.CASES if n[-1] in "67" and n.startswith(("dna-g4", "protein-g4"))])
def test_old_form_lost_the_saturated_counts(fix, name):
    """why the old form failed, restated (_phi_old is oracle.c's and the engine's former expression in numpy): its Phi is not
    finite on the saturated branches, where the new one is.  The before / after evidence itself is the fixture comparison
    of test_oracle_mapping_meets_the_fixture run on the parent (70 ... 100 % low)."""
    c = oe.load(fix, name)
    lam, V, Vinv = npo.eigen_reversible(c["Q"], c["pi"])
    t = c["blen"].max() * c["rates"].max()
    assert not np.isfinite(_phi_old(lam, t)[1]).all()
    assert np.isfinite(npo.count_matrix_decomposition(lam, V, Vinv, npo.rate_matrix_register(c["Q"]), t)).all()


def test_star_is_the_smallest_that_rescales():
    """the one case of tests/test_gpu_operator_edges.py that only the fp64 reference can serve: with Invariant + Gamma(4)
    rates a star of 62 leaves is the smallest at which scaled_reference rescales a site; on that (variable) site class 0
    has likelihood exactly 0, so the site exponent comes from the classes with a positive share.  With V Vinv for the P of
    the rate-zero class (off-diagonals of +-1e-15, either sign) the reference's logL was NaN here from 42 leaves on."""
    def run(n, **kw):
        base, rates, probs, aln = oe.star_case(n)
        with np.errstate(all="ignore"):
            return sr.map_sites(base.parent, base.blen, base.lot, aln, base.Q, base.pi, rates, probs, **kw)
    assert not run(oe.STAR_LEAVES - 1)["exponent"].any()
    ref = run(oe.STAR_LEAVES)
    assert ref["exponent"].any() and np.isfinite(ref["logL"]).all() and np.isfinite(ref["counts"]).all()
    if sr.has_extended_range():         # the unscaled computation in long double does not underflow here
        ld = run(oe.STAR_LEAVES, dtype=np.longdouble, scale=False)
        assert np.max(np.abs(ref["logL"] - ld["logL"]) / np.abs(ld["logL"])) < 1e-13
        assert np.max(np.abs(ref["counts"] - ld["counts"]) / np.abs(ld["counts"])) < 1e-13
        assert np.array_equal(ref["rate_class"], ld["rate_class"])


def test_a_rate_zero_class_has_the_identity_exactly():
    """... in every restatement; a zero-length branch under a positive rate keeps the eigen product V Vinv"""
    for gen in ("dna", "protein", "s61"):
        Q, pi, _, _ = oe.generator(gen)
        eig = npo.eigen_reversible(Q, pi)
        assert np.array_equal(npo.class_transition_matrix(*eig, 0.3, 0.0), np.eye(len(pi)))
        assert np.array_equal(npo.class_transition_matrix(*eig, 0.0, 1.0), npo.transition_matrix(*eig, 0.0))
        assert np.array_equal(npo.class_transition_matrix(*eig, 0.3, 2.0), npo.transition_matrix(*eig, 0.6))
    parent, blen, _ = oe.TREES["t4"]
    Q, pi, _, _ = oe.generator("protein")
    with np.errstate(all="ignore"):
        ops = sr.operators(parent, blen, Q, pi, oe.rate_set("ig5")[0])
    for b in range(len(parent) - 1):
        assert np.array_equal(ops["P"][0, b], np.eye(20)) and not ops["NC"][0, b].any()


def test_fixture_inputs_are_the_cases(fix):
    """the stored inputs are what tests/operator_edge_cases.py describes, and every stored logL is finite"""
    for name in oe.CASES:
        c, i = oe.load(fix, name), oe.Inputs(name)
        aln, cls = i.draw()
        assert np.array_equal(c["aln"], aln) and np.array_equal(c["classes"], cls)
        assert np.array_equal(c["blen"], i.blen) and np.array_equal(c["Q"], i.Q) and np.array_equal(c["rates"], i.rates)
        assert aln.shape == (len(i.lot), oe.NSITES) and np.isfinite(c["logL"]).all() and np.isfinite(c["counts"]).all()


if __name__ == "__main__":          # the tables of the docstring, measured anew
    f = np.load(os.path.join(ROOT, "tests", "golden", "operator_edges.npz"))
    print("MEASURED-CASES\n  case                          counts:unif  decomp     logL  post_rate")
    for name in oe.CASES:
        c = oe.load(f, name)
        u = measure_case(c, oracle.METHOD_UNIF) if unif_terms(c) <= UNIF_MAX_TERMS else None
        d = measure_case(c, oracle.METHOD_DECOMP)
        assert d[3] and (u is None or u[3]), name
        logl, pr = max(d[1], u[1] if u else 0), max(d[2], u[2] if u else 0)
        print(f"  {name:28s} {'-' if u is None else '%.1e' % u[0]:>10s} {d[0]:9.1e} {logl:9.1e} {pr:9.1e}")
        sys.stdout.flush()
    print("\nMEASURED-VARIANTS (decomposition; largest over the cases of each generator and rate set)\n  cases                a0j1     a1j0     a0j0")
    groups = {}
    for name in VARIANT_CASES:
        c = oe.load(f, name)
        g = groups.setdefault(name.rsplit("-", 2)[0], [0.0, 0.0, 0.0])
        for q, key in enumerate(VARIANTS):
            g[q] = max(g[q], variant_figure(map_variant(c, key), c, key))
    for k, v in groups.items():
        print(f"  {k:18s} " + " ".join(f"{x:8.1e}" for x in v))
    print("\nMEASURED-OPERATORS\n  generator         np:P   unif J  decomp J     sr:P  sr:P o NC")
    for gen in oe.OPERATOR_MODELS:
        print(f"  {gen:14s} " + " ".join(f"{v:8.1e}" for v in _operator_figures(f, gen)))
