"""Regenerates tests/golden/mica_counts.npz: the column mutual information, joint entropy and entropies of the cases of
tests/mica_count_cases.py from the definition (SiteTools::mutualInformation / jointEntropy / entropy with resolveUnknowns =
true, natural log; SURVEY.md row a12, tests/mica_wide_reference.py) at 50 digits.

Counts are exact.  A symbol spreads the weight 1 / |mask| over the states of its mask, so with L = lcm of the mask sizes
every fractional count is m / L^2 with the INTEGER m = sum_t u_a(t) v_b(t), u = L / |mask| (with full unknowns alone:
m / A^2, m = A^2 N_ab + A (N_aG + N_Gb) + N_GG); the marginals are u_a / L.  For the pairs of a column with a partial code
the same tables are summed a second time as fractions.Fraction from the weights themselves and compared.  Then, with ln of
every distinct integer evaluated once,

    MI     = sum_ab  p_ab ln(p_ab / (p_a p_b))     p_ab = m / (L^2 T), p_a = u_a / (L T)
    Hjoint = - sum_ab p_ab ln p_ab                 H = - sum_a p_a ln p_a

and the second route MI = H1 + H2 - Hjoint must agree to 1e-40.

    python tests/golden/make_mica_count_fixture.py            (a few minutes)
"""
import os
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mica_count_cases as mc  # noqa: E402

mp.mp.dps = 50
_LN = {}


def ln(k):
    k = int(k)
    v = _LN.get(k)
    if v is None:
        v = _LN[k] = mp.log(k)
    return v


def entropy(u, L, T):
    """u: [A] integer marginal; p = u / (L T)"""
    lnLT = ln(L * T)
    return -mp.fsum(int(x) * (ln(x) - lnLT) for x in u if x) / (L * T)


def pair(m, ua, ub, L, T):
    """m [A, A], ua, ub [A] -> (MI, Hjoint), both routes compared"""
    D = L * L * T
    a, b = np.nonzero(m)
    lnT, lnD = ln(T), ln(D)
    mi = mp.fsum(int(m[x, y]) * (ln(m[x, y]) + lnT - ln(ua[x]) - ln(ub[y])) for x, y in zip(a, b)) / D
    hj = -mp.fsum(int(m[x, y]) * (ln(m[x, y]) - lnD) for x, y in zip(a, b)) / D
    second = entropy(ua, L, T) + entropy(ub, L, T) - hj
    assert abs(mi - second) < mp.mpf(10) ** -40, (mi, second)
    return mi, hj


def fraction_table(c1, c2, A):
    """the joint table of two columns summed as fractions from the weights 1 / |mask|"""
    k, t = mc.popcounts(A)
    tab = [[Fraction(0)] * A for _ in range(A)]
    codes, counts = np.unique(np.stack([c1, c2], axis=1), axis=0, return_counts=True)
    for (x, y), n in zip(codes, counts):
        w = Fraction(int(n), int(k[x]) * int(k[y]))
        for a in range(A):
            if (int(t[x]) >> a) & 1:
                for b in range(A):
                    if (int(t[y]) >> b) & 1:
                        tab[a][b] += w
    return tab


def evaluate(c):
    A, T, a1, a2 = c["A"], c["T"], c["a1"], c["a2"]
    L = mc.denominator(A)
    u1, u2 = mc.units(a1, A), mc.units(a2, A)
    m12, m11 = mc.gram(u1, u2), mc.gram(u1, u1)
    s1, s2 = u1.sum(axis=0), u2.sum(axis=0)
    n1, n2 = a1.shape[1], a2.shape[1]
    assert (m12.sum(axis=3) == L * s1[:, None, :]).all() and (m12.sum(axis=2) == L * s2[None, :, :]).all()
    # the pairs of the partial-code columns, a second time from the weights themselves
    p1, p2 = mc.has_partial(a1, A), mc.has_partial(a2, A)
    for i in range(n1):
        for j in range(n2):
            if p1[i] or p2[j]:
                ft = fraction_table(a1[:, i], a2[:, j], A)
                assert all(ft[a][b] == Fraction(int(m12[i, j, a, b]), L * L) for a in range(A) for b in range(A))
    # with full unknowns alone the table is the kernels' m / A^2
    k = L // A
    clean = ~(p1[:, None] | p2[None, :])
    assert (m12[clean] == k * k * mc.weighted_cells(mc.pseudo_counts(a1, a2, A), A)[clean]).all()
    out = {}
    mi, hj = np.zeros((n1, n2)), np.zeros((n1, n2))
    for i in range(n1):
        for j in range(n2):
            mi[i, j], hj[i, j] = (float(v) for v in pair(m12[i, j], s1[i], s2[j], L, T))
    out["mi"], out["hjoint"] = mi, hj
    iu = np.triu_indices(n1)
    imi, ihj = np.zeros((n1, n1)), np.zeros((n1, n1))
    for i, j in zip(*iu):
        imi[i, j], ihj[i, j] = (float(v) for v in pair(m11[i, j], s1[i], s1[j], L, T))
    out["imi"], out["ihjoint"] = imi[iu], ihj[iu]
    out["h1"] = np.array([float(entropy(s1[i], L, T)) for i in range(n1)])
    out["h2"] = np.array([float(entropy(s2[j], L, T)) for j in range(n2)])
    full = imi + np.triu(imi, 1).T, ihj + np.triu(ihj, 1).T
    out["pmi"], out["phjoint"] = mi[c["i1"], c["i2"]], hj[c["i1"], c["i2"]]
    out["qmi"], out["qhjoint"] = full[0][c["i1"], c["i2"]], full[1][c["i1"], c["i2"]]
    out["hash"] = np.array(mc.input_hash(c))
    return out


def main():
    data = {}
    for name in mc.CASES:
        for k, v in evaluate(mc.case(name)).items():
            data[f"{name}.{k}"] = v
        print(name, flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "mica_counts.npz"), **data)


if __name__ == "__main__":
    main()
