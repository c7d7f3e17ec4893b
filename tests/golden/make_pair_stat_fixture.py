"""Generator of tests/golden/pair_stats.npz: the pair and group statistics of the inputs of tests/pair_stat_cases.py,
evaluated from their definitions with mpmath (200 digits) and rounded once to double.

    python tests/golden/make_pair_stat_fixture.py [output.npz]

Definitions restated (mapping[i][b][k] = counts[i, b, k]; x = type 0, t = per-branch total):
* Correlation / Covariance / Cosinus (CoMap/Statistics.h:164-228): VectorTools::cor, cov (unbiased, B - 1), cos of x; with
  weights cor(x, y, w, false), cov(x, y, w, false, false), cos(x, y, w) as DESIGN.md A.7 reads them: mean sum w x, the
  weights once on the products (squared for cos), no B - 1.
* CorrectedCorrelation (:176-204): cor of x - meanVector.
* Cosubstitution (:230-245): branches with t1 >= 1 and t2 >= 1.
* Compensation (:247-295): 1 - sqrt(sum w (t1 + t2)^2) / (sqrt(sum w t1^2) + sqrt(sum w t2^2)); for a group
  1 - sqrt(sum_b w (sum_j t_jb)^2) / sum_j sqrt(sum_b w t_jb^2).
* DiscreteMI (:307-327): classes Domain::getIndex (Domain.cpp:113-122: first i >= 1 with t < bounds[i], out of range
  outside [bounds[0], bounds[last])), VectorTools::miDiscrete = sum over observed cells of (n_ac / B) ln(n_ac B / (n_a n_c))
  / ln(2.7182818); an out-of-range total makes the pair NaN (the reference throws).
* EuclidianDistance (Distance.h:150-171): sqrt(sum w (t2 - t1)^2).
* a group (AbstractMinimumStatistic, Statistics.h:121-133): the minimum over pairs (i, j < i) with "val < mini", so a NaN
  never wins and a group without a finite pair gives +inf.
The indicator kinds use the double total (VectorTools::sum, one rounding for K = 2); the others the exact one.
A quotient 0 / 0 is NaN, as it is in the reference's doubles.
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pair_stat_cases as pc  # noqa: E402

mp.mp.dps = 200     # 50 digits pin a double; the pair (2^-100 v, 2^100 v) of Compensation cancels over 60 of them
NAN, INF = float("nan"), float("inf")


def _v(a):
    return [mp.mpf(float(x)) for x in a]


def _div(a, b):
    if b == 0:
        return NAN if a == 0 else (INF if a > 0 else -INF)
    return a / b


def _dot(x, y, w=None):
    return mp.fsum(a * b * (1 if w is None else c) for a, b, c in zip(x, y, w if w is not None else x))


def _centre(x, w):
    m = mp.fsum(x) / len(x) if w is None else _dot(x, [1] * len(x), w)
    return [a - m for a in x]


def pair_value(cs, key, i, j):
    kind, B = pc.kind_of(key), cs.B
    w = _v(cs.w) if key[0] == "w" else None
    ci, cj = cs.counts[i], cs.counts[j]
    if kind in (0, 4, 6, 3, 9):
        x, y = _v(ci[:, 0]), _v(cj[:, 0])
        if kind == 6:
            mv = _v(cs.mv)
            x, y = [a - m for a, m in zip(x, mv)], [a - m for a, m in zip(y, mv)]
        if kind == 9:
            return _dot(x, y)
        if kind == 3:
            w2 = None if w is None else [a * a for a in w]
            return _div(_dot(x, y, w2), mp.sqrt(_dot(x, x, w2)) * mp.sqrt(_dot(y, y, w2)))
        dx, dy = _centre(x, w), _centre(y, w)
        sxy, sxx, syy = _dot(dx, dy, w), _dot(dx, dx, w), _dot(dy, dy, w)
        if kind == 4:
            return sxy if w is not None else sxy / (B - 1)
        if w is not None:
            return _div(sxy, mp.sqrt(sxx) * mp.sqrt(syy))
        return _div(sxy / (B - 1), mp.sqrt(sxx / (B - 1)) * mp.sqrt(syy / (B - 1)))
    if kind in (1, 7):
        t1 = [mp.fsum(_v(r)) for r in ci]
        t2 = [mp.fsum(_v(r)) for r in cj]
        if kind == 7:
            return mp.sqrt(_dot([b - a for a, b in zip(t1, t2)], [b - a for a, b in zip(t1, t2)], w))
        s3 = [a + b for a, b in zip(t1, t2)]
        q = _div(mp.sqrt(_dot(s3, s3, w)), mp.sqrt(_dot(t1, t1, w)) + mp.sqrt(_dot(t2, t2, w)))
        return q if q != q else 1 - q
    T = pc.totals(cs.counts[[i, j]])
    if kind == 2:
        return float(((T[0] >= 1.0) & (T[1] >= 1.0)).sum())
    C = pc.classes(T, pc.MI_BOUNDS[key])
    if (C < 0).any():
        return NAN
    s = mp.fsum(mp.mpf(n) / B * mp.log(mp.mpf(n) * B / (mp.mpf(a) * c)) for n, a, c in pc.mi_terms(C[0], C[1]))
    return s / mp.log(mp.mpf(2.7182818))


def group_value(cs, key, members, pairs):
    """pairs: the [19, 19] matrix of the pair values of this key, already rounded to double"""
    if pc.kind_of(key) == 1:
        w = _v(cs.w) if key[0] == "w" else None
        t = [[mp.fsum(_v(r)) for r in cs.counts[s]] for s in members]
        tot = [mp.fsum(col) for col in zip(*t)]
        q = _div(mp.sqrt(_dot(tot, tot, w)), mp.fsum(mp.sqrt(_dot(x, x, w)) for x in t))
        return float(q if q != q else 1 - q)
    mini = INF
    for a in range(1, len(members)):
        for b in range(a):
            val = pairs[members[a], members[b]]
            if val < mini:
                mini = val
    return mini


def case_arrays(cs):
    out = {cs.name + ".counts": cs.counts, cs.name + ".w": cs.w_raw, cs.name + ".mv": cs.mv}
    for key in pc.KEYS:
        tri = np.array([float(pair_value(cs, key, i, j)) for i, j in zip(*pc.IU)])
        out[f"{cs.name}.{key}"] = tri
        if key in pc.GROUP_KEYS:
            full = pc.full_matrix(tri)
            out[f"{cs.name}.g_{key}"] = np.array([group_value(cs, key, g, full) for g in pc.GROUPS])
    return out


def main(path):
    arrays = {}
    for cs in pc.all_cases():
        arrays.update(case_arrays(cs))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "pair_stats.npz"))
