"""Numpy restatement of the weighted statistics (weighted), a plain helper module imported by the tests.

Two forms of the same definitions:
* `pair_brute` / `matrix_brute` / `group_brute`: one pair at a time, branch by branch in the reference's order, as
  CoMap/Statistics.h:164-294 and Distance.h:150-171 write them with a weight vector attached;
* `matrix_gram`: the form the device computes -- per-site operands X_b = weight_factor(kind, w_b) * value_b, one
  product X1 . X2^T, the unweighted epilogues of the Cosinus / scalar product / Compensation statistics, and for
  EuclidianDistance the differences of the scaled totals.

Counts are site-major [N, B, K] (the reference's mapping[i][b][k]); w is normalised (sum 1) by `normalise`, which is
what Statistic::setWeights stores (Statistics.h:135-140).  Parity unpinned: bpp-core's VectorTools (the weighted
mean / cov / cos) is not restated in the reference tree; Cosinus squares the weights here, the other kinds take them once.
"""
import math

import numpy as np

CORRELATION, COMPENSATION, COSUBSTITUTION, COSINUS, COVARIANCE, DISCRETE_MI, CORRECTED_CORRELATION, EUCLIDIAN = range(8)
WEIGHTED_KINDS = (CORRELATION, COMPENSATION, COSINUS, COVARIANCE, CORRECTED_CORRELATION, EUCLIDIAN)
IGNORING_KINDS = (COSUBSTITUTION, DISCRETE_MI, 8)   # Cosubstitution, DiscreteMI, DiscreteMI with bounds


def normalise(w):
    w = np.asarray(w, dtype=np.float64)
    s = 0.0
    for x in w:            # VectorTools::sum: in order
        s += x
    return w / s


def weight_factor(kind, w):
    """the per-branch factor of the operand (cmx_pairstat.h weight_factor)"""
    return np.asarray(w, dtype=np.float64) if kind == COSINUS else np.sqrt(w)


# ------------------------------------------------------------------------------------------------ pair by pair
def pair_brute(kind, v1, v2, w, mv1=None, mv2=None):
    """one pair: v1, v2 [B, K]; mv1 / mv2 the mean vectors of CorrectedCorrelation"""
    B = v1.shape[0]
    if kind in (CORRELATION, COVARIANCE, CORRECTED_CORRELATION):
        x = [v1[b, 0] - (mv1[b] if kind == CORRECTED_CORRELATION else 0.0) for b in range(B)]
        y = [v2[b, 0] - (mv2[b] if kind == CORRECTED_CORRELATION else 0.0) for b in range(B)]
        mx = my = 0.0
        for b in range(B):                       # weighted mean: scalar(v, w)
            mx += w[b] * x[b]
            my += w[b] * y[b]
        sxy = sxx = syy = 0.0
        for b in range(B):                       # cov / var: w applied once to the products, not unbiased
            sxy += w[b] * (x[b] - mx) * (y[b] - my)
            sxx += w[b] * (x[b] - mx) ** 2
            syy += w[b] * (y[b] - my) ** 2
        if kind == COVARIANCE:
            return sxy
        return _div(sxy, math.sqrt(sxx) * math.sqrt(syy))
    if kind == COSINUS:
        sxy = sxx = syy = 0.0
        for b in range(B):
            sxy += w[b] * w[b] * v1[b, 0] * v2[b, 0]
            sxx += w[b] * w[b] * v1[b, 0] ** 2
            syy += w[b] * w[b] * v2[b, 0] ** 2
        return _div(sxy, math.sqrt(sxx) * math.sqrt(syy))
    if kind == COMPENSATION:                     # Statistics.h:250-264
        s1 = s2 = s3 = 0.0
        for b in range(B):
            t1, t2 = float(np.sum(v1[b])), float(np.sum(v2[b]))
            s1 += t1 ** 2 * w[b]
            s2 += t2 ** 2 * w[b]
            s3 += (t1 + t2) ** 2 * w[b]
        return 1.0 - _div(math.sqrt(s3), math.sqrt(s1) + math.sqrt(s2))
    if kind == EUCLIDIAN:                        # Distance.h:157-171
        d = 0.0
        for b in range(B):
            t1, t2 = float(np.sum(v1[b])), float(np.sum(v2[b]))
            d += w[b] * (t2 - t1) ** 2
        return math.sqrt(d)
    raise ValueError(kind)


def _div(a, b):
    if b == 0.0:
        return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a)
    return a / b


def matrix_brute(kind, c1, w, c2=None, mv=None):
    """all pairs; intra (c2 None): entries j > i, NaN elsewhere (CoETools.cpp:680).  mv: [2, B] (CorrectedCorrelation;
    intra uses mv[0] on both sides, as the engine's one-operand intra form does)"""
    intra = c2 is None
    c2 = c1 if intra else c2
    mv1 = None if mv is None else mv[0]
    mv2 = None if mv is None else (mv[0] if intra else mv[1])
    out = np.full((len(c1), len(c2)), np.nan)
    for i in range(len(c1)):
        for j in range(i + 1 if intra else 0, len(c2)):
            out[i, j] = pair_brute(kind, c1[i], c2[j], w, mv1, mv2)
    return out


def group_brute(kind, counts, sites, w):
    """Statistic::getValueForGroup: Compensation's closed form (Statistics.h:267-294) or the minimum over pairs (i, j),
    j < i, where a NaN pair never wins (AbstractMinimumStatistic, :121-133)"""
    v = [counts[s] for s in sites]
    if kind == COMPENSATION:
        B = counts.shape[1]
        sumsq1 = [0.0] * len(v)
        sumsq2 = 0.0
        for b in range(B):
            s = 0.0
            for j in range(len(v)):
                sv = float(np.sum(v[j][b]))
                sumsq1[j] += sv ** 2 * w[b]
                s += sv
            sumsq2 += s ** 2 * w[b]
        return 1.0 - _div(math.sqrt(sumsq2), sum(math.sqrt(x) for x in sumsq1))
    mini = math.inf
    for i in range(1, len(v)):
        for j in range(i):
            val = pair_brute(kind, v[i], v[j], w)
            if val < mini:
                mini = val
    return mini


# ------------------------------------------------------------------------------------------------ the device's form
def operand(kind, counts, w, mv=None):
    """X [N, B] of pair_prep_kernel with weights"""
    if kind in (CORRELATION, COVARIANCE, CORRECTED_CORRELATION):
        x = counts[:, :, 0] - (mv[None, :] if mv is not None else 0.0)
        x = x - (x * w[None, :]).sum(1, keepdims=True)
    elif kind == COSINUS:
        x = counts[:, :, 0]
    else:
        x = counts.sum(2)
    return x * weight_factor(kind, w)[None, :]


def matrix_gram(kind, c1, w, c2=None, mv=None):
    intra = c2 is None
    mvs = (None, None) if mv is None else (mv[0], mv[0] if intra else mv[1])
    X1 = operand(kind, c1, w, mvs[0])
    X2 = X1 if intra else operand(kind, c2, w, mvs[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == EUCLIDIAN:
            out = np.sqrt(((X2[None, :, :] - X1[:, None, :]) ** 2).sum(2))
        else:
            g = X1 @ X2.T
            s1, s2 = (X1 ** 2).sum(1), (X2 ** 2).sum(1)
            if kind == COVARIANCE:
                out = g
            elif kind == COMPENSATION:
                s3 = np.maximum(s1[:, None] + s2[None, :] + 2 * g, 0.0)
                direct = ((X1[:, None, :] + X2[None, :, :]) ** 2).sum(2)      # signed totals: where the identity cancels
                s3 = np.where(2 * g < -0.5 * (s1[:, None] + s2[None, :]), direct, s3)
                out = 1.0 - np.sqrt(s3) / (np.sqrt(s1)[:, None] + np.sqrt(s2)[None, :])
            else:     # correlation (centred operand) and cosinus: g / sqrt(s_i s_j)
                out = g / (np.sqrt(s1)[:, None] * np.sqrt(s2)[None, :])
    if intra:
        out[np.tril_indices(len(c1))] = np.nan
    return out


def unweighted_brute(kind, c1, c2=None):
    """the unweighted statistics the uniform-weight identities compare with (VectorTools::cor / cov unbiased / cos)"""
    intra = c2 is None
    c2 = c1 if intra else c2
    B = c1.shape[1]
    out = np.full((len(c1), len(c2)), np.nan)
    for i in range(len(c1)):
        for j in range(i + 1 if intra else 0, len(c2)):
            x, y = c1[i, :, 0], c2[j, :, 0]
            t1, t2 = c1[i].sum(1), c2[j].sum(1)
            if kind in (CORRELATION, COVARIANCE):
                cov = float(((x - x.mean()) * (y - y.mean())).sum()) / (B - 1)
                out[i, j] = cov if kind == COVARIANCE else _div(cov, math.sqrt(((x - x.mean()) ** 2).sum() / (B - 1)) *
                                                                math.sqrt(((y - y.mean()) ** 2).sum() / (B - 1)))
            elif kind == COSINUS:
                out[i, j] = _div(float(x @ y), math.sqrt(float(x @ x)) * math.sqrt(float(y @ y)))
            elif kind == COMPENSATION:
                out[i, j] = 1.0 - _div(math.sqrt(float(((t1 + t2) ** 2).sum())), math.sqrt(float(t1 @ t1)) + math.sqrt(float(t2 @ t2)))
            elif kind == EUCLIDIAN:
                out[i, j] = math.sqrt(float(((t2 - t1) ** 2).sum()))
    return out


def close(a, b, rtol, atol):
    """same NaN pattern, and |a - b| <= rtol |b| + atol elsewhere; returns (ok, worst excess)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False, math.inf
    m = ~np.isnan(b)
    if not m.any():
        return True, 0.0
    excess = np.abs(a[m] - b[m]) - (rtol * np.abs(b[m]) + atol)
    return bool((excess <= 0).all()), float(excess.max())


def random_counts(rng, n, B, K, constant_sites=(), scale=3.0):
    """non-negative random counts [n, B, K] with a few exact zeros; sites in constant_sites have no type-0 substitution
    on any branch (a constant type-0 vector: correlation and cosinus NaN on every path -- a constant c != 0 is not
    exactly constant after the weighted mean sum_b w_b c, whose weights sum to 1 only up to rounding)"""
    c = rng.gamma(0.7, scale, size=(n, B, K))
    c[rng.random(size=c.shape) < 0.15] = 0.0
    for s in constant_sites:
        c[s, :, 0] = 0.0
    return c
