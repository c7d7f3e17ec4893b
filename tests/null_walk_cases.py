"""What the null's mapping walks are held to on supplied alignments, from the 50-digit fixtures alone: a plain helper module
(no GPU) shared by tests/test_null_walk_reference.py (CPU: the oracle against these answers, and the evidence for the bars)
and tests/test_gpu_null_walk_edges.py (every device path of the null against the same answers at the same bars).

The fixtures are tests/golden/operator_edges.npz (trees t4, t5) and tests/golden/null_walk_edges.npz (tree t12); cases,
trees and profiles in tests/operator_edge_cases.py.  A null over supplied alignments maps every supplied column and scores
column j of side 0 against column j of side 1, so every expected output follows from the fixture's per-column answers:

    nmin, prmin, rcmin      the minima over the two columns of the norm (square root of the sum over the branches of the
                            squared K-sums, as test_gpu_operator_edges._check forms it), post_rate and rate_class; rcmin is
                            compared where both columns are class_clear
    stat                    oracle.stat_pair of the two columns' fixture counts (pinned to the definitions by
                            tests/test_pair_stat_fixture.py; its own fp64 error at kappa <= 3 is orders below the bars)

BARS.  They come from the inputs alone.  With the case's row of MEASURED-CASES (test_operator_edges for t4 and t5,
test_null_walk_reference for t12; both measured from the oracle, never from the engine):

    e       = max(1e-9, bound(decomposition figure of the counts))     the counts' relative bar of test_gpu_operator_edges
    atol_b  = count_atol(c)[b] = A t_b r_top                           the counts' absolute term (operator_rounding)
    a       = K ||atol||                                               the absolute term of a site's vector of K-sums
    delta_i = e ||t_i|| + a                                            how far, in the 2-norm, column i's vector may be off

t_i is the vector a statistic reads: the per-branch totals (K-sums) for Compensation, EuclidianDistance, Cosubstitution and
MI; type 0 alone for Correlation, Covariance and Cosinus (VectorTools::cor / cov / cos on the first type: oracle.c
orc_stat_pair, pair_stat_strided).  A counts array within its bar, |n' - n| <= e |n| + atol_b entrywise, has ||t' - t|| <=
delta (for the K-sums: |sum_k dn| <= e sum_k |n_k| + K atol_b, and sum_k |n_k| = |t| for K = 1 and for non-negative counts --
every case here; a signed register with K = 2 would need sum |n_k| in place of |t|).

    nmin        relative e, absolute a          (| ||t'|| - ||t|| | <= ||t' - t||; the minimum of two such is one of them)
    prmin       relative max(1e-12, bound(post_rate figure))
    rcmin       equal

With d the centred vector (centring is a projection: ||d' - d|| <= ||t' - t||), n = ||t||, r_i = delta_i / ||d_i|| (or / n_i)
the perturbation bounds of the statistics are, to first order,

    Correlation         2 (r_i + r_j)           a unit vector moves by at most 2 delta / ||d||, and |u'.v' - u.v| <=
    Cosinus             2 (r_i + r_j)           ||u' - u|| + ||v' - v|| + ||u' - u|| ||v' - v||
    Compensation        2 (delta_i + delta_j) / (n_i + n_j)     q = ||t_i + t_j|| / (n_i + n_j) <= 1: numerator and
                                                                denominator each move by at most delta_i + delta_j
    EuclidianDistance   delta_i + delta_j                       the triangle inequality
    Covariance          (delta_i ||d_j|| + delta_j ||d_i||) / (B - 1)

The asserted bar is C_BAR = 3 times the sum in brackets for every kind (one constant): 2 is the largest first-order
constant above; the second-order terms are below 0.4 % of the first-order ones on every compared pair (each r < 1e-3, the
left-out rule below), and the fp64 error of stat_pair itself (a few B eps at kappa <= 3) is six orders below e; the third
unit covers both.  tests/test_null_walk_reference.py holds the constant from both sides: counts perturbed entrywise by the
full +-(e |n| + atol_b) never move stat_pair by more than the bar, and move it by more than a hundredth of it.

Cosubstitution and MI (threshold 0.99: bounds {0, 0.99, 10000}) compare totals with thresholds, so they are exact -- NaN
where a total leaves [0, 10000) -- on every pair without a total within 10 (e |t| + K atol_b) of a threshold (0.99, 1,
10000; for a signed register also 0, unless the total is exactly 0: clamped counts are sums of non-negative products and
cannot leave the range there).  Cosubstitution is compared for equality; MI, a sum of logarithms over an
exact table, within twice pair_stat_cases.bound_mi (two fp64 evaluations of the same table).

LEFT OUT.  A condition on the inputs, not a measurement: a pair is left out of a centred kind (Correlation, Covariance) when
||d|| <= 1e3 delta on either side, of Cosinus when ||t|| <= 1e3 delta on either side, of Compensation when n_i + n_j <=
1e3 (delta_i + delta_j), of the threshold kinds by the rule above.  Outside the cases whose name ends in p4 no pair is left
out of any kind (asserted on the CPU and again by the GPU test), with one exception that the inputs force: MI of the
signed register.  Its W(x, y) = (y - x) / 10 is a gradient, so the signed count along any path from x to x is exactly 0: a
branch below a zero-length sister, or between equal neighbours, has a total that is 0 in exact arithmetic and +-1e-20 in any
other, and MI's lower bound 0 turns its sign into NaN or not.  Those pairs are left out of MI there (leaves_out), by the
same threshold rule; every other kind of those cases compares every pair.  In the p4 cases (every branch at 1e-12: the counts lie
below the operator's own rounding) stat is not compared; nmin, prmin and finiteness are."""
import numpy as np

import oracle
import operator_edge_cases as oe
import pair_stat_cases as pc
import test_operator_edges as cpu

C_BAR = 3
LEFT_OUT = 1e3
THRESHOLD_MARGIN = 10.0
KINDS = (0, 1, 2, 3, 4, 5, 7)
KIND_NAMES = {0: "Correlation", 1: "Compensation", 2: "Cosubstitution", 3: "Cosinus", 4: "Covariance", 5: "MI",
              7: "EuclidianDistance"}
TYPE0_KINDS = (0, 3, 4)
THRESHOLDS = {2: (0.99, 1.0, 10000.0), 5: (0.0, 0.99, 1.0, 10000.0)}
MI_THRESHOLD = 0.99


def supplied_pairs(aln, S):
    """-> (sup [3, 2, T, n], i0 [3 n], i1 [3 n]): three supplied replicates over the n fully resolved columns `res` of aln
    (every code < S; a null refuses anything else), and per pair the columns of aln on side 0 and side 1.
    Replicate 0: res against res rotated by one; 1: res reversed against res reversed and rotated by seven; 2: res against
    res, every column against itself (both sides share every pattern)."""
    aln = np.asarray(aln)
    res = np.flatnonzero((aln < S).all(axis=0))
    rev = res[::-1]
    sides = [(res, np.roll(res, 1)), (rev, np.roll(rev, 7)), (res, res)]
    sup = np.ascontiguousarray(np.stack([np.stack([aln[:, a], aln[:, b]]) for a, b in sides]), dtype=np.uint8)
    return sup, np.concatenate([a for a, _ in sides]), np.concatenate([b for _, b in sides])


def counts_bar(row):
    """e of the docstring; row = the case's MEASURED-CASES figures (counts unif, counts decomp, logL, post_rate)"""
    return max(1e-9, cpu.bound(row[1]))


def compares_stat(name):
    return not name.endswith("p4")


def leaves_out(name, kind):
    """whether pairs of case `name` may be left out of statistic `kind` (docstring, LEFT OUT)"""
    return not compares_stat(name) or (kind == 5 and name.startswith("protein_signed"))


def _vectors(c, kind):
    """[N, B]: what statistic `kind` reads of every column"""
    return np.ascontiguousarray(c["counts"][:, :, 0]) if kind in TYPE0_KINDS else pc.totals(c["counts"])


def expected(c, i0, i1, kind, params=None, *, row):
    """the null's outputs over the pairs (column i0[j], column i1[j]) of the stored case c -> dict:
    nmin, prmin, rcmin, rc_clear [P] (where rcmin is compared), stat [P]; the bars nmin_rtol, nmin_atol, prmin_rtol,
    stat_atol [P] (absolute; 0 = equality); left_out [P] (pairs whose stat is not compared)"""
    e, atol = counts_bar(row), cpu.count_atol(c)
    K, B = c["counts"].shape[2], c["counts"].shape[1]
    a = K * float(np.linalg.norm(atol))
    norm = np.sqrt((pc.totals(c["counts"]) ** 2).sum(axis=1))
    out = dict(nmin=np.minimum(norm[i0], norm[i1]), nmin_rtol=e, nmin_atol=a,
               prmin=np.minimum(c["post_rate"][i0], c["post_rate"][i1]), prmin_rtol=max(1e-12, cpu.bound(row[3])),
               rcmin=np.minimum(c["rate_class"][i0], c["rate_class"][i1]).astype(np.int32),
               rc_clear=c["class_clear"][i0] & c["class_clear"][i1])
    params = (oracle.stat_params(kind, MI_THRESHOLD) if params is None else params)
    with np.errstate(all="ignore"):
        out["stat"] = np.array([oracle.stat_pair(kind, c["counts"][p], c["counts"][q], params) for p, q in zip(i0, i1)])
    t = _vectors(c, kind)
    if kind in THRESHOLDS:
        margin = THRESHOLD_MARGIN * (e * np.abs(t) + K * atol[None, :])
        near = np.zeros(len(t), dtype=bool)
        for th in THRESHOLDS[kind]:
            if th == 0.0 and bool(c["clamp"]):      # clamped counts are sums of non-negative products: never below 0
                continue
            near |= ((np.abs(t - th) < margin) & ~((th == 0.0) & (t == 0.0))).any(axis=1)
        out["left_out"] = near[i0] | near[i1]
        if kind == 5:
            cls = pc.classes(t, params[1:])
            out["stat_atol"] = 2.0 * np.array([pc.bound_mi(cls[p:p + 1], cls[q:q + 1], False)[0, 0] for p, q in zip(i0, i1)])
        else:
            out["stat_atol"] = np.zeros(len(i0))
        return out
    n = np.sqrt((t * t).sum(axis=1))
    delta = e * n + a
    d = np.sqrt(((t - t.mean(axis=1, keepdims=True)) ** 2).sum(axis=1))
    di, dj, ni, nj, ci, cj = delta[i0], delta[i1], n[i0], n[i1], d[i0], d[i1]
    none = np.zeros(len(i0), dtype=bool)
    with np.errstate(all="ignore"):
        if kind == 0:
            bar, left = di / ci + dj / cj, (ci <= LEFT_OUT * di) | (cj <= LEFT_OUT * dj)
        elif kind == 3:
            bar, left = di / ni + dj / nj, (ni <= LEFT_OUT * di) | (nj <= LEFT_OUT * dj)
        elif kind == 1:
            bar, left = (di + dj) / (ni + nj), (ni + nj) <= LEFT_OUT * (di + dj)
        elif kind == 7:
            bar, left = di + dj, none
        elif kind == 4:
            bar, left = (di * cj + dj * ci) / (B - 1), (ci <= LEFT_OUT * di) | (cj <= LEFT_OUT * dj)
        else:
            raise KeyError(kind)
    out["stat_atol"], out["left_out"] = C_BAR * bar, left
    return out


def figures(got, exp, name):
    """a null's outputs against `expected`: -> dict of error / bar per output (inf where something that has to be met
    exactly is not): nmin, prmin, stat (the largest over the compared pairs; 0 where stat is not compared), and
    compared / left_out, the numbers of pairs.  Every output must be free of NaN except where the expected stat is NaN."""
    fig = {}
    for key in ("nmin", "prmin"):
        bar = exp[key + "_rtol"] * np.abs(exp[key]) + exp.get(key + "_atol", 0.0)
        err = np.abs(got[key] - exp[key])
        with np.errstate(all="ignore"):
            r = np.where(err == 0, 0.0, err / bar)
        fig[key] = float(np.max(np.where(np.isnan(r), np.inf, r)))
    clear = exp["rc_clear"]
    fig["rcmin"] = 0.0 if np.array_equal(np.asarray(got["rcmin"])[clear], exp["rcmin"][clear]) else np.inf
    keep = ~exp["left_out"]
    if compares_stat(name):
        r = pc.ratio(got["stat"][keep], exp["stat"][keep], exp["stat_atol"][keep])
        fig["stat"] = float(r.max()) if r.size else 0.0
    else:       # finiteness: a NaN only where the definition gives one (MI with a total out of range)
        fig["stat"] = 0.0 if np.array_equal(np.isnan(got["stat"][keep]), np.isnan(exp["stat"][keep])) else np.inf
    fig["compared"], fig["left_out"] = int(keep.sum()), int((~keep).sum())
    return fig


def deep_fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "null_walk_edges.npz"))
