"""TEST INFRASTRUCTURE ONLY: a second, fast route to oracle.cluster.hclust's answer, and the group properties from
their definitions.

hclust_fast follows the definition of oracle.cluster.hclust (NaN -> +inf; closest pair by strict `<`, first pair in
row-major order; everything +inf: the first live pair; linkage update (ni*x + nj*y)/(ni + nj) with every operation
rounded on its own) but keeps an exact (minimum, first column) per row beside the matrix and repairs it EAGERLY after
each join, so a step costs O(n) numpy work plus the rows it has to rescan.  It knows nothing of stale marks or lower
bounds: it is not a restatement of the device kernel.

group_properties_exact computes Nmin and Stat of every inner node from the node's member list, in 50-digit arithmetic;
props_restated is the kernel's own form (host norm loop, sons-first running sums, the device's summation order) in
fp64, whose distance from the exact values gives the tolerances of the GPU tests."""
import math
from fractions import Fraction

import numpy as np

from oracle import cluster as oc

SEGMENT = 512      # columns one wave rescans at a time in the device kernel; only the `spanning` counter knows of it

MUTANTS = ("tie_last", "keep_cached", "grew_taken", "avg_unweighted", "avg_fma", "size_one_son")


def _fma(a, x, q):
    """round(a * x + q) elementwise for fp64 arrays (a: scalar): Dekker's exact product, then the three terms summed with
    the rounding errors carried along -- the fused form of the average linkage (mutant only)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * x
        split = 134217729.0                       # 2^27 + 1
        ah = split * a
        ah = ah - (ah - a)
        al = a - ah
        xh = split * x
        xh = xh - (xh - x)
        xl = x - xh
        e = ((ah * xh - p) + ah * xl + al * xh) + al * xl     # p + e == a * x exactly
        s = p + q
        bb = s - p
        t = (p - (s - bb)) + (q - bb)             # s + t == p + q exactly
        r = s + (t + e)
    return np.where(np.isfinite(r), r, p + q)


def hclust_fast(dist, linkage, mutant=None):
    """-> merge int32 [n-1][2], dmax float64 [n-1], size int32 [n-1], counters dict(ties, rescans, spanning, inf_joins):
    ties      steps at which more than one live pair attained the minimum,
    rescans   rows rescanned because their cached neighbour was one of the joined pair,
    spanning  of those, rows with a live column SEGMENT or more columns right of their first candidate column,
    inf_joins joins made at +inf.
    mutant: one of MUTANTS, a deliberately wrong variant (tests/test_cluster_reference.py)."""
    assert mutant is None or mutant in MUTANTS
    last = mutant == "tie_last"
    D = np.array(dist, dtype=np.float64, copy=True)
    n = D.shape[0]
    D[np.isnan(D)] = np.inf
    live = np.ones(n, dtype=bool)
    cid = np.arange(n)
    csz = np.ones(n, dtype=np.int64)
    rmin = np.full(n, np.inf)
    nn = np.full(n, -1)
    merge = np.zeros((max(n - 1, 0), 2), dtype=np.int32)
    dmax = np.zeros(max(n - 1, 0))
    size = np.zeros(max(n - 1, 0), dtype=np.int32)
    cnt = dict(ties=0, rescans=0, spanning=0, inf_joins=0)

    def first_min(v):
        return int(np.argmin(v)) if not last else len(v) - 1 - int(np.argmin(v[::-1]))

    def rescan(r):
        cols = r + 1 + np.flatnonzero(live[r + 1:])
        if len(cols) == 0:
            rmin[r], nn[r] = np.inf, -1
            return cols
        seg = D[r, cols]
        c = first_min(seg)
        rmin[r], nn[r] = seg[c], cols[c]
        return cols

    for r in range(n):
        rescan(r)
    for m in range(n - 1):
        rows = np.flatnonzero(nn >= 0)
        i = int(rows[first_min(rmin[rows])])
        j = int(nn[i])
        d = rmin[i]
        right = i + 1 + np.flatnonzero(live[i + 1:])
        if np.count_nonzero(rmin[rows] == d) > 1 or np.count_nonzero(D[i, right] == d) > 1:
            cnt["ties"] += 1
        cnt["inf_joins"] += int(d == np.inf)
        merge[m] = (cid[i], cid[j])
        dmax[m] = d
        ni, nj = float(csz[i]), float(csz[j])
        if linkage == oc.LINK_COMPLETE:
            new = np.maximum(D[i], D[j])
        elif linkage == oc.LINK_SINGLE:
            new = np.minimum(D[i], D[j])
        elif mutant == "avg_unweighted":
            new = (D[i] + D[j]) / 2.0
        elif mutant == "avg_fma":
            new = _fma(ni, D[i], nj * D[j]) / (ni + nj)
        else:
            new = (ni * D[i] + nj * D[j]) / (ni + nj)
        live[j] = False
        keep = live.copy()
        keep[i] = False
        D[i, keep] = new[keep]
        D[keep, i] = new[keep]
        size[m] = csz[i] if mutant == "size_one_son" else csz[i] + csz[j]
        cid[i] = n + m
        csz[i] += csz[j]
        rmin[j], nn[j] = np.inf, -1
        # rows whose cached neighbour was one of the pair: left of i both can be, between i and j only j
        lost = np.flatnonzero(keep & ((nn == i) | (nn == j)))
        for r in lost:
            r = int(r)
            if mutant == "grew_taken" and r < i:
                rmin[r], nn[r] = new[r], i
                continue
            old = rmin[r]
            cols = rescan(r)
            if mutant == "keep_cached" and nn[r] >= 0:
                rmin[r] = old
            cnt["rescans"] += 1
            cnt["spanning"] += int(len(cols) > 0 and cols[-1] - (r + 1) >= SEGMENT)
        # every other live row left of i takes the new entry by the (value, column) rule
        other = keep[:i].copy()
        other[lost[lost < i]] = False
        left = np.flatnonzero(other)
        v = new[left]
        if last:
            take = (v < rmin[left]) | ((v == rmin[left]) & (i > nn[left]))
        else:
            take = (v < rmin[left]) | ((v == rmin[left]) & (i < nn[left]))
        rmin[left[take]] = v[take]
        nn[left[take]] = i
        rescan(i)
    return merge, dmax, size, cnt


def same_tree(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


# ---- group properties

def _exact_sites(counts):
    """per site: the branch totals as exact fractions [n][B] and the norm sqrt(sum_b total^2) to 50 digits"""
    import mpmath
    mpmath.mp.dps = 50
    c = np.asarray(counts, dtype=np.float64)
    sigma = [[sum((Fraction(float(x)) for x in row), Fraction(0)) for row in site] for site in c]
    norm = []
    for s in sigma:
        q = sum((t * t for t in s), Fraction(0))
        norm.append(mpmath.sqrt(mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator)))
    return sigma, norm


def exact_norm(counts):
    """every site's norm, 50 digits rounded to fp64"""
    return np.array([float(x) for x in _exact_sites(counts)[1]])


def host_norm(counts):
    """the engine's host loop in fp64: branch totals over K in order, squared and accumulated in branch order"""
    c = np.asarray(counts, dtype=np.float64)
    n, B, K = c.shape
    sigma = np.zeros((n, B))
    for k in range(K):
        sigma = sigma + c[:, :, k]
    q = np.zeros(n)
    for b in range(B):
        q = q + sigma[:, b] * sigma[:, b]
    return np.sqrt(q)


def group_properties_exact(dist_kind, merge, dmax, counts):
    """"Stat" and "Nmin" of every inner node from its member list (oracle.cluster.groups), no running sums:
    Nmin = the smallest norm among the members; Stat = the join distance (Euclidean), 1 - it (correlation), or
    1 - |sum of the members' vectors| / sum of the members' norms (compensation).  50 digits, rounded to fp64 at the end."""
    import mpmath
    mpmath.mp.dps = 50
    n = len(merge) + 1
    sigma, norm = _exact_sites(counts)
    normf = np.array([float(x) for x in norm])                   # monotone rounding: the minimum commutes with it
    stat, nmin = np.zeros(n - 1), np.zeros(n - 1)
    for m, mem in oc.groups(merge):
        nmin[m] = normf[mem].min()
        if dist_kind == oc.DIST_EUCLIDIAN:
            stat[m] = dmax[m]
        elif dist_kind == oc.DIST_CORRELATION:
            stat[m] = float(mpmath.mpf(1) - mpmath.mpf(float(dmax[m])))
        else:
            B = len(sigma[0])
            tot = [sum((sigma[s][b] for s in mem), Fraction(0)) for b in range(B)]
            q = sum((t * t for t in tot), Fraction(0))
            num = mpmath.sqrt(mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator))
            den = mpmath.fsum(norm[s] for s in mem)
            stat[m] = float(mpmath.mpf(1) - num / den)
    return stat, nmin


def _wave_sum(v):
    """the xor butterfly of the device's wave_sum over 64 lanes (offsets 32, 16, .. 1); every lane ends up the same"""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ off]
    return v[0]


def props_restated(dist_kind, merge, dmax, counts):
    """the engine's form in fp64: the host's norm loop (branch totals over K in order, squared and accumulated in branch
    order), then per merge in order nm = min of the sons', sn = sum of the sons', the branch vector = sum of the sons',
    its squares summed per thread (stride 256), per wave (butterfly) and over the four waves in order"""
    c = np.asarray(counts, dtype=np.float64)
    n, B, K = c.shape
    sigma = np.zeros((n, B))
    for k in range(K):
        sigma = sigma + c[:, :, k]
    norm = host_norm(c)
    nm = np.concatenate([norm, np.zeros(n - 1)])
    sn = nm.copy()
    sg = np.concatenate([sigma, np.zeros((n - 1, B))])
    stat = np.zeros(n - 1)
    for m in range(n - 1):
        x, y = merge[m]
        nm[n + m] = min(nm[x], nm[y])
        sn[n + m] = sn[x] + sn[y]
        if dist_kind == oc.DIST_EUCLIDIAN:
            stat[m] = dmax[m]
        elif dist_kind == oc.DIST_CORRELATION:
            stat[m] = 1.0 - dmax[m]
        else:
            s = sg[x] + sg[y]
            sg[n + m] = s
            sq = np.zeros(256)
            for t0 in range(0, B, 256):
                part = s[t0:t0 + 256]
                sq[:len(part)] = sq[:len(part)] + part * part
            w = [_wave_sum(sq[64 * k:64 * k + 64]) for k in range(4)]
            stat[m] = 1.0 - math.sqrt(w[0] + w[1] + w[2] + w[3]) / sn[n + m]
    return stat, nm[n:]
