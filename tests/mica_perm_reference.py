"""Test support: Mica's permutation test (miTest, CoMap/Mica.cpp:93-118) for any alphabet of 2 .. 64 states without a mask
table, restated in numpy / Python from the rules of oracle/oracle.c (orc_mica_permutation_test_masks) with one non-state
code: a code < A is that state, every code >= A is the unknown.  The oracle is generic only up to 31 states (32-bit masks,
32 extended codes); tests/test_mica_perm_reference.py pins this restatement to it, as bytes, where both are defined.

  pairs in row-major (i < j) order; pvalue = (count + 1) / (nperm + 1); a pair stops at the 5th shuffle with s >= s_obs or at
  max_perm; a column with at most one distinct state among its resolved symbols makes the pair (1.0, 0);
  shuffle k of pair p: forward Fisher-Yates over the positions of the pair's copy of column j, jj = t + mulhi32(r, T - t),
  r = word t & 3 of Philox4x32-10(key = seed, counter = (p, p >> 32, k, 'P' << 24 | t >> 2));
  resolved pair: position t carries column i's states in sorted order, column j starts in taxon order,
  s = sum F[c_xy], F[c] = llround(c ln c 2^40);
  pair with an unknown: positions in column i's order (unknowns, then states ascending, stable), column j carried along,
  s = sum_ab F_g[A^2 N_ab + A (N_aU + N_Ub) + N_UU], F_g[m] = llround(m ln m 2^sh), sh = min(40, 62 - ceil(log2(M ln M))),
  M = A^2 T.  Logarithms are math.log (libm, as the oracle's and the library's host tables); F_g is evaluated only where it is
  read."""
import math

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _llround(x):
    f = math.floor(x)
    return f + (1 if x - f >= 0.5 else 0)


def philox4x32_10(c0, c1, c2, c3, seed):
    """arrays of 32-bit counter words (as uint64) -> four arrays of 32-bit results"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def shuffles(base, p, ks, seed):
    """the copies of `base` [T] after shuffle k, for every k of ks -> [len(ks), T]"""
    T, K = len(base), len(ks)
    nb = (T + 3) // 4
    kk = np.repeat(np.asarray(ks, dtype=np.uint64)[:, None], nb, axis=1)
    blk = np.uint64(0x50000000) | np.arange(nb, dtype=np.uint64)[None, :].repeat(K, axis=0)
    w = philox4x32_10(np.full((K, nb), p & 0xFFFFFFFF, dtype=np.uint64), np.full((K, nb), (p >> 32) & 0xFFFFFFFF, dtype=np.uint64), kk, blk, seed)
    r = np.stack(w, axis=2).reshape(K, 4 * nb)                      # word t & 3 of block t >> 2 at [k, t]
    q = np.repeat(np.asarray(base)[None, :], K, axis=0).copy()
    rows = np.arange(K)
    for t in range(T):
        jj = t + ((r[:, t] * np.uint64(T - t)) >> np.uint64(32)).astype(np.int64)
        vj = q[rows, jj]
        q[rows, jj] = q[:, t]
        q[:, t] = vj
    return q


class _Tables:
    def __init__(self, A, T):
        self.A, self.T = A, T
        self.F = np.array([0] + [_llround(c * math.log(c) * 1099511627776.0) for c in range(1, T + 1)], dtype=np.int64)
        M = float(A) * A * T
        self.sh = min(40, 62 - int(math.ceil(math.log2(M * math.log(M)))))
        self.scale = math.ldexp(1.0, self.sh)
        self.Fg = {0: 0}

    def fg(self, m):
        """F_g at every entry of the integer array m"""
        u, inv = np.unique(m, return_inverse=True)
        vals = np.empty(len(u), dtype=np.int64)
        for x, v in enumerate(u.tolist()):
            f = self.Fg.get(v)
            if f is None:
                f = self.Fg[v] = _llround(v * math.log(v) * self.scale)
            vals[x] = f
        return vals[inv.reshape(m.shape)]


def _sums_resolved(tb, xs, q):
    """sum_xy F[c_xy] of column i's sorted states xs [T] against every row of q [K, T]"""
    A, K = tb.A, q.shape[0]
    cell = (np.arange(K)[:, None] * (A * A) + xs[None, :].astype(np.int64) * A + q).ravel()
    c = np.bincount(cell, minlength=K * A * A).reshape(K, A * A)
    return tb.F[c].sum(axis=1)


def _sums_general(tb, xs, q):
    """the same over the integer table m_ab; xs, q hold the unknown as code A"""
    A, K = tb.A, q.shape[0]
    B = A + 1
    cell = (np.arange(K)[:, None] * (B * B) + xs[None, :].astype(np.int64) * B + q).ravel()
    c = np.bincount(cell, minlength=K * B * B).reshape(K, B, B)
    m = A * A * c[:, :A, :A] + A * (c[:, :A, A][:, :, None] + c[:, A, :A][:, None, :]) + c[:, A, A][:, None, None]
    return tb.fg(m).sum(axis=(1, 2))


def permutation_test(aln, A, max_perm, seed, pair_begin=0, pair_end=None):
    """-> (pvalue float64, nperm int32, general bool) of the pairs [pair_begin, pair_end); general: the pair took the
    unknowns' path"""
    aln = np.minimum(np.asarray(aln).astype(np.int64), A)            # every code >= A is the one unknown
    T, n = aln.shape
    npairs = n * (n - 1) // 2
    pair_end = npairs if pair_end is None else pair_end
    tb = _Tables(A, T)
    pv, nb = np.zeros(pair_end - pair_begin), np.zeros(pair_end - pair_begin, dtype=np.int32)
    gen = np.zeros(pair_end - pair_begin, dtype=bool)
    distinct = [len(set(aln[:, c][aln[:, c] < A].tolist())) for c in range(n)]
    has_unk = (aln >= A).any(axis=0)
    p = -1
    for i in range(n - 1):
        for j in range(i + 1, n):
            p += 1
            if p < pair_begin or p >= pair_end:
                continue
            o = p - pair_begin
            gen[o] = bool(has_unk[i] or has_unk[j])
            if distinct[i] <= 1 or distinct[j] <= 1:
                pv[o], nb[o] = 1.0, 0
                continue
            ci, cj = aln[:, i], aln[:, j]
            order = np.argsort(np.where(ci >= A, -1, ci), kind="stable")   # unknowns first, then the states ascending
            xs = ci[order]
            # the shuffled copy: column j along column i's order on the unknowns' path, in taxon order on the resolved one
            base, sums = (cj[order], _sums_general) if gen[o] else (cj, _sums_resolved)
            sobs = int(sums(tb, xs, cj[order][None, :])[0])              # observed: the columns paired taxon by taxon
            k, count = 0, 0
            while count < 5 and k < max_perm:
                K = min(16 if k == 0 else 64, max_perm - k)
                hits = sums(tb, xs, shuffles(base, p, np.arange(k, k + K), seed)) >= sobs
                for h in hits.tolist():
                    k += 1
                    count += 1 if h else 0
                    if count == 5:
                        break
            pv[o], nb[o] = (count + 1) / (k + 1), k
    return pv, nb, gen


def columns(A, T, n, seed):
    """the inputs of the permutation tests: every column shares a fraction drawn from {0, 0.1, 0.25, 0.5} of its cells with a
    common column; unknowns (codes A, 200, 255) in a tenth of the cells of the first third of the columns; from n >= 8 on
    three special columns: all unknown, constant at state A - 1, constant but for a single unknown"""
    rng = np.random.default_rng(seed)
    common = rng.integers(0, A, size=(T, 1))
    share = rng.choice([0.0, 0.1, 0.25, 0.5], size=(1, n))
    aln = np.where(rng.random((T, n)) < share, common, rng.integers(0, A, size=(T, n)))
    third = max(1, n // 3)
    u = rng.random((T, third))
    code = rng.choice([A, 200, 255], size=(T, third))
    aln[:, :third] = np.where(u < 0.1, code, aln[:, :third])
    if n >= 8:
        aln[:, 1] = 200
        aln[:, n - 2] = A - 1
        aln[:, n - 1] = A - 1
        aln[T // 2, n - 1] = A
    return aln.astype(np.uint8)
