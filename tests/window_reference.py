"""Brute-force restatement of the "exact procedure" of `test` in the reference's R/CoMapFunctions.R:168-215 (what get.pred runs:
grid.Rate = FALSE), in numpy, O(nq * nnull).  A helper of the window tests, pinned by tests/test_window_reference.py.

R lines:  ws <- (max(sim[, Nmin]) - min(sim[, Nmin])) * window / 2                                  (:172)
          d  <- sim[sim[, Nmin] > nmin - ws & sim[, Nmin] < nmin + ws, ]                            (:182)
          nmin < 0.01 -> p = 1;  nrow(d) < min.nobs -> NA;  (sum(d[, Stat] >= stat) + 1) / (nrow(d) + 1), lower: <=   (:183-208)
          nobs = nrow(d)                                                                            (:211)
Kept null entries: neither value NaN.  A NaN query statistic: count 0, p NaN unless the conserved rule gave 1.  A NaN query Nmin:
nobs = count = 0, p NaN."""
import numpy as np


def window_half_width(null_stat, null_nmin, window):
    """-> (kept mask, ws); ws = 0.0 when nothing is kept"""
    ns, nm = np.asarray(null_stat, dtype=np.float64), np.asarray(null_nmin, dtype=np.float64)
    kept = ~(np.isnan(ns) | np.isnan(nm))
    if not kept.any():
        return kept, 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        ws = (np.float64(nm[kept].max()) - np.float64(nm[kept].min())) * np.float64(window) / np.float64(2.0)
    return kept, float(ws)


def window_test(null_stat, null_nmin, stat, nmin, window, min_nobs=1, lower=False, conserved_nmin=0.01):
    """-> (pvalue float64, count uint32, nobs uint32), one entry per query"""
    ns, nm = np.asarray(null_stat, dtype=np.float64).ravel(), np.asarray(null_nmin, dtype=np.float64).ravel()
    s, m = np.asarray(stat, dtype=np.float64).ravel(), np.asarray(nmin, dtype=np.float64).ravel()
    kept, ws = window_half_width(ns, nm, window)
    ns, nm = ns[kept], nm[kept]
    nq = len(s)
    pv, cnt, nobs = np.full(nq, np.nan), np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    ws = np.float64(ws)
    with np.errstate(invalid="ignore"):
        for q in range(nq):
            if not np.isnan(m[q]):
                inside = (nm > m[q] - ws) & (nm < m[q] + ws)
                nobs[q] = np.count_nonzero(inside)
                if not np.isnan(s[q]):
                    d = ns[inside]
                    cnt[q] = np.count_nonzero(d <= s[q]) if lower else np.count_nonzero(d >= s[q])
            if m[q] < conserved_nmin:
                pv[q] = 1.0
            elif not np.isnan(m[q]) and nobs[q] >= min_nobs and not np.isnan(s[q]):
                pv[q] = np.float64(int(cnt[q]) + 1) / np.float64(int(nobs[q]) + 1)
    return pv, cnt, nobs
