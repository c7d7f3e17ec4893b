"""What the reference's R scripts do with the window p-values, on the host in plain numpy (R/CoMapFunctions.R).

  window_predictions   <- get.pred (:429-438): the rows that keep a p-value
  benjamini_hochberg   <- format.pred's pairwise branch (:485-517): level filter, Benjamini-Hochberg threshold, FDR flag
The p-values themselves come from the device (engine.window_test*, pipeline.IntraAnalysis.compute_intra_window).  Not restated:
round.pval, the Const column, the nested-group correction (ernest, build.cliques) and fdrcalc of the clustering branch."""
import numpy as np


def window_predictions(pvalue, nobs):
    """get.pred: pred[!is.na(pred$p.value), ] -> (indices of the kept rows, their p-values, their nobs)"""
    pvalue, nobs = np.asarray(pvalue, dtype=np.float64).ravel(), np.asarray(nobs).ravel()
    keep = np.flatnonzero(~np.isnan(pvalue))
    return keep, pvalue[keep], nobs[keep]


def benjamini_hochberg(pvalue, nobs, min_nobs, level=0.05, fdr=0.05):
    """format.pred on pairs.  nbtests = #{p not NaN and nobs >= min_nobs} (:485, on get.pred's rows); the rows with
    p <= level are kept and sorted ascending (level None, R's NA: every row with a p-value); t = the largest x[k] with
    x[k] <= k * fdr / nbtests, k = 1 .. over the kept list, or 0 when there is none (:513-515); flag = p <= t (:517).
    -> (t, nbtests, flags): flags is a bool array over all input rows, False where the row was not kept"""
    pvalue, nobs = np.asarray(pvalue, dtype=np.float64).ravel(), np.asarray(nobs).ravel()
    has_p = ~np.isnan(pvalue)
    nbtests = int(np.count_nonzero(has_p & (nobs >= min_nobs)))
    kept = has_p if level is None else has_p & (pvalue <= level)
    x = np.sort(pvalue[kept])
    t = 0.0
    if len(x):
        with np.errstate(divide="ignore"):   # nbtests = 0 (only conserved rows left): R divides by it too, every row passes
            ok = np.flatnonzero(x <= np.arange(1, len(x) + 1) * fdr / np.float64(nbtests))
        if len(ok):
            t = float(x[ok[-1]])
    return t, nbtests, kept & (pvalue <= t)
