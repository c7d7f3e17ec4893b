"""Hand-worked cases that pin tests/window_reference.py (the restatement of R/CoMapFunctions.R:168-215 the GPU tests compare
with) and comap_amd/pvalues.py (format.pred's pairwise branch, :485-517).  No GPU."""
import numpy as np

from comap_amd import pvalues
from window_reference import window_half_width, window_test

NMIN = [0.0, 1.0, 2.0, 3.0, 4.0]
STAT = [0.1, 0.5, 0.3, 0.9, 0.7]


def _one(s, m, **kw):
    pv, cnt, nobs = window_test(STAT, NMIN, [s], [m], 0.5, **kw)
    return pv[0], int(cnt[0]), int(nobs[0])


def test_worked_example():
    kept, ws = window_half_width(STAT, NMIN, 0.5)
    assert kept.all() and ws == 1.0
    # (1, 3) strict holds nmin 2 alone: stat .3 < .4
    assert _one(0.4, 2.0) == (0.5, 0, 1)
    # (1.5, 3.5) holds nmin 2 and 3: stats .3 and .9
    assert _one(0.4, 2.5) == (2.0 / 3.0, 1, 2)
    assert _one(0.4, 2.0, lower=True) == (1.0, 1, 1)
    # the conserved rule wins over min_nobs (the reference tests nmin < 0.01 first): window (-0.995, 1.005) holds nmin 0 and 1
    pv, cnt, nobs = _one(0.9, 0.005, min_nobs=50)
    assert pv == 1.0 and nobs == 2
    pv, cnt, nobs = window_test(STAT, NMIN, [0.9], [0.005], 0.5 * 0.99)    # ws = 0.99: (-0.985, 0.995) holds nmin 0 alone
    assert pv[0] == 1.0 and nobs[0] == 1
    pv, cnt, nobs = _one(0.4, 9.0)
    assert np.isnan(pv) and (cnt, nobs) == (0, 0)


def test_min_nobs_boundary():
    pv, cnt, nobs = _one(0.4, 2.5, min_nobs=3)      # nobs = min_nobs - 1
    assert np.isnan(pv) and (cnt, nobs) == (1, 2)
    assert _one(0.4, 2.5, min_nobs=2) == (2.0 / 3.0, 1, 2)   # nobs = min_nobs


def test_nan_rules_and_dropped_entries():
    ns, nm = STAT + [np.nan, 0.2], NMIN + [2.0, np.nan]      # both extra entries are dropped: nothing changes
    kept, ws = window_half_width(ns, nm, 0.5)
    assert kept.tolist() == [True] * 5 + [False] * 2 and ws == 1.0
    pv, cnt, nobs = window_test(ns, nm, [0.4, np.nan, 0.4, np.nan], [2.5, 2.5, np.nan, 0.005], 0.5)
    assert pv[0] == 2.0 / 3.0 and np.isnan(pv[1]) and np.isnan(pv[2]) and pv[3] == 1.0
    assert cnt.tolist() == [1, 0, 0, 0] and nobs.tolist() == [2, 2, 0, 2]
    pv, cnt, nobs = window_test([np.nan], [1.0], [0.4], [1.0], 0.5)
    assert np.isnan(pv[0]) and nobs[0] == 0
    pv, cnt, nobs = window_test([], [], [0.4], [0.001], 0.5)
    assert pv[0] == 1.0 and nobs[0] == 0


P8 = np.array([0.001, 0.008, 0.03, 0.0125, 1.0, np.nan, 0.0099, 0.045])
NOBS8 = np.array([10, 10, 10, 10, 3, 0, 10, 10])


def test_benjamini_hochberg_by_hand():
    # nbtests: rows 0 1 2 3 6 7 (row 4 has a p-value, the conserved 1, but nobs 3 < 5; row 5 has none) = 6
    # kept and sorted: .001 .008 .0099 .0125 .03 .045 against k * .02 / 6 = .00333 .00667 .01 .01333 .01667 .02
    #                   yes   no   yes    yes    no   no   -> t = x[4] = .0125; the .008 row is flagged too (step-up)
    t, nbtests, flags = pvalues.benjamini_hochberg(P8, NOBS8, 5, level=0.05, fdr=0.02)
    assert nbtests == 6 and t == 0.0125
    assert flags.tolist() == [True, True, False, True, False, False, True, False]
    # counting every row with a p-value (7) would give .00286 .00571 .00857 .01143 ..: t = .001
    t7, _, _ = pvalues.benjamini_hochberg(P8, np.full(8, 10), 5, level=0.05, fdr=0.02)
    assert t7 == 0.001


def test_benjamini_hochberg_without_a_passing_rank():
    t, nbtests, flags = pvalues.benjamini_hochberg(P8, NOBS8, 5, level=0.05, fdr=0.0001)    # .001 > 1 * .0001 / 6
    assert t == 0.0 and nbtests == 6 and not flags.any()
    t, nbtests, flags = pvalues.benjamini_hochberg([np.nan, 0.5], [0, 9], 1, level=0.05, fdr=0.05)   # nothing at the level
    assert t == 0.0 and nbtests == 1 and not flags.any()


def test_window_predictions_drop_rows_without_a_p_value():
    keep, p, nobs = pvalues.window_predictions(P8, NOBS8)
    assert keep.tolist() == [0, 1, 2, 3, 4, 6, 7] and p.tolist() == P8[keep].tolist() and nobs.tolist() == NOBS8[keep].tolist()
