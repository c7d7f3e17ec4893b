"""Inputs and error bounds of the pair-statistics fixture (tests/golden/pair_stats.npz), a plain helper module imported
by tests/test_pair_stat_fixture.py, tests/test_gpu_pair_stat_edges.py and tests/golden/make_pair_stat_fixture.py.

The fixture pins the statistics of CoMap/Statistics.h:164-329, Distance.h:150-171 and Domain.cpp:113-122 to their
definitions: the generator evaluates them with mpmath (200 digits; 50 pin a double, one pair cancels 60) and rounds once to double.  This module builds the inputs
(deterministically, numpy.random.default_rng) and derives, from the inputs alone, how far an fp64 implementation of the
same formula may be from that value -- whatever order it sums in.

Inputs
------
`CASES` are (B branches, K substitution types, signed): (3,1) (4,1) (5,1) (5,2 signed) (6,2) (7,1) (78,1): every residue
of B mod 4, B <= 4 (one k-step of the Gram kernel), B > 64 (more than one trip of the per-wave loops).  Each case has
`NV` = 19 site vectors counts[19, B, K] (19 is coprime to 16, 64 and 256, the tile sizes of the device paths):

    0-7   Gamma(0.3) * 3 draws (in the signed case the second type is negated on about half the branches)
    8     the zero vector
    9     constant 0.5 in type 0 (its mean is exact: the centred vector is exactly zero)
    10    2^-3 * vector 0          (Correlation = Cosinus = 1, Compensation = 0 in exact arithmetic)
    11    vector 1 * (1 + 1e-9 eps)
    12    vector 2 with 64 added to type 0 (a large mean over a small spread)
    13    totals exactly on thresholds: 1 - 2^-53, 1, 0.99, 0.5, 0, 2, 9999.5, ... (halved over K: the sums are exact)
    14    |vector 6| with one total of exactly 10000 (outside the range of the MI kinds: every pair of it is NaN there)
    15    one-hot
    16    2^-100 * vector 4
    17    2^100 * vector 5
    18    signed case: -vector 3 * (1 + 1e-9 eps); otherwise one more Gamma draw

The draw of a case is repeated with the next sub-seed until every non-degenerate operand has kappa <= 1e3 (below).
Weights are small integers over a power of two with one zero entry: they are normalised exactly and the weighted mean of
the constant vector is exact, so its weighted Correlation is NaN on every path.  CorrectedCorrelation uses one mean vector
(multiples of 1/16) for both operands.

Statistic keys: k0..k7 (the kinds of comap_amd.engine), k8a (DiscreteMI with the bounds {0, 0.5, 1, 2, 1e4}), k8l (the
Label bounds -0.5, 0.5, .., 12.5), sp (scalar product), w0 w1 w3 w4 w6 w7 (the weighted kinds).

Totals.  The per-branch total is the double sum of the K types (VectorTools::sum); with K <= 2 it is one rounding and
does not depend on order.  The indicator kinds (Cosubstitution, the MI kinds) compare that double with their thresholds
and are exact; Compensation and EuclidianDistance are defined on the exact totals and their bounds carry the rounding.

Bounds (u = 2^-53, gamma = (B + 2K + 8) u)
-----------------------------------------
A sum of B products computed in fp64, in any order and with or without fused multiply-adds, is within gamma * (sum of
the absolute terms) of the exact sum of the same operands; the 2K + 8 leave room for the roundings before and after the
sum (the K-sum, a subtraction, a scale factor, square roots, a quotient).

Centring.  d_b = x_b - m with m the mean.  A computed mean m^ = m + e shifts every d_b by the same e, and since
sum_b d_b = 0 (sum_b w_b d_b = 0 with weights), sum (d_b + e)(d'_b + e') = sum d_b d'_b + B e e': the shift enters at
second order only, |e| <= gamma ||x|| / sqrt(B), i.e. relative (gamma kappa)^2 with kappa = ||x|| / ||x - mean||.  What is
first order is the rounding of x_b - m^ itself, u |d_b|.  CorrectedCorrelation first forms z_b = x_b - meanvector_b, one
rounding relative to z_b, which the centring amplifies: u kappa with kappa = ||z|| / ||z - mean||.  So an operand has
eps = c kappa u + (gamma kappa)^2, c = 1 for kind 6 and 0 otherwise.  (A bound linear in B kappa u for every centred
kind cannot meet the sensitivity requirement below at kappa = 1e4; the cancellation above is why it need not.)

* scalar product            gamma A,  A = sum |x_b y_b|
* Covariance                ((gamma + 8u) A + (eps1 + eps2) n1 n2) / (B - 1) + 2u |cov|   (weighted: no B - 1)
* Correlation / Cosinus / CorrectedCorrelation, r = g / (n1 n2):
                            (gamma + 8u) (A / (n1 n2) + |r|) + (eps1 + eps2) (1 + |r|) + 8u |r|
* Compensation, q = n3 / (n1 + n2), a = (K - 1) u (+ 2u with weights: the square root of w_b and the product):
                            a + q (1.5 gamma + a + 3u) + u
  -- the totals are off by a |t|, so ||t1 + t2|| is off by a (n1 + n2) + u n3 whatever n3 is; sqrt halves gamma.  The
  1.5 admits the identity n3^2 = n1^2 + n2^2 + 2 t1.t2 (three sums, absolute terms n1^2 + n2^2 + 2 |t1.t2|) wherever
  it keeps at least half of n1^2 + n2^2: then 2 |t1.t2| <= (n1^2 + n2^2) / 2, the absolute terms are at most 3 n3^2
  and the square root halves that.  Below that half the identity has no bound and the sum has to be taken directly.
* Compensation of a group of m: a + q (gamma + a + (m + 2) u) + u with a = (m K - 1) u (+ 2u).
* EuclidianDistance         a (n1 + n2) + (gamma / 2 + 3u) d
  -- the K-sums round relative to ||t||, not to the distance: near-identical vectors with K = 2 are only this good.
* MI kinds                  (cells + 10) u (1 + sum p |log|) / ln(2.7182818): the cell counts are integers, each term
  carries three roundings of the logarithm's argument and the logarithm's own; k8a / k8l add cells 2^-47 / ln(2.7182818)
  for the 2^-46 fixed point in which mi_pair_wave sums its terms.
* Cosubstitution, every NaN or +-inf reference value, and every value whose bound is 0: compared exactly (0 matches
  -0).  The bound is 0 where the computation is exact on every path: a centred operand that is exactly zero
  (Covariance), a product with the zero vector, Compensation against the zero vector (sum (0 + t)^2 is the same sum as
  sum t^2, so the quotient is exactly 1), an MI table with n_ac B = n_a n_c in every cell (the quotient is exactly 1
  and its logarithm 0).

Observed on the CPU (tests/test_pair_stat_fixture.py asserts <= 0.5): the largest error / bound over the oracle, the
numpy restatements and the candidate-group statistic is 0.222 (oracle.stat_pair, EuclidianDistance, B = 5, K = 2 signed).
"""
import math
import os

import numpy as np

U = 2.0 ** -53
NV = 19
KAPPA_MAX = 1e3
LN_BASE = math.log(2.7182818)
CASES = [(3, 1, False), (4, 1, False), (5, 1, False), (5, 2, True), (6, 2, False), (7, 1, False), (78, 1, False)]
THRESHOLD_TOTALS = [1.0 - 2.0 ** -53, 1.0, 0.99, 0.5, 0.0, 2.0, 9999.5]
BOUNDS_5 = np.array([0.0, 0.99, 10000.0])
BOUNDS_8A = np.array([0.0, 0.5, 1.0, 2.0, 1e4])
BOUNDS_8L = -0.5 + np.arange(4 * 3 + 2, dtype=np.float64)          # engine.label_mi_bounds(4)
MI_BOUNDS = {"k5": BOUNDS_5, "k8a": BOUNDS_8A, "k8l": BOUNDS_8L}
UNWEIGHTED_KEYS = ["k0", "k1", "k2", "k3", "k4", "k5", "k6", "k7", "k8a", "k8l", "sp"]
WEIGHTED_KEYS = ["w0", "w1", "w3", "w4", "w6", "w7"]
KEYS = UNWEIGHTED_KEYS + WEIGHTED_KEYS
GROUP_KEYS = [k for k in KEYS if k != "sp"]
EXACT_KEYS = ("k2",)
# groups of 1, 2, 3, 12 (66 pairs: more than one wave) and 19 members; [9, 8] has no finite pair under Correlation / Cosinus
GROUPS = [[4], [9, 8], [5, 0, 10], [3, 14, 11, 1, 13, 7, 16, 0, 18, 12, 6, 15],
          [7, 2, 18, 11, 0, 15, 9, 4, 13, 6, 17, 1, 10, 8, 3, 16, 5, 14, 12]]
IU = np.triu_indices(NV)                 # the stored entries: upper triangle and diagonal, row order


def case_name(B, K, signed):
    return f"B{B}K{K}" + ("s" if signed else "")


def kind_of(key):
    """engine / oracle kind number of a statistic key (k8a / k8l: 8, sp: 9)"""
    return {"k8a": 8, "k8l": 8, "sp": 9}.get(key, int(key[1]) if key[0] in "kw" else -1)


def weights_raw(B):
    """small integers, one of them 0, that sum to a power of two"""
    w = [(1, 0, 2, 3, 1, 2, 5)[b % 7] for b in range(B - 1)]
    total = 1
    while total <= sum(w):
        total *= 2
    return np.array(w + [total - sum(w)], dtype=np.float64)


def mean_vector(B):
    return np.array([((5 * b + 3) % 11) / 16.0 for b in range(B)])


# ---------------------------------------------------------------------------------------------------- operands
def type0(counts, mv=None):
    x = counts[:, :, 0]
    return x if mv is None else x - mv[None, :]


def totals(counts):
    """the double per-branch totals (VectorTools::sum: in order; one rounding for K = 2)"""
    t = np.zeros(counts.shape[:2])
    for k in range(counts.shape[2]):
        t = t + counts[:, :, k]
    return t


def centred(x, w=None):
    """(scaled centred operand [n, B], kappa [n]) -- kappa = inf where the centred operand is exactly zero"""
    if w is None:
        d = x - (x.sum(1) / x.shape[1])[:, None]
        nx = np.sqrt((x * x).sum(1))
    else:
        f = np.sqrt(w)[None, :]
        d = f * (x - (x * w[None, :]).sum(1)[:, None])
        nx = np.sqrt((w[None, :] * x * x).sum(1))
    nd = np.sqrt((d * d).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(nd > 0, nx / nd, np.inf)
    return d, kappa


def _draw(B, K, signed, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros((NV, B, K))
    g = rng.gamma(0.3, 3.0, size=(9, B, K))
    if signed:
        g[:, :, 1] *= np.where(rng.random(size=(9, B)) < 0.5, -1.0, 1.0)
    c[0:8] = g[0:8]
    c[9, :, 0] = 0.5
    c[10] = c[0] * 2.0 ** -3
    c[11] = c[1] * (1.0 + 1e-9 * rng.standard_normal(size=(B, K)))
    c[12] = c[2]
    c[12, :, 0] += 64.0
    for b in range(B):
        c[13, b, :] = THRESHOLD_TOTALS[b % len(THRESHOLD_TOTALS)] / K
    c[14] = np.abs(c[6])
    c[14, 1, :] = 10000.0 / K
    c[15, B // 2, 0] = 1.0
    c[16] = c[4] * 2.0 ** -100
    c[17] = c[5] * 2.0 ** 100
    c[18] = -c[3] * (1.0 + 1e-9 * rng.standard_normal(size=(B, K))) if signed else g[8]
    return c


class Case:
    """one (B, K, signed): counts [19, B, K], normalised weights w, the raw ones, the mean vector"""

    def __init__(self, B, K, signed):
        self.B, self.K, self.signed, self.name = B, K, signed, case_name(B, K, signed)
        self.w_raw = weights_raw(B)
        self.w = self.w_raw / self.w_raw.sum()
        self.mv = mean_vector(B)
        for attempt in range(200):
            self.counts = _draw(B, K, signed, [20260, B, K, int(signed), attempt])
            if self.max_kappa() <= KAPPA_MAX:
                break
        else:
            raise AssertionError(f"{self.name}: no draw with kappa <= {KAPPA_MAX}")
        self.seed_attempt = attempt

    def kappas(self):
        out = []
        for mv in (None, self.mv):
            for w in (None, self.w):
                out.append(centred(type0(self.counts, mv), w)[1])
        return np.array(out)

    def max_kappa(self):
        k = self.kappas()
        return float(k[np.isfinite(k)].max())

    def expand(self, n, start=0):
        """site i of an n-site input is vector (start + i) % 19 -> (counts [n, B, K], index [n])"""
        idx = (start + np.arange(n)) % NV
        return np.ascontiguousarray(self.counts[idx]), idx


_CASES = {}


def case(B, K, signed):
    key = (B, K, signed)
    if key not in _CASES:
        _CASES[key] = Case(B, K, signed)
    return _CASES[key]


def all_cases():
    return [case(*c) for c in CASES]


# ---------------------------------------------------------------------------------------------------- bounds
def gamma(B, K):
    return (B + 2 * K + 8) * U


def _eps(kappa, g, c):
    k = np.where(np.isfinite(kappa), kappa, 0.0)
    return c * k * U + (g * k) ** 2


def _norms(D):
    return np.sqrt((D * D).sum(1))


def bound_scalar(X1, X2, g):
    return g * (np.abs(X1) @ np.abs(X2).T)


def bound_covariance(D1, k1, D2, k2, g, c, divisor):
    A = np.abs(D1) @ np.abs(D2).T
    nn = _norms(D1)[:, None] * _norms(D2)[None, :]
    cov = (D1 @ D2.T) / divisor
    return ((g + 8 * U) * A + (_eps(k1, g, c)[:, None] + _eps(k2, g, c)[None, :]) * nn) / divisor + 2 * U * np.abs(cov)


def bound_cosine(D1, k1, D2, k2, g, c):
    A = np.abs(D1) @ np.abs(D2).T
    nn = _norms(D1)[:, None] * _norms(D2)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(D1 @ D2.T) / nn
        b = (g + 8 * U) * (A / nn + r) + (_eps(k1, g, c)[:, None] + _eps(k2, g, c)[None, :]) * (1.0 + r) + 8 * U * r
    return np.where(nn > 0, b, 0.0)


def bound_compensation(T1, T2, g, a):
    n1, n2 = _norms(T1)[:, None], _norms(T2)[None, :]
    n3 = np.sqrt(((T1[:, None, :] + T2[None, :, :]) ** 2).sum(2))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(n1 + n2 > 0, n3 / (n1 + n2), 0.0)
    return np.where((n1 == 0) | (n2 == 0), 0.0, a + q * (1.5 * g + a + 3 * U) + U)


def bound_compensation_group(T, g, K, weighted):
    """T: [m, B] totals of the members"""
    m = T.shape[0]
    a = (m * K - 1 + (2 if weighted else 0)) * U
    ns, nj = math.sqrt(float((T.sum(0) ** 2).sum())), float(_norms(T).sum())
    q = ns / nj if nj > 0 else 0.0
    return a + q * (g + a + (m + 2) * U) + U


def bound_euclid(T1, T2, g, a):
    n1, n2 = _norms(T1)[:, None], _norms(T2)[None, :]
    d = np.sqrt(((T2[None, :, :] - T1[:, None, :]) ** 2).sum(2))
    return a * (n1 + n2) + (g / 2 + 3 * U) * d


def classes(T, bounds):
    """Domain::getIndex of every total (-1: out of range)"""
    c = np.searchsorted(bounds, T, side="right") - 1
    c[(T < bounds[0]) | (T >= bounds[-1]) | np.isnan(T)] = -1
    return c


def mi_terms(c1, c2):
    """the joint table of two class vectors -> list of (n_ac, n_a, n_c)"""
    cells = {}
    for a, c in zip(c1.tolist(), c2.tolist()):
        cells[(a, c)] = cells.get((a, c), 0) + 1
    na = {a: int((c1 == a).sum()) for a in set(c1.tolist())}
    nc = {c: int((c2 == c).sum()) for c in set(c2.tolist())}
    return [(n, na[a], nc[c]) for (a, c), n in cells.items()]


def bound_mi(C1, C2, fixed_point):
    B = C1.shape[1]
    out = np.zeros((C1.shape[0], C2.shape[0]))
    for i in range(C1.shape[0]):
        for j in range(C2.shape[0]):
            if (C1[i] < 0).any() or (C2[j] < 0).any():
                continue
            t = mi_terms(C1[i], C2[j])
            if all(n * B == a * c for n, a, c in t):
                continue
            s = sum((n / B) * abs(math.log(n * B / (a * c))) for n, a, c in t)
            out[i, j] = ((len(t) + 10) * U * (1.0 + s) + (len(t) * 2.0 ** -47 if fixed_point else 0.0)) / LN_BASE
    return out


def pair_bounds(cs, key, idx1=None, idx2=None):
    """bound of statistic `key` for every pair (vector idx1[i], vector idx2[j]) of case cs -> [len(idx1), len(idx2)]"""
    full = _pair_bounds_full(cs, key)
    if idx1 is None:
        return full
    return full[np.ix_(idx1, idx1 if idx2 is None else idx2)]


def _pair_bounds_full(cs, key):
    cache = cs.__dict__.setdefault("_bounds", {})
    if key not in cache:
        cache[key] = _compute_pair_bounds(cs, key)
    return cache[key]


def _compute_pair_bounds(cs, key):
    return counts_bounds(key, cs.counts, None, cs.w if key[0] == "w" else None, cs.mv)


def counts_bounds(key, c1, c2=None, w=None, mv=None):
    """bound of statistic `key` for every pair (site i of c1, site j of c2 or of c1) of any counts [n, B, K]; w: normalised
    weights (the w-keys); mv: CorrectedCorrelation's mean vector, or [2, B] for the two operands"""
    c1 = np.asarray(c1, dtype=np.float64)
    c2 = c1 if c2 is None else np.asarray(c2, dtype=np.float64)
    B, K = c1.shape[1], c1.shape[2]
    g, kind, weighted = gamma(B, K), kind_of(key), w is not None
    if key in MI_BOUNDS:
        return bound_mi(classes(totals(c1), MI_BOUNDS[key]), classes(totals(c2), MI_BOUNDS[key]), key != "k5")
    if kind == 2:
        return np.zeros((len(c1), len(c2)))
    if kind in (0, 4, 6):
        mv = np.asarray(mv).reshape(-1, B) if kind == 6 else [None]
        (D1, k1), (D2, k2) = centred(type0(c1, mv[0]), w), centred(type0(c2, mv[-1]), w)
        c = 1.0 if kind == 6 else 0.0
        if kind == 4:
            return bound_covariance(D1, k1, D2, k2, g, c, 1.0 if weighted else B - 1.0)
        return bound_cosine(D1, k1, D2, k2, g, c)
    if kind == 3:
        X1, X2 = (type0(c) * (w[None, :] if weighted else 1.0) for c in (c1, c2))
        return bound_cosine(X1, np.zeros(len(X1)), X2, np.zeros(len(X2)), g, 0.0)
    if kind == 9:
        return bound_scalar(type0(c1), type0(c2), g)
    T1, T2 = (totals(c) * (np.sqrt(w)[None, :] if weighted else 1.0) for c in (c1, c2))
    a = (K - 1 + (2 if weighted else 0)) * U
    return bound_compensation(T1, T2, g, a) if kind == 1 else bound_euclid(T1, T2, g, a)


def check_two(a, b, bound, what=""):
    """two fp64 implementations of one statistic, each within `bound` of its exact value: |a - b| <= 2 bound, the same
    NaNs, and equality where the bound is 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN pattern differs"
    ok = ~np.isnan(b)
    return check(a[ok], b[ok], 2.0 * np.broadcast_to(bound, b.shape)[ok], what)


def natural_scale(cs, key):
    """the size a value of statistic `key` has when nothing cancels, per pair [19, 19]: 1 for the normalised kinds, 1/4
    for DiscreteMI and 2 with bounds (up to 16 cells, each within 2^-47 in the fixed point), n1 n2 (/ (B - 1)) for the scalar product and Covariance, n1 + n2
    for EuclidianDistance"""
    kind, weighted = kind_of(key), key[0] == "w"
    w = cs.w if weighted else None
    if kind == 4:
        n = _norms(centred(type0(cs.counts), w)[0])
        return n[:, None] * n[None, :] / (1.0 if weighted else cs.B - 1.0)
    if kind == 9:
        n = _norms(type0(cs.counts))
        return n[:, None] * n[None, :]
    if kind == 7:
        n = _norms(totals(cs.counts) * (np.sqrt(w)[None, :] if weighted else 1.0))
        return n[:, None] + n[None, :]
    return np.full((NV, NV), {"k5": 0.25, "k8a": 2.0, "k8l": 2.0}.get(key, 1.0))


def group_bound(cs, key, members, ref_pairs):
    """bound of getValueForGroup: Compensation's closed form, or -- the minimum of values each within its bound of the
    pair's reference is within the largest of those bounds of the minimum of the references -- the largest pair bound"""
    kind, weighted = kind_of(key), key[0] == "w"
    if kind == 1:
        T = totals(cs.counts[members]) * (np.sqrt(cs.w)[None, :] if weighted else 1.0)
        return bound_compensation_group(T, gamma(cs.B, cs.K), cs.K, weighted)
    b = pair_bounds(cs, key)
    worst = 0.0
    for i in range(1, len(members)):
        for j in range(i):
            if np.isfinite(ref_pairs[members[i], members[j]]):
                worst = max(worst, float(b[members[i], members[j]]))
    return worst


# ---------------------------------------------------------------------------------------------------- the fixture
def full_matrix(tri):
    """[190] stored entries -> symmetric [19, 19]"""
    m = np.zeros((NV, NV))
    m[IU] = tri
    m.T[IU] = tri
    return m


def load(path):
    """-> {case name: {key: [19, 19], "g_" + key: [len(GROUPS)], "counts": ...}}; checks that the stored inputs are the ones
    this module builds"""
    z = np.load(path)
    out = {}
    for cs in all_cases():
        assert np.array_equal(z[cs.name + ".counts"], cs.counts), cs.name + ": the fixture was made from other inputs"
        assert np.array_equal(z[cs.name + ".w"], cs.w_raw) and np.array_equal(z[cs.name + ".mv"], cs.mv)
        d = {"counts": cs.counts}
        for k in KEYS:
            d[k] = full_matrix(z[f"{cs.name}.{k}"])
        for k in GROUP_KEYS:
            d["g_" + k] = z[f"{cs.name}.g_{k}"]
        out[cs.name] = d
    return out


_FIXTURE = []


def fixture():
    """the committed fixture, loaded once"""
    if not _FIXTURE:
        _FIXTURE.append(load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_stats.npz")))
    return _FIXTURE[0]


def ratio(got, ref, bound):
    """error / bound, elementwise.  NaN and +-inf references and every entry whose bound is 0 must be met exactly: ratio 0
    where they are, inf where they are not."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    exact = ~np.isfinite(ref) | (bound == 0.0)
    same = (np.isnan(got) & np.isnan(ref)) | (got == ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - ref) / bound
    r = np.where(exact, np.where(same, 0.0, np.inf), r)
    return np.where(np.isnan(r), np.inf, r)


def check(got, ref, bound, what=""):
    """assert that got is within bound of ref (see ratio); returns the largest error / bound"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(ref), (what, got.shape, np.shape(ref))
    r = ratio(got, ref, bound)
    worst = float(r.max()) if r.size else 0.0
    if worst > 1.0:
        at = np.unravel_index(int(np.argmax(r)), r.shape) if r.ndim else ()
        raise AssertionError(f"{what}: error / bound = {worst:.3g} at {at}: got {got[at]!r}, reference {np.asarray(ref)[at]!r}, "
                             f"bound {np.broadcast_to(bound, r.shape)[at]:.3g}; {int((r > 1).sum())} of {r.size} entries out")
    return worst


# ---------------------------------------------------------------------------------------------------- plain vectors
def vector_matrix_reference(kind, X, Y=None):
    """AnalysisTools::compute{ScalarProduct,Cosinus,Correlation,Covariance}Matrix (AnalysisTools.cpp:102-339) by brute force:
    means with math.fsum (exact sum of doubles), everything else in np.longdouble (64-bit significand: each operation is
    2^-11 of a double's rounding).  One set: matrix[i][i] = 1 for Cosinus / Correlation (:178, :236), f(v_i, v_i) for the
    other two, and the lower triangle mirrors the upper one."""
    L = np.longdouble
    one = Y is None
    Y = X if one else Y

    def operand(V):
        V = np.asarray(V, dtype=np.float64)
        if kind in (0, 4):
            return np.array([[L(x) - L(math.fsum(v)) / L(len(v)) for x in v] for v in V], dtype=L)
        return V.astype(L)
    A, Bm = operand(X), operand(Y)
    dim = A.shape[1]
    out = np.zeros((len(A), len(Bm)))
    for i in range(len(A)):
        for j in range(len(Bm)):
            g = (A[i] * Bm[j]).sum()
            if kind == 9:
                v = g
            elif kind == 4:
                v = g / L(dim - 1)
            else:
                den = np.sqrt((A[i] * A[i]).sum()) * np.sqrt((Bm[j] * Bm[j]).sum())
                v = g / den if den != 0 else L(np.nan)
            out[i, j] = float(v)
    if one:
        for i in range(len(A)):
            if kind in (0, 3):
                out[i, i] = 1.0
            for j in range(i):
                out[i, j] = out[j, i]
    return out


def vector_matrix_bounds(kind, X, Y=None):
    """the bounds above for plain vectors (B = the vector length, K = 1)"""
    X = np.asarray(X, dtype=np.float64)
    Y = X if Y is None else np.asarray(Y, dtype=np.float64)
    g = gamma(X.shape[1], 1)
    if kind == 9:
        return bound_scalar(X, Y, g)
    if kind == 3:
        return bound_cosine(X, np.zeros(len(X)), Y, np.zeros(len(Y)), g, 0.0)
    (D1, k1), (D2, k2) = centred(X), centred(Y)
    if kind == 4:
        return bound_covariance(D1, k1, D2, k2, g, 0.0, X.shape[1] - 1.0)
    return bound_cosine(D1, k1, D2, k2, g, 0.0)
