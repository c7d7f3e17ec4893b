"""TEST INFRASTRUCTURE ONLY: the clustering kernel's case table ("Clustering stage at every kernel shape").

hclust_kernel<LINK, PER> keeps PER = 1, 2, 4, 6 or 10 columns of a row per thread (n <= 512, 1024, 2048, 3072, 5000).
Every class boundary is run from both sides with random and tie-heavy matrices, and the bottom n of each class with the
matrices built to stress the lazy row minima over several 512-column rescan segments.  All matrices come from
np.random.default_rng, are symmetric and have a zero diagonal.  reference() caches hclust_fast's answer per case;
check_preconditions() asserts from its counters that a case does what it was built for."""
import functools

import numpy as np

from oracle import cluster as oc
import cluster_reference as cr

LINKS = (oc.LINK_COMPLETE, oc.LINK_SINGLE, oc.LINK_AVERAGE)
LINK_NAME = {oc.LINK_COMPLETE: "complete", oc.LINK_SINGLE: "single", oc.LINK_AVERAGE: "average"}
CLASSES = {"per1-2": (512, 513), "per2-4": (1024, 1025), "per4-6": (2048, 2049), "per6-10": (3072, 3073)}
LIMIT = 5000
NAN_ROWS = 3


def _sym(u):
    d = np.triu(u, 1)
    return d + d.T


def random_matrix(n, seed):
    return _sym(np.random.default_rng(seed).random((n, n)))


def _tie_values(rng, n):
    """integer distances in {1, 2, 3}, about four 1s per row: most steps have several closest pairs, and the closest pair of
    a row lies anywhere in it.  (With the three values equally likely, single linkage grows one cluster from row 0 and its
    next column and never loses a cached neighbour.)"""
    p1 = min(1.0 / 3.0, 4.0 / n)
    return rng.choice([1.0, 2.0, 3.0], p=[p1, (1 - p1) / 2, (1 - p1) / 2], size=(n, n))


def tie_matrix(n, seed):
    return _sym(_tie_values(np.random.default_rng(seed), n))


def _nan_rows(n, rng):
    """row 0, one row with index > 512 (n = 513 has none: its last row, 512), one more"""
    return [0, int(rng.integers(min(513, n - 1), n)), int(rng.integers(1, 512))]


def holes_matrix(n, seed):
    """three NaN rows/columns (see _nan_rows) and ten entries given as +inf instead.  The ten lie in the NaN rows: a +inf
    between two ordinary sites keeps their clusters apart to the end under complete and average linkage, which adds +inf
    joins beyond the NaN rows' (scatter_matrix has those)"""
    rng = np.random.default_rng(seed)
    d = _sym(rng.random((n, n)))
    rows = _nan_rows(n, rng)
    for r in rows:
        d[r, :] = d[:, r] = np.nan
        d[r, r] = 0.0
    for q in range(10):
        r = rows[q % NAN_ROWS]
        c = int(rng.integers(0, n))
        if c != r:
            d[r, c] = d[c, r] = np.inf
    return d


def scatter_matrix(n, seed):
    """ten +inf entries between ordinary sites of a random matrix, one end left and one right of the first segment"""
    rng = np.random.default_rng(seed)
    d = _sym(rng.random((n, n)))
    for q in range(10):
        a, b = int(rng.integers(0, 512)), int(rng.integers(512, n))
        d[a, b] = d[b, a] = np.inf
    return d


def nan_matrix(n, seed):
    return np.full((n, n), np.nan)


def two_block_matrix(n, seed):
    """even and odd indices form two blocks: ties (_tie_values) inside a block, larger and pairwise distinct distances
    between the blocks, so a row's neighbour is routinely more than a segment away"""
    rng = np.random.default_rng(seed)
    d = _tie_values(rng, n)
    idx = np.arange(n)
    between = (idx[:, None] + idx[None, :]) % 2 == 1
    nb = int(np.count_nonzero(np.triu(between, 1)))
    d[np.triu(between, 1)] = 10.0 + rng.permutation(nb) / nb
    return _sym(d)


BUILDERS = {"random": random_matrix, "ties": tie_matrix, "holes": holes_matrix, "scatter": scatter_matrix, "allnan": nan_matrix,
            "twoblock": two_block_matrix}


def _table():
    """[(class, n, input, linkage)]"""
    rows = []
    for cls, (top, bottom) in CLASSES.items():
        for n in (top, bottom):
            for kind in ("random", "ties"):
                rows += [(cls, n, kind, link) for link in LINKS]
        for kind in ("holes", "allnan", "twoblock", "scatter"):
            rows += [(cls, bottom, kind, link) for link in LINKS]
    rows += [("limit", LIMIT, "ties", oc.LINK_COMPLETE), ("limit", LIMIT, "random", oc.LINK_AVERAGE),
             ("limit", LIMIT, "random", oc.LINK_SINGLE)]
    return rows


CASES = _table()


def case_id(case):
    cls, n, kind, link = case
    return f"{cls}-{n}-{kind}-{LINK_NAME[link]}"


@functools.lru_cache(maxsize=None)
def matrix(n, kind):
    d = BUILDERS[kind](n, 1000 * n + sorted(BUILDERS).index(kind))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(n, kind, link):
    """(merge, dmax, size, counters) of hclust_fast, computed once per process and left unchanged"""
    out = cr.hclust_fast(matrix(n, kind), link)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def check_preconditions(case):
    """what each designed case is for, from the reference's counters"""
    cls, n, kind, link = case
    cnt = reference(n, kind, link)[3]
    steps = n - 1
    if kind == "ties":
        assert 2 * cnt["ties"] > steps, (case_id(case), cnt)
    if kind in ("ties", "twoblock") and n > 512:
        # a row has more than a segment of columns right of its diagonal only from n = 514 on; at n = 513 the kernel's
        # second segment exists and is always empty, and the rescans themselves are what the case is for
        assert cnt["spanning" if n - 1 > cr.SEGMENT else "rescans"] >= 100, (case_id(case), cnt)
    if kind == "holes":
        assert cnt["inf_joins"] == NAN_ROWS, (case_id(case), cnt)
    if kind == "allnan":
        assert cnt["inf_joins"] == steps and cnt["ties"] == steps - 1, (case_id(case), cnt)
    if kind == "scatter":   # single linkage joins round a missing distance; the other two carry it to the last joins
        assert (cnt["inf_joins"] == 0) == (link == oc.LINK_SINGLE), (case_id(case), cnt)


# ---- group properties (cluster_props_kernel): inputs, and the tolerances of Stat and Nmin

WIDE_TREES = {"B77": 40, "B277": 140}      # taxa -> branches 2T - 3: thread-per-branch sums in (64, 256] and above 256
WIDE_SITES, WIDE_K = 40, 2
LARGE_SITES = (2049, LIMIT)
LARGE_TAXA, LARGE_TREE_SEED = 6, 2


def wide_tree(name):
    from comap_amd import synthetic
    return synthetic.random_tree(WIDE_TREES[name], 20 + WIDE_TREES[name])


@functools.lru_cache(maxsize=None)
def wide_counts(name):
    """signed counts [WIDE_SITES, B, WIDE_K]"""
    B = len(wide_tree(name)[0]) - 1
    c = np.random.default_rng(7 * B).uniform(-1.0, 1.0, size=(WIDE_SITES, B, WIDE_K))
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def large_counts(n):
    from comap_amd import synthetic
    B = len(synthetic.random_tree(LARGE_TAXA, LARGE_TREE_SEED)[0]) - 1
    c = np.random.default_rng(n).random((n, B, 1))
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def wide_tree_of(name, dist, link):
    """the oracle's tree of wide_counts: (merge, dmax, size)"""
    return cr.hclust_fast(oc.distance_matrix(dist, wide_counts(name)), link)[:3]


def measure_props_error(dist, merge, dmax, counts):
    """largest absolute distance of the engine's form in fp64 (cluster_reference.props_restated) from the 50-digit values:
    (Stat over the tree's nodes, Nmin as the largest error of any site's norm, which bounds every node's)"""
    stat, _ = cr.props_restated(dist, merge, dmax, counts)
    stat_x, _ = cr.group_properties_exact(dist, merge, dmax, counts)
    return float(np.abs(stat - stat_x).max()), float(np.abs(cr.host_norm(counts) - cr.exact_norm(counts)).max())


# measure_props_error on these very inputs (tests/test_cluster_reference.py keeps the table honest): the restated form's
# error, NOT the device's.  A tolerance is ten times the tabled error, and never below FLOOR_UNITS * 2^-53 of the
# quantity's scale (1 for Stat = 1 - x with x near 1, hence absolute; the largest norm for Nmin), so that a case the
# restatement happens to get exactly right is not held to zero.
FLOOR_UNITS = 4
STAT_ERR = {"B77": 1.6653345369377348e-16, "B277": 3.3306690738754696e-16}      # compensation, the same under every linkage
NORM_ERR = {"B77": 1.7763568394002505e-15, "B277": 1.0658141036401503e-14, 2049: 4.440892098500626e-16,
            LIMIT: 4.440892098500626e-16}


def stat_bound(key):
    return max(10.0 * STAT_ERR[key], FLOOR_UNITS * 2.0 ** -53)


def nmin_bound(key, counts):
    return max(10.0 * NORM_ERR[key], FLOOR_UNITS * 2.0 ** -53 * max(1.0, float(cr.host_norm(counts).max())))
