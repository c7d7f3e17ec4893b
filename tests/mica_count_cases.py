"""The cases of tests/golden/mica_counts.npz: Mica's column mutual information for 4 and 20 states at the taxon counts where
launch_mi_columns (comap_amd/csrc/cmx_mica.hip, mica_path) changes kernels, with the columns on which a count table can go
wrong.  A plain helper module (numpy only) shared by the fixture's generator (tests/golden/make_mica_count_fixture.py),
tests/test_mica_count_edges.py (CPU) and tests/test_gpu_mica_count_edges.py.

Per alphabet ONE pair of alignments is drawn at 2 049 taxa; the case of T taxa takes its first T, so a wrong T or a taxon
dropped or counted twice at a k-step boundary shows against the neighbouring case.

    taxa (padded to 32)    proteins                                  nucleotides
    1 .. 64                four-wave kernel, 2 k-steps               four-wave kernel, 2 k-steps
    65 .. 128              4 k-steps                                 4 k-steps
    129 .. 256             8 k-steps                                 8 k-steps
    257 .. 512             16 k-steps (one workgroup per CU)         mica_mfma_kernel<4> (one column per tile)
    513 .. 2047            eight-wave mica_mfma3_kernel              mica_mfma_kernel<4>
    >= 2048                LDS-table kernel alone                    LDS-table kernel alone

Every grid case ("a20-t257") carries on BOTH sides (the first side's operands live in registers, twelve columns of a
workgroup; the second's in the operand image, three columns of a tile): columns with signal, clean and with unknowns (code A
and code 200, which has no mask entry), a constant column of state 0 and one of state A - 1, an all-unknown column, a column
with exactly one unknown, one unknown in every taxon but one, a two-state column split 1 : T - 1, a copy and a
state-permuted copy of the first side's column 0 (MI = H), a column with a partial ambiguity code (code A + 1 = states
{0, 2}: its pairs go to the LDS-table kernel) and, where A^2 divides T, a column whose joint table with the other side's is
exactly uniform (MI = 0, Hjoint = ln A^2, all A^2 cells live).  "-one" is 1 x 1 column, "-two" the intra form with two.

Three designed protein cases (their preconditions are asserted from the integer tables in tests/test_mica_count_edges.py):

    a20-t256-queue, a20-t512-queue   the weighted four-wave instantiation's queue of cells of m >= 4 096 at the most that
        whole taxa can give: 23 (46) blocks of 11 - 12 taxa, the first side's state by block % 20, the second's by
        block * 20 / blocks (all (a, b) distinct), states permuted per column: 23 (46) such cells per pair, nine pairs per
        wave and tile = 207 of 232 (414 of 464) slots.  The unknowns sit in OTHER columns of the same twelve, so the
        weighted instantiation takes the tile while the nine pairs keep whole counts.  Those other columns are the three
        pairs whose tables hold a cell of m = 4 095, 4 096, 4 097 (N_ab = 10, N_aG + N_Gb = 4, N_GG = 15, 16, 17): the last
        entry of f2 in LDS, the first two gathered from global memory; 8 k-steps at 256 taxa, 16 at 512.
    a20-t2047-dump16   the eight-wave kernel's 16-bit dump of the accumulators: constant columns with one unknown each
        (cells of 2 045 and 2 046 taxa, m near 400 x 2 047) and all-unknown x all-unknown (every cell m = T).
"""
import functools
import hashlib

import numpy as np

TMAX = 2049
FAR = 200                    # a code without a mask entry: an unknown
TAXA = {20: [1, 2, 33, 64, 65, 128, 129, 256, 257, 400, 512, 513, 2000, 2047, 2048, 2049],
        4: [1, 2, 33, 64, 65, 128, 129, 256, 257, 512, 2047, 2048, 2049]}
UNIFORM = {20: (400, 2000), 4: (256, 512)}
NSIGNAL = {1: (12, 8), 2: (2, 2)}             # per side: clean, with unknowns
PARTIAL_MASK = 0b101
kMicaLdsF2 = 4096                             # cmx_device.h: entries of f2 the weighted four-wave kernel keeps in LDS


def masks_of(A):
    """the table handed to the engine: A + 2 entries, code A the unknown, code A + 1 partial; longer codes have no entry"""
    m = np.zeros(A + 2, dtype=np.uint32)
    m[:A] = 1 << np.arange(A, dtype=np.uint32)
    m[A] = (1 << A) - 1
    m[A + 1] = PARTIAL_MASK
    return m


def mask_table(A):
    """all 256 codes as the engine completes them: no entry = unknown"""
    m = np.full(256, (1 << A) - 1, dtype=np.uint32)
    m[: A + 2] = masks_of(A)
    return m


def state_permutation(A):
    return (3 * np.arange(A) + 1) % A          # 3 is coprime to 4 and to 20


@functools.lru_cache(maxsize=None)
def _shared(A):
    rng = np.random.default_rng(7000 + A)
    base = rng.integers(0, A, size=(TMAX, 1))
    out = {}
    for side, p in ((1, 0.6), (2, 0.4)):
        n = sum(NSIGNAL[side])
        out[side] = (np.where(rng.random((TMAX, n)) < p, base, rng.integers(0, A, size=(TMAX, n))), rng.random((TMAX, n)))
    return out


def _side(A, T, side, uniform):
    """-> ([T, n] uint8, {name: column})"""
    sig, u = _shared(A)[side]
    nclean = NSIGNAL[side][0]
    col0 = _shared(A)[1][0][:T, 0]
    cols, names = [], []

    def add(name, c):
        names.append(name)
        cols.append(np.broadcast_to(np.asarray(c), (T,)).astype(np.uint8))

    for k in range(sig.shape[1]):
        c = sig[:T, k].copy()
        if k >= nclean:
            c[u[:T, k] < 0.06] = A
            c[(u[:T, k] >= 0.06) & (u[:T, k] < 0.12)] = FAR
        add(("clean%d" if k < nclean else "gapped%d") % k, c)
    add("const0", 0)
    add("constlast", A - 1)
    add("allunknown", A if side == 1 else FAR)
    c = sig[:T, min(1, nclean - 1)].copy()
    c[T // 2] = A
    add("oneunknown", c)
    c = np.full(T, FAR if side == 1 else A)
    c[min(3, T - 1)] = 1
    add("allbutone", c)
    c = np.full(T, 2)
    c[T - 1] = 1
    add("split", c)
    add("copy", col0)
    add("permuted", state_permutation(A)[col0])
    c = sig[:T, min(2, nclean - 1)].copy()
    c[[0, T // 2, T - 1]] = A + 1
    if T > 3:
        c[T // 3] = A
    add("partial", c)
    if uniform:
        t = np.arange(T)
        add("uniform", t % A if side == 1 else (t // A) % A)
    # the special columns scattered among the others; column 0 stays (the copies are copies of the first side's)
    order = np.concatenate([[0], 1 + np.random.default_rng(100 * A + side).permutation(len(cols) - 1)])
    aln = np.stack([cols[k] for k in order], axis=1)
    return np.ascontiguousarray(aln), {names[k]: p for p, k in enumerate(order)}


def _listed(n1, n2, idx1, idx2, extra=()):
    """pairs for mi_pairs, valid against the second side and against the first itself: i = j, a pair twice, the designed ones"""
    lim = min(n1, n2)
    pairs = [(0, 0), (min(1, n1 - 1), min(2, lim - 1)), (min(1, n1 - 1), min(2, lim - 1)), (n1 - 1, lim - 1), (n1 - 1, 0)]
    for name in ("allunknown", "const0", "constlast", "copy", "permuted", "partial", "uniform", "oneunknown", "allbutone", "split"):
        if name in idx1 and name in idx2:
            pairs.append((idx1[name], idx2[name]))
    if "copy" in idx2:
        pairs += [(0, idx2["copy"]), (0, idx2["permuted"])]
    pairs += list(extra)
    assert all(i < n1 and j < lim for i, j in pairs)
    return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64)


def _grid(A, T):
    uniform = T in UNIFORM[A]
    a1, idx1 = _side(A, T, 1, uniform)
    a2, idx2 = _side(A, T, 2, uniform)
    i1, i2 = _listed(a1.shape[1], a2.shape[1], idx1, idx2)
    return dict(A=A, T=T, a1=a1, a2=a2, idx1=idx1, idx2=idx2, i1=i1, i2=i2, kind="grid")


def _tiny(A, T, n1):
    g = _grid(A, T)
    a1 = np.ascontiguousarray(g["a1"][:, [g["idx1"]["clean0"], g["idx1"]["gapped%d" % NSIGNAL[1][0]]][:n1]])
    a2 = np.ascontiguousarray(g["a2"][:, [g["idx2"]["gapped%d" % NSIGNAL[2][0]]]])
    return dict(A=A, T=T, a1=a1, a2=a2, idx1={}, idx2={}, i1=np.array([0, n1 - 1, n1 - 1], dtype=np.int64), i2=np.zeros(3, dtype=np.int64),
                kind="tiny")


QUEUE_BLOCKS = {256: 23, 512: 46}
F2_CELLS = (kMicaLdsF2 - 1, kMicaLdsF2, kMicaLdsF2 + 1)
QUEUE_N = (11, 7)            # designed columns per side; three more per side carry the f2 cells (and the only unknowns)


def _queue(T):
    A, blocks = 20, QUEUE_BLOCKS[T]
    rng = np.random.default_rng(9000 + T)
    block = np.arange(T) * blocks // T
    key1, key2 = block % A, block * A // blocks
    assert len({(a, b) for a, b in zip(key1, key2)}) == blocks and np.bincount(block).min() >= 11

    def draw(n, key):
        return [rng.permutation(A)[key] for _ in range(n)]

    c1, c2 = draw(QUEUE_N[0], key1), draw(QUEUE_N[1], key2)
    extra = []
    for k in range(3):       # cell (0, 0) of pair (QUEUE_N[0] + k, QUEUE_N[1] + k): N_ab = 10, N_aG = N_Gb = 2, N_GG = 15 + k
        x, y = rng.integers(1, A, size=T), rng.integers(1, A, size=T)
        x[:12], y[:10], y[12:14] = 0, 0, 0
        x[12:14], y[10:12] = A, FAR
        x[14:29 + k], y[14:29 + k] = FAR, A
        c1.append(x)
        c2.append(y)
        extra.append((QUEUE_N[0] + k, QUEUE_N[1] + k))
    a1, a2 = np.stack(c1, axis=1).astype(np.uint8), np.stack(c2, axis=1).astype(np.uint8)
    i1, i2 = _listed(a1.shape[1], a2.shape[1], {}, {}, extra)
    return dict(A=A, T=T, a1=np.ascontiguousarray(a1), a2=np.ascontiguousarray(a2), idx1={}, idx2={}, i1=i1, i2=i2, kind="queue",
                f2_pairs=extra)


def _dump16():
    A, T = 20, 2047
    g = _grid(A, T)

    def const(state, unknown_at, code):
        c = np.full(T, state, dtype=np.uint8)
        c[unknown_at] = code
        return c

    a1 = np.stack([const(0, 5, A), const(0, 7, FAR), const(A - 1, T - 1, A), np.full(T, A, dtype=np.uint8), g["a1"][:, 0]], axis=1)
    a2 = np.stack([const(0, 5, FAR), const(3, 0, A), np.full(T, FAR, dtype=np.uint8), g["a2"][:, g["idx2"]["gapped2"]]], axis=1)
    i1, i2 = _listed(5, 4, {}, {}, [(0, 0), (1, 0), (2, 1), (3, 2)])
    return dict(A=A, T=T, a1=np.ascontiguousarray(a1), a2=np.ascontiguousarray(a2), idx1={}, idx2={}, i1=i1, i2=i2, kind="dump16")


def _names():
    out = []
    for A in (20, 4):
        out += [f"a{A}-t{T}" for T in TAXA[A]]
        out += [f"a{A}-t33-one", f"a{A}-t33-two", f"a{A}-t300-one", f"a{A}-t300-two"]
    return out + ["a20-t256-queue", "a20-t512-queue", "a20-t2047-dump16"]


CASES = _names()


@functools.lru_cache(maxsize=None)
def case(name):
    f = name.split("-")
    A, T = int(f[0][1:]), int(f[1][1:])
    if len(f) == 2:
        c = _grid(A, T)
    elif f[2] in ("one", "two"):
        c = _tiny(A, T, 1 if f[2] == "one" else 2)
    elif f[2] == "queue":
        c = _queue(T)
    else:
        c = _dump16()
    c.update(name=name, masks=masks_of(A))
    return c


def input_hash(c):
    h = hashlib.sha256()
    for k in ("a1", "a2", "masks", "i1", "i2"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()


def load(fix, name):
    """the fixture's record of a case: mi, hjoint [n1, n2]; imi, ihjoint [n1, n1] (the first side against itself, symmetric,
    the diagonal included: MI = Hjoint = H there); h1, h2; the listed pairs against the second side (pmi, phjoint) and against
    the first itself (qmi, qhjoint)"""
    r = {k: fix[f"{name}.{k}"] for k in ("mi", "hjoint", "h1", "h2", "pmi", "phjoint", "qmi", "qhjoint")}
    n1 = len(r["h1"])
    iu = np.triu_indices(n1)
    for k in ("imi", "ihjoint"):
        full = np.zeros((n1, n1))
        full[iu] = fix[f"{name}.{k}"]
        r[k] = full + np.triu(full, 1).T
    r["hash"] = str(fix[f"{name}.hash"])
    return r


# ------------------------------------------------------------------------------------------------ integer tables
def popcounts(A):
    t = mask_table(A)
    return np.array([bin(int(x)).count("1") for x in t]), t


def has_partial(aln, A):
    """[n] column carries a partial ambiguity code (the matrix-core kernels leave its pairs to the LDS-table kernel)"""
    k, _ = popcounts(A)
    kk = k[aln]
    return ((kk > 1) & (kk < A)).any(axis=0)


def denominator(A):
    """L: every weight 1 / |mask| of the table is a whole multiple of 1 / L"""
    k, _ = popcounts(A)
    return int(np.lcm.reduce(k[: A + 2]))


def units(aln, A):
    """[T, n, A] int64: L / |mask| in the states of each symbol's mask"""
    k, t = popcounts(A)
    L = denominator(A)
    bits = (t[aln][:, :, None] >> np.arange(A, dtype=np.uint32)) & 1
    return bits.astype(np.int64) * (L // k[aln])[:, :, None]


def gram(u1, u2):
    """[n1, n2, A, A] int64: m = L^2 x the fractional count of (column i state a, column j state b); exact (integers below
    2^53 through the fp64 matrix product)"""
    T, n1, A = u1.shape
    n2 = u2.shape[1]
    g = u1.reshape(T, n1 * A).astype(np.float64).T @ u2.reshape(T, n2 * A).astype(np.float64)
    return np.rint(g).astype(np.int64).reshape(n1, A, n2, A).transpose(0, 2, 1, 3)


def pseudo_counts(a1, a2, A):
    """[n1, n2, A + 1, A + 1] int64: the matrix-core kernels' integer table N over states and the pseudo-state G of unknowns;
    columns with partial codes have no such table (has_partial)"""
    def onehot(aln):
        code = np.where(aln < A, aln, A)
        return (code[:, :, None] == np.arange(A + 1)).astype(np.float64)

    o1, o2 = onehot(a1), onehot(a2)
    T, n1, n2 = a1.shape[0], a1.shape[1], a2.shape[1]
    g = o1.reshape(T, -1).T @ o2.reshape(T, -1)
    return np.rint(g).astype(np.int64).reshape(n1, A + 1, n2, A + 1).transpose(0, 2, 1, 3)


def weighted_cells(N, A):
    """m = A^2 N_ab + A (N_aG + N_Gb) + N_GG, [.., A, A]"""
    return A * A * N[..., :A, :A] + A * (N[..., :A, A:] + N[..., A:, :A]) + N[..., A:, A:]


# ------------------------------------------------------------------------------------------------ the two forms in fp64
def _seq(x, axis=-1):
    """sum in plain order (np.sum adds pairwise)"""
    return np.add.accumulate(x, axis=axis).take(-1, axis=axis)


def f2_table(A, T):
    m = np.arange(A * A * T + 1, dtype=np.float64) / (A * A)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > 0, m * np.log(m), 0.0)


def column_sums(aln, A):
    """S = sum_a c ln c, c = count_a + count_G / A (mica_codes_kernel)"""
    code = np.where(aln < A, aln, A)
    cnt = (code[:, :, None] == np.arange(A + 1)).sum(axis=0).astype(np.float64)      # [n, A + 1]
    c = cnt[:, :A] + (cnt[:, A] / A)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return _seq(np.where(c > 0, c * np.log(c), 0.0))


def table_form(a1, a2, A, T=None, f2=None, bump=False):
    """the matrix-core kernels' documented form: MI = ln T + (sum f2[m] - S1 - S2) / T, Hjoint = ln T - sum f2[m] / T, f2[m] =
    (m / A^2) ln (m / A^2) read from a table (for whole counts f2[A^2 N] has the bits of f[N] = N ln N).  NaN where a column
    carries a partial code.  T, f2, bump: what test_the_bound_tells_a_wrong_table_from_a_right_one changes."""
    T = a1.shape[0] if T is None else T
    f2 = f2_table(A, T + (1 if bump else 0)) if f2 is None else f2     # (bump: the neighbour of the last entry exists)
    m = weighted_cells(pseudo_counts(a1, a2, A), A).reshape(a1.shape[1], a2.shape[1], A * A)
    if bump:                 # the first cell of every pair that is read from global memory reads its neighbour
        big = m >= kMicaLdsF2
        first = big & (np.cumsum(big, axis=-1) == 1)
        m = m + first
    s = _seq(f2[m])
    lnT, invT = np.log(float(T)), 1.0 / float(T)
    mi = lnT + (s - column_sums(a1, A)[:, None] - column_sums(a2, A)[None, :]) * invT
    hj = lnT - s * invT
    bad = has_partial(a1, A)[:, None] | has_partial(a2, A)[None, :]
    return dict(mi=np.where(bad, np.nan, mi), hjoint=np.where(bad, np.nan, hj))


def definition_form(a1, a2, A):
    """the LDS-table kernel's form (mi_columns_kernel, mi_pairs_kernel): fractional counts in fp64, a logarithm per cell,
    MI = sum p_ab ln(p_ab / (p_a p_b)) with the marginals summed from the table.  The table is filled as the device fills
    it, the weights 1 / (k1 k2) added taxon by taxon (adding 1 / 400 two thousand times drifts, it does not random-walk);
    the device's four lanes per pair take every fourth taxon each, which is another order of the same adds."""
    T, n1, n2 = a1.shape[0], a1.shape[1], a2.shape[1]
    k, t = popcounts(A)

    def spread(aln):         # [T, n A]: the mask bits, the mask sizes
        bits = ((t[aln][:, :, None] >> np.arange(A, dtype=np.uint32)) & 1).astype(np.float64)
        return bits.reshape(T, -1), np.repeat(k[aln].astype(np.float64), A, axis=1)

    (b1, k1), (b2, k2) = spread(a1), spread(a2)
    tab = np.zeros((n1 * A, n2 * A))
    for x in range(T):
        tab += np.outer(b1[x], b2[x]) / np.outer(k1[x], k2[x])
    tab = tab.reshape(n1, A, n2, A).transpose(0, 2, 1, 3)                              # [n1, n2, A, A]
    p1 = np.add.accumulate(tab, axis=3)[..., -1]                                     # [n1, n2, A]: sum over b in order
    p2 = np.add.accumulate(tab, axis=2)[..., -1, :]
    pab = tab / T
    with np.errstate(divide="ignore", invalid="ignore"):
        ts = np.where(pab > 0, pab * np.log(pab / ((p1[..., :, None] / T) * (p2[..., None, :] / T))), 0.0)
        th = np.where(pab > 0, pab * np.log(pab), 0.0)
    return dict(mi=_seq(ts.reshape(n1, n2, A * A)), hjoint=-_seq(th.reshape(n1, n2, A * A)))


def entropy_form(aln, A):
    """column_entropy_kernel: every state's weight summed over the taxa in taxon order, the A terms added in state order"""
    T = aln.shape[0]
    k, t = popcounts(A)
    bits = ((t[aln][:, :, None] >> np.arange(A, dtype=np.uint32)) & 1).astype(np.float64)
    w = np.where(aln < A, 1.0, 1.0 / k[aln])
    p = _seq(bits * w[:, :, None], axis=0)                                           # [n, A]
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(p > 0, (p / T) * np.log(p / T), 0.0)
    return -_seq(term)


# ------------------------------------------------------------------------------------------------ the four-wave kernel's tiling
def four_wave_layout(a1, a2, A):
    """how launch_mica4 tiles a protein call: columns sorted (those without unknowns first, stable), blocks of three sorted
    columns, a workgroup's twelve first-side columns, a tile's three second-side columns; the weighted instantiation walks a
    (workgroup, tile) where any of its fifteen columns carries an unknown.
    -> list of (block of first-side columns [<= 3], tile of second-side columns [<= 3], weighted)"""
    def order(aln):
        k, _ = popcounts(A)
        gap = (k[aln] == A).any(axis=0)
        return np.concatenate([np.nonzero(~gap)[0], np.nonzero(gap)[0]]), gap

    o1, g1 = order(a1)
    o2, g2 = order(a2)
    out = []
    for w0 in range(0, len(o1), 12):
        group = o1[w0:w0 + 12]
        for t0 in range(0, len(o2), 3):
            tile = o2[t0:t0 + 3]
            weighted = bool(g1[group].any() or g2[tile].any())
            for b0 in range(0, len(group), 3):
                out.append((group[b0:b0 + 3], tile, weighted))
    return out
