"""Test support: column mutual information for any alphabet size, restated in numpy from the definition (SiteTools::
mutualInformation / jointEntropy / entropy with resolveUnknowns = true, natural log).  A code < A is that state, every code
>= A is an unknown = 1/A in every state.  The oracle's mi_columns is generic only up to 31 states (32-bit masks);
tests/test_mica_wide_reference.py pins this restatement to it where both are defined."""
import numpy as np


def onehot(aln, A):
    """[T, n] codes -> [T, n, A] rows: a state is one-hot, an unknown is 1/A everywhere"""
    aln = np.asarray(aln)
    T, n = aln.shape
    oh = np.full((T, n, A), 1.0 / A)
    known = aln < A
    oh[known] = 0.0
    t, i = np.nonzero(known)
    oh[t, i, aln[t, i]] = 1.0
    return oh


def _plogp(p, axis):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0.0, p * np.log(p), 0.0).sum(axis=axis)


def entropy(aln, A):
    p = onehot(aln, A).mean(axis=0)          # [n, A]
    return -_plogp(p, -1)


def mi_columns(aln1, aln2, A):
    """-> dict(mi [n1, n2], hjoint [n1, n2], h1 [n1], h2 [n2]); aln2 None: aln1 against itself, every cell filled"""
    aln2 = aln1 if aln2 is None else aln2
    o1, o2 = onehot(aln1, A), onehot(aln2, A)
    T = o1.shape[0]
    p = np.einsum("tia,tjb->ijab", o1, o2) / T
    pa, pb = o1.mean(axis=0), o2.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = p / (pa[:, None, :, None] * pb[None, :, None, :])
        mi = np.where(p > 0.0, p * np.log(ratio), 0.0).sum(axis=(2, 3))
    return dict(mi=mi, hjoint=-_plogp(p, (2, 3)), h1=-_plogp(pa, -1), h2=-_plogp(pb, -1))


def mi_pairs(aln1, idx1, idx2, A, aln2=None):
    aln2 = aln1 if aln2 is None else aln2
    o1, o2 = onehot(np.asarray(aln1)[:, idx1], A), onehot(np.asarray(aln2)[:, idx2], A)
    T = o1.shape[0]
    p = np.einsum("tpa,tpb->pab", o1, o2) / T
    pa, pb = o1.mean(axis=0), o2.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = p / (pa[:, :, None] * pb[:, None, :])
        mi = np.where(p > 0.0, p * np.log(ratio), 0.0).sum(axis=(1, 2))
    return dict(mi=mi, hjoint=-_plogp(p, (1, 2)))


def columns(A, T, n, seed, clean_half=True):
    """the inputs of the wide-alphabet tests: columns with signal, code A and code 200 unknowns in 10 % of the cells, the
    second half of the columns without any unknown (both epilogues in one call), one all-unknown and one constant column"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, A, size=(T, 1))
    aln = np.where(rng.random((T, n)) < 0.6, base, rng.integers(0, A, size=(T, n)))
    u = rng.random((T, n))
    aln = np.where(u < 0.05, A, np.where(u < 0.10, 200, aln))
    if clean_half and n >= 2:
        clean = rng.integers(0, A, size=(T, n))
        aln[:, n // 2:] = np.where(aln[:, n // 2:] >= A, clean[:, n // 2:], aln[:, n // 2:])
    if n >= 3:
        aln[:, 1] = A + 1 if A < 255 else 255       # all unknown: h = ln A, MI = 0
        aln[:, n - 1] = A - 1                       # constant (the last state: 63 is a real state at A = 64): h = 0, MI = 0
    return aln.astype(np.uint8)
