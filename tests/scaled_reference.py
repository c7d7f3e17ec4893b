"""numpy restatement of the mapping with per-site likelihood scaling (cmx_set_likelihood_scaling), a plain
helper module imported by the tests: oracle/np_oracle.py::map_sites (uniformization counts) with a power-of-two exponent per
(class, node, site) beside the inside and the outside vectors, extended to the three mapping variants (nijt.average /
nijt.joint, as oracle.c restates them) and to marginal ancestral states (tests/ancestral_reference.py).

    true value = stored value * 2^exponent
    inside:   D_n = prod over the children m of M_m, exponent = sum of theirs; after EVERY factor: mx = max over the states,
              0 < mx < 2^-256  =>  the vector times 2^-ilogb(mx), exponent += ilogb(mx).  M_n = P_n D_n shares D_n's exponent.
    outside:  U_n = Up_f * prod over the siblings m of M_m, exponent = eUp_f + sum eD_m, the same rule per factor;
              Up_n = P_n^T U_n shares U_n's exponent; Up_root = pi with exponent 0.
    sums over the rate classes: every term is brought to the site likelihood's exponent E with ldexp, classes in order;
              E = the largest root exponent among the classes with a positive share of the likelihood.

Only powers of two are applied, so scale=True and scale=False give the same bits wherever scale=False meets no underflow.
dtype=np.longdouble with scale=False is the range-safe comparison partner where fp64 underflows (x87 extended: exponents down
to -16382).  The operators (P, the count matrices) are always computed in fp64, once per model (operators()).

Conventions are the engine's: nodes in post-order, root last, parent[root] = -1, lot[t] = node of taxon t, branch b = the
branch above node b; codes >= S are unknowns (masks[code] bits when a table is given)."""
import numpy as np

import oracle
from oracle import np_oracle as npo

RESCALE_BELOW_EXP = -256     # a vector whose largest element is below 2^-256 is rescaled


def has_extended_range():
    """long double reaches below fp64's smallest subnormal (x87 80-bit or binary128)"""
    return np.finfo(np.longdouble).minexp < -2000


def operators(parent, blen, Q, pi, rates, Bk=None, nonneg=True):
    """fp64 operators of a homogeneous model: dict(P [C, nn, S, S], PN [C, nn, K, S, S] the joint count operator P o NC,
    NC [C, nn, K, S, S] conditional counts at r_c t_b,
    N1 [nn, K, S, S] conditional counts at t_b itself); the root's entries stay 0"""
    Q, pi = np.asarray(Q, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    S, C, nn = len(pi), len(rates), len(parent)
    if Bk is None:
        Bk = [npo.rate_matrix_register(Q)]
    K = len(Bk)
    eig = npo.eigen_reversible(Q, pi)
    P, NC, N1 = np.zeros((C, nn, S, S)), np.zeros((C, nn, K, S, S)), np.zeros((nn, K, S, S))

    PN = np.zeros((C, nn, K, S, S))

    def cond(t, Pt, joint=None):
        Js = [npo.count_matrix_uniformization(Q, B, t) for B in Bk]
        N = np.stack([npo.conditional_counts(J, Pt, nonneg) for J in Js])
        if joint is not None:       # P o N, keeping a positive J(x, y) where P is not positive (oracle.c joint_count_matrix)
            for k, J in enumerate(Js):
                joint[k] = np.where(~(Pt > 0) & (J > 0), J, Pt * N[k]) if nonneg else np.where(Pt == 0, J, Pt * N[k])
        return N

    for b in range(nn):
        if parent[b] < 0:
            continue
        N1[b] = cond(blen[b], npo.transition_matrix(*eig, blen[b]))
        for c in range(C):
            P[c, b] = npo.class_transition_matrix(*eig, blen[b], rates[c])
            NC[c, b] = cond(blen[b] * rates[c], P[c, b], PN[c, b])
    return dict(P=P, NC=NC, N1=N1, PN=PN)


def _ilogb(m):
    return np.frexp(m)[1].astype(np.int64) - 1


def _rescale(v, e, scale):
    """v [C, N, S], e [C, N]: the rule above, in place"""
    if not scale:
        return
    m = v.max(axis=-1)
    with np.errstate(invalid="ignore"):
        sel = (m > 0) & (m < np.ldexp(v.dtype.type(1), RESCALE_BELOW_EXP))
    if sel.any():
        k = np.where(sel, _ilogb(np.where(sel, m, 1)), 0)
        v[...] = np.ldexp(v, (-k)[..., None].astype(np.intc))
        e += k


def _shift(x, k):
    return np.ldexp(x, np.asarray(k).astype(np.intc))


class Vectors:
    """inside / outside vectors of every node [C, N, S] with their exponents [C, N], and the site likelihood L * 2^E"""


def vectors(parent, lot, aln, ops, pi, probs, masks=None, dtype=np.float64, scale=True, outside=True):
    parent = np.asarray(parent)
    nn, root = len(parent), len(parent) - 1
    pi, probs = np.asarray(pi, dtype=dtype), np.asarray(probs, dtype=dtype)
    P = ops["P"].astype(dtype)
    C, S = P.shape[0], P.shape[-1]
    aln = np.asarray(aln)
    N = aln.shape[1]
    mk = oracle.default_masks(S) if masks is None else np.asarray(masks, dtype=np.uint32)
    ch = npo.children_lists(parent)
    taxon = {int(n): t for t, n in enumerate(lot)}
    v = Vectors()
    v.ch, v.nn, v.root, v.C, v.S, v.N = ch, nn, root, C, S, N
    D, M, eD = [None] * nn, [None] * nn, [None] * nn
    for n in range(nn):
        e = np.zeros((C, N), dtype=np.int64)
        if not ch[n]:
            lp = npo.leaf_partials(aln[taxon[n]], mk, S).astype(dtype)
            d = np.broadcast_to(lp[None], (C, N, S)).copy()
        else:
            d = np.ones((C, N, S), dtype=dtype)
            for m in ch[n]:
                d *= M[m]
                e += eD[m]
                _rescale(d, e, scale)
        D[n], eD[n] = d, e
        if n != root:
            M[n] = np.einsum("cxz,cnz->cnx", P[:, n], d)
    v.D, v.M, v.eD = D, M, eD
    # p_c L_c as stored, the site exponent, the site likelihood at that exponent (classes in order)
    w = probs[:, None] * np.einsum("cnx,x->cn", D[root], pi)
    with np.errstate(invalid="ignore"):
        pos = w > 0
    E = np.where(pos.any(axis=0), np.where(pos, eD[root], np.iinfo(np.int64).min).max(axis=0), 0)
    v.terms = _shift(w, eD[root] - E[None])
    L = np.zeros(N, dtype=dtype)
    for c in range(C):
        L = L + v.terms[c]
    v.L, v.E = L, E
    if not outside:
        return v
    U, Up, eU = [None] * nn, [None] * nn, [None] * nn
    Up[root] = np.broadcast_to(pi[None, None, :], (C, N, S)).copy()
    eU[root] = np.zeros((C, N), dtype=np.int64)
    for f in range(nn - 1, -1, -1):
        for n in ch[f]:
            u, e = Up[f].copy(), eU[f].copy()
            for m in ch[f]:
                if m != n:
                    u *= M[m]
                    e += eD[m]
                    _rescale(u, e, scale)
            U[n], eU[n] = u, e
            if ch[n]:
                Up[n] = np.einsum("cxz,cnx->cnz", P[:, n], u)
    v.U, v.Up, v.eU = U, Up, eU
    return v


def _node_shift(v, n):
    """[C, N]: what brings U_n D_n (or Up_n D_n) to the site likelihood's exponent"""
    return v.eU[n] + v.eD[n] - v.E[None]


def _posterior(v, n, probs, dtype):
    """[C, N, S] p_c Up_n D_n / L of an internal node (or the root)"""
    return _shift(v.Up[n] * v.D[n] * probs[:, None, None], _node_shift(v, n)[..., None]) / v.L[None, :, None]


def _first_two(a):
    """along the last axis: (index of the first maximum, relative gap between the two largest values)"""
    a = np.asarray(a, dtype=np.float64)
    idx = np.argmax(a, axis=-1)
    s = np.sort(a, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (s[..., -1] - s[..., -2]) / np.abs(s[..., -1])
    return idx, gap


def map_sites(parent, blen, lot, aln, Q, pi, rates, probs, masks=None, ops=None, average=True, joint=True, dtype=np.float64,
              scale=True):
    """-> dict(counts [N, B, K], norm, logL, post_rate [N] (fp64), rate_class [N], exponent [N] of the site likelihood); average / joint as
    cmx_set_mapping_options; without averaging also margin [N, B]: the relative gap between the two best candidates of the
    branch's choice of states (both ends' for joint = False), below which another implementation may choose differently"""
    ops = operators(parent, blen, Q, pi, rates) if ops is None else ops
    v = vectors(parent, lot, aln, ops, pi, probs, masks, dtype, scale)
    rates_t, probs_t = np.asarray(rates, dtype=dtype), np.asarray(probs, dtype=dtype)
    P, NC, N1 = ops["P"].astype(dtype), ops["NC"].astype(dtype), ops["N1"]
    PN = ops["PN"].astype(dtype) if "PN" in ops else P[:, :, None] * NC
    C, S, N, nn, root = v.C, v.S, v.N, v.nn, v.root
    B, K = nn - 1, NC.shape[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        pr = np.zeros(N, dtype=dtype)
        for c in range(C):
            pr = pr + rates_t[c] * v.terms[c]
        out = dict(logL=(np.log(v.L) + v.E * np.log(dtype(2))).astype(np.float64), post_rate=(pr / v.L).astype(np.float64),
                   rate_class=np.argmax(v.terms, axis=0).astype(np.int32))
        counts = np.zeros((N, B, K), dtype=dtype)
        margin = np.full((N, B), np.inf)
        post = {}
        if not joint:
            for n in range(nn):
                if v.ch[n]:
                    post[n] = _posterior(v, n, probs_t, dtype)
                else:                   # leaf: e(x) p_c / sum e
                    post[n] = v.D[n] * probs_t[:, None, None] / v.D[n][0].sum(axis=-1)[None, :, None]
        for b in range(B):
            f = int(parent[b])
            if joint and average:
                sh = _node_shift(v, b)
                for k in range(K):
                    tot = np.zeros(N, dtype=dtype)
                    for c in range(C):
                        vc = np.einsum("nx,xy,ny->n", v.U[b][c], PN[c, b, k], v.D[b][c])
                        tot = tot + _shift(probs_t[c] * vc, sh[c])
                    counts[:, b, k] = tot / v.L
            elif joint:
                sh = _node_shift(v, b)
                pxy = np.zeros((N, S, S), dtype=dtype)
                for c in range(C):
                    pxy = pxy + _shift(probs_t[c] * (v.U[b][c][:, :, None] * P[c, b][None] * v.D[b][c][:, None, :]), sh[c][:, None, None])
                idx, margin[:, b] = _first_two(pxy.reshape(N, S * S))
                counts[:, b, :] = N1[b].reshape(K, S * S)[:, idx].T
            elif average:
                for k in range(K):
                    counts[:, b, k] = np.einsum("cnx,cxy,cny->n", post[f], NC[:, b, k], post[b])
            else:
                xs, gf = _first_two(post[f].sum(axis=0))
                ys, gn = _first_two(post[b].sum(axis=0) if v.ch[b] else v.D[b][0])
                margin[:, b] = np.minimum(gf, gn)
                counts[:, b, :] = N1[b][:, xs, ys].T
        counts = counts.astype(np.float64)
    out.update(counts=counts, norm=np.sqrt((counts.sum(axis=2) ** 2).sum(axis=1)), margin=margin, exponent=v.E)
    return out


def ancestral_states(parent, blen, lot, aln, Q, pi, rates, probs, masks=None, ops=None, dtype=np.float64, scale=True):
    """-> dict(nodes [n_inner], states [n_inner, N], post [n_inner, N, S] fp64, gap [n_inner, N]: the two largest
    posteriors' difference)"""
    ops = operators(parent, blen, Q, pi, rates) if ops is None else ops
    v = vectors(parent, lot, aln, ops, pi, probs, masks, dtype, scale)
    probs_t = np.asarray(probs, dtype=dtype)
    nodes = [n for n in range(v.nn) if v.ch[n]]
    with np.errstate(divide="ignore", invalid="ignore"):
        post = np.zeros((len(nodes), v.N, v.S), dtype=dtype)
        for q, n in enumerate(nodes):
            pc = _posterior(v, n, probs_t, dtype)
            for c in range(v.C):
                post[q] = post[q] + pc[c]
    post = post.astype(np.float64)
    s = np.sort(post, axis=-1)
    return dict(nodes=nodes, states=np.argmax(post, axis=-1), post=post, gap=s[..., -1] - s[..., -2])
