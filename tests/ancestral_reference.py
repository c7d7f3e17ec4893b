"""numpy restatement of asr.method = marginal (CoMap/CoMap.cpp:169-197: LegacyMarginalAncestralStateReconstruction::
getAncestralStatesForNode), a plain helper module imported by the tests.  It also takes a non-homogeneous model set
(one generator per branch, root frequencies), which the oracle does not.  For an internal node n and a site i:

    post_n(i, x) = sum_c p_c Up_n(i, c, x) D_n(i, c, x) / L_i      (Up_root = root frequencies)
    state_n(i)   = first x that maximises post_n(i, x)

D: the inside (conditional) vectors; Up: the outside vectors at the node (the father's outside vector times the
siblings' messages, carried down the branch).  Conventions are the engine's: nodes in post-order, root last,
parent[root] = -1, leaf_of_taxon[t] = node of taxon t; codes >= S are unknowns (masks[code] bits when a table is given)."""
import itertools

import numpy as np
import scipy.linalg


def _leaf_vectors(aln, S, masks):
    """[T, N, S] compatibility of every alignment code with every state"""
    aln = np.asarray(aln)
    e = np.zeros(aln.shape + (S,))
    for x in range(S):
        if masks is None or S > 32:
            e[..., x] = np.where(aln < S, aln == x, 1.0)
        else:
            m = np.asarray(masks, dtype=np.uint64)[aln]
            e[..., x] = np.where(aln < S, aln == x, (m >> np.uint64(x)) & np.uint64(1))
    return e


def transition_matrices(parent, blen, Qs, rates, model_of_branch=None):
    """P[c, b] = expm(Q_{m(b)} r_c t_b) for the branches b (nodes other than the root)"""
    Qs = np.asarray(Qs, dtype=np.float64)
    if Qs.ndim == 2:
        Qs = Qs[None]
    nn = len(parent)
    mob = np.zeros(nn, dtype=int) if model_of_branch is None else np.asarray(model_of_branch)
    S = Qs.shape[-1]
    P = np.zeros((len(rates), nn, S, S))
    for c, r in enumerate(rates):
        for b in range(nn):
            if parent[b] >= 0:
                P[c, b] = scipy.linalg.expm(Qs[mob[b]] * (r * blen[b]))
    return P


def inner_nodes(parent):
    parent = np.asarray(parent)
    return [n for n in range(len(parent)) if (parent == n).any()]


def ancestral_states(parent, blen, lot, Qs, rates, probs, root_freqs, aln, masks=None, model_of_branch=None):
    """-> dict(nodes [n_inner], states int [n_inner, N], post [n_inner, N, S])"""
    parent = np.asarray(parent)
    nn = len(parent)
    root = int(np.flatnonzero(parent < 0)[0])
    pi = np.asarray(root_freqs, dtype=np.float64)
    S, C = len(pi), len(rates)
    P = transition_matrices(parent, blen, Qs, rates, model_of_branch)
    e = _leaf_vectors(aln, S, masks)
    N = e.shape[1]
    children = [[] for _ in range(nn)]
    for b in range(nn):
        if parent[b] >= 0:
            children[parent[b]].append(b)
    taxon = {int(n): t for t, n in enumerate(lot)}
    D = np.zeros((nn, C, N, S))
    M = np.zeros((nn, C, N, S))   # message of node n to its father: P_n D_n
    for n in range(nn):           # post-order
        D[n] = np.broadcast_to(e[taxon[n]], (C, N, S)) if not children[n] else np.prod([M[m] for m in children[n]], axis=0)
        if n != root:
            M[n] = np.einsum("cxz,ciz->cix", P[:, n], D[n])
    Up = np.zeros((nn, C, N, S))
    Up[root] = pi
    for f in range(nn - 1, -1, -1):
        for n in children[f]:
            u = Up[f] * np.prod([M[m] for m in children[f] if m != n] or [np.ones((C, N, S))], axis=0)
            Up[n] = np.einsum("cxz,cix->ciz", P[:, n], u)
    L = np.einsum("c,x,cix->i", np.asarray(probs, dtype=np.float64), pi, D[root])
    nodes = inner_nodes(parent)
    post = np.einsum("c,qcix->qix", np.asarray(probs, dtype=np.float64), Up[nodes] * D[nodes]) / L[None, :, None]
    return dict(nodes=nodes, states=np.argmax(post, axis=2), post=post)


def brute_force(parent, blen, lot, Qs, rates, probs, root_freqs, aln, masks=None, model_of_branch=None):
    """the same posteriors by enumerating every assignment of states to the internal nodes: [n_inner, N, S]"""
    parent = np.asarray(parent)
    nn = len(parent)
    pi = np.asarray(root_freqs, dtype=np.float64)
    S = len(pi)
    P = transition_matrices(parent, blen, Qs, rates, model_of_branch)
    e = _leaf_vectors(aln, S, masks)
    N = e.shape[1]
    taxon = {int(n): t for t, n in enumerate(lot)}
    nodes = inner_nodes(parent)
    root = int(np.flatnonzero(parent < 0)[0])
    post = np.zeros((len(nodes), N, S))
    for st in itertools.product(range(S), repeat=len(nodes)):
        x = dict(zip(nodes, st))
        w = np.zeros(N)
        for c, pc in enumerate(probs):
            wc = np.full(N, pc * pi[x[root]])
            for b in range(nn):
                if parent[b] < 0:
                    continue
                row = P[c, b, x[int(parent[b])]]
                wc = wc * (row @ e[taxon[b]].T if b in taxon else row[x[b]])
            w += wc
        for q, n in enumerate(nodes):
            post[q, :, x[n]] += w
    return post / post[0].sum(axis=1)[None, :, None]


def model_set(S, seed):
    """two reversible generators with their own frequencies (mean rate 1) and root frequencies of neither:
    (Qs [2, S, S], pis [2, S], root_freqs [S])"""
    rng = np.random.default_rng(seed)
    Qs, pis = [], []
    for _ in range(2):
        pi = rng.uniform(0.5, 1.5, S)
        pi /= pi.sum()
        R = rng.uniform(0.2, 2.0, (S, S))
        Q = (R + R.T) / 2 * pi[None, :]
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
        Qs.append(Q / -(pi * np.diag(Q)).sum())
        pis.append(pi)
    rf = rng.uniform(0.5, 1.5, S)
    return np.array(Qs), np.array(pis), rf / rf.sum()


def brute_force_joint(parent, blen, lot, Qs, rates, probs, root_freqs, aln, masks=None, model_of_branch=None):
    """every assignment of states to ALL nodes (a leaf takes the states compatible with its code), per site and class ->
    dict(L [N] site likelihood, pair [nn, C, N, S, S] Pr(class c, father = x, node = y, data) of every branch,
    node [nn, C, N, S] Pr(class c, node = x, data)); divide by L for the posteriors"""
    parent = np.asarray(parent)
    nn = len(parent)
    pi = np.asarray(root_freqs, dtype=np.float64)
    S, C = len(pi), len(rates)
    P = transition_matrices(parent, blen, Qs, rates, model_of_branch)
    e = _leaf_vectors(aln, S, masks)
    N = e.shape[1]
    taxon = {int(n): t for t, n in enumerate(lot)}
    root = int(np.flatnonzero(parent < 0)[0])
    L, pair, node = np.zeros(N), np.zeros((nn, C, N, S, S)), np.zeros((nn, C, N, S))
    for i in range(N):
        allowed = [np.flatnonzero(e[taxon[n], i]) if n in taxon else range(S) for n in range(nn)]
        for st in itertools.product(*allowed):
            for c in range(C):
                w = probs[c] * pi[st[root]]
                for b in range(nn):
                    if parent[b] >= 0:
                        w *= P[c, b, st[parent[b]], st[b]]
                L[i] += w
                for b in range(nn):
                    node[b, c, i, st[b]] += w
                    if parent[b] >= 0:
                        pair[b, c, i, st[parent[b]], st[b]] += w
    return dict(L=L, pair=pair, node=node)
