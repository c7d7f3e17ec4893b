#!/usr/bin/env python3
"""Known answers at the edges of branch length and rate, in 50-digit arithmetic (mpmath) from the DEFINITIONS: the cases of
tests/operator_edge_cases.py (zero, 1e-100, 1e-12 and saturated branches, a rate-zero class, degenerate spectra).

  * P(t) = exp(Q t) from the symmetrised generator's eigen-system at 50 digits;
  * J_k(t) = integral_0^t exp(Q s) B_k exp(Q (t - s)) ds = V [ (Vinv B_k V) o Phi ] Vinv with the exact divided difference
    Phi_ij = (e^{l_i t} - e^{l_j t}) / (l_i - l_j), evaluated at 50 digits as t e^{max(l_i, l_j) t} (-expm1(-|d|)) / |d|,
    d = (l_i - l_j) t (no cancellation where mpmath's eigenvalues of a degenerate spectrum differ by 1e-50).  Checked twice
    before anything is written: against the plain quotient at 200 digits for every stored time, and against a Gauss-Legendre
    quadrature of the matrix-valued integrand (as make_small_tree_fixture.py computes it) at t = 0.3 and t = 3, where the
    quadrature converges; the file is not written if either disagrees beyond 1e-30 relative;
  * Felsenstein pruning down and up, site likelihood, posterior rate, rate class and the averaged joint counts
    n(b, i, k) = sum_c p_c sum_xy U_b(x) J_k(r_c t_b)(x, y) D_b(y) / L_i; codes >= S are unknowns (every state compatible).

Stored, rounded to fp64: per case the inputs and logL, post_rate, rate_class, class_clear, counts [N, B, K]; P [C, B, S, S] for
S <= 7 and, once per distinct time r_c t_b, P of the 20-state cases of ANCESTRAL_CASES (the ancestral states); for the cases of has_variants() the counts of the
three other nijt.average / nijt.joint options (counts_a0j1, counts_a1j0, counts_a0j0, from the conditional counts N = J / P
at t_b and at r_c t_b) with the relative gap between the two best candidates of every choice of states (margin_*); per generator of OPERATOR_MODELS P and J_k at operator_times().  The reference log-
likelihood of every stored site is asserted finite.

    python tests/golden/make_operator_edge_fixture.py        # a few minutes; writes tests/golden/operator_edges.npz"""
import os
import sys
import time

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import operator_edge_cases as oe  # noqa: E402

mp.mp.dps = 50
mpf = mp.mpf


def matmul(A, B):
    Bt = list(zip(*B))
    return [[mp.fdot(row, col) for col in Bt] for row in A]


def maxabs(A):
    return max(abs(v) for row in A for v in row)


class Spectrum:
    """exp(Q t) and the count integral of a generator that is reversible w.r.t. pi, from the symmetrised generator's
    eigen-system"""

    def __init__(self, Q, pi):
        S = self.S = len(pi)
        sq = [mp.sqrt(mpf(float(p))) for p in pi]
        A = mp.matrix(S, S)
        for x in range(S):
            for y in range(S):
                A[x, y] = sq[x] * mpf(float(Q[x, y])) / sq[y]
        A = (A + A.T) / 2
        lam, U = mp.eigsy(A)
        self.lam = [lam[k] for k in range(S)]
        self.L = [[U[x, k] / sq[x] for k in range(S)] for x in range(S)]      # V
        self.R = [[U[x, k] * sq[x] for x in range(S)] for k in range(S)]      # Vinv
        self.pi = [mpf(float(p)) for p in pi]
        self._P, self._J, self._W = {}, {}, {}

    def P(self, t):
        if t not in self._P:
            e = [mp.exp(l * mpf(t)) for l in self.lam]
            self._P[t] = matmul([[v * e[k] for k, v in enumerate(row)] for row in self.L], self.R)
        return self._P[t]

    def phi(self, i, j, t):
        t = mpf(t)
        d = abs(self.lam[i] - self.lam[j]) * t
        top = t * mp.exp(max(self.lam[i], self.lam[j]) * t)
        return top if d == 0 else top * -mp.expm1(-d) / d

    def check_phi(self, t):
        """the stable form against the plain divided difference at 200 digits, where the eigenvalues are far enough apart
        for the latter to keep 40 digits"""
        worst = mpf(0)
        for i in range(self.S):
            for j in range(self.S):
                dl = self.lam[i] - self.lam[j]
                if t == 0 or abs(dl) < mpf(10) ** -20:
                    continue
                with mp.workdps(200):
                    plain = (mp.exp(self.lam[i] * mpf(t)) - mp.exp(self.lam[j] * mpf(t))) / dl
                worst = max(worst, abs(self.phi(i, j, t) - plain) / abs(plain))
        assert worst < mpf(10) ** -30, (t, worst)

    def J(self, key, Bm, t):
        """Bm [S][S] of mpf (the register), key names it"""
        if key not in self._W:
            self._W[key] = matmul(matmul(self.R, Bm), self.L)
        if (key, t) not in self._J:
            W, S = self._W[key], self.S
            X = [[W[i][j] * self.phi(i, j, t) for j in range(S)] for i in range(S)]
            self._J[(key, t)] = matmul(matmul(self.L, X), self.R)
        return self._J[(key, t)]

    def J_quadrature(self, Bm, t, degree):
        nodes = sorted(mp.calculus.quadrature.GaussLegendre(mp.mp).calc_nodes(degree, mp.mp.prec))
        half = mpf(t) / 2
        E = [self.P(half * (x + 1)) for x, _ in nodes]
        n, S = len(nodes), self.S
        J = [[mpf(0)] * S for _ in range(S)]
        for k in range(n):
            T = matmul(matmul(E[k], Bm), E[n - 1 - k])
            w = nodes[k][1] * half
            J = [[J[x][y] + w * T[x][y] for y in range(S)] for x in range(S)]
        return J


def registers(Q, Bk):
    """[K] registers as lists of mpf"""
    S = Q.shape[0]
    if Bk is None:
        Bk = np.array(Q, copy=True)
        np.fill_diagonal(Bk, 0.0)
        Bk = Bk[None]
    return [[[mpf(float(B[x, y])) for y in range(S)] for x in range(S)] for B in Bk]


def to_np(A):
    return np.array([[float(v) for v in row] for row in A])


_spectra = {}


def spectrum(gen):
    if gen not in _spectra:
        Q, pi, Bk, _ = oe.generator(gen)
        sp = Spectrum(Q, pi)
        sp.regs = registers(Q, Bk)
        t0 = time.time()
        for t, degree in ((0.3, 5), (3.0, 5)) if sp.S <= 20 else ((0.3, 4),):     # 48 / 24 nodes
            for k, Bm in enumerate(sp.regs):
                a, b = sp.J(k, Bm, t), sp.J_quadrature(Bm, t, degree)
                err = maxabs([[a[x][y] - b[x][y] for y in range(sp.S)] for x in range(sp.S)]) / maxabs(a)
                assert err < mpf(10) ** -30, (gen, t, k, err)
        sp._P.clear()
        print(f"  {gen}: closed form == quadrature ({time.time() - t0:.0f} s)", flush=True)
        _spectra[gen] = sp
    return _spectra[gen]


def solve_case(name, inputs=None, variants=None, store_P=True):
    """inputs: the case's oe.Inputs (or an object like it; default oe.Inputs(name)); variants: whether the three other
    nijt options are solved too (default oe.has_variants(name)); store_P: P of the cases with S <= 7"""
    c = oe.Inputs(name) if inputs is None else inputs
    sp = spectrum(c.gen)
    aln, cls = c.draw()
    S, C, K = c.S, len(c.rates), len(sp.regs)
    parent, nn = c.parent, len(c.parent)
    B, root = nn - 1, nn - 1
    children = [[] for _ in range(nn)]
    for i in range(nn - 1):
        children[parent[i]].append(i)
    taxon_of = {int(n): t for t, n in enumerate(c.lot)}
    # what the draw must have given (the definition of "possible under the tree")
    for b in range(B):
        if c.blen[b] == 0.0 and not children[b]:
            sib = [m for m in children[parent[b]] if m != b and not children[m] and c.blen[m] == 0.0]
            for m in sib:
                a, bb = aln[taxon_of[b]], aln[taxon_of[m]]
                assert np.all((a == bb) | (a >= S) | (bb >= S)), name
    for i in np.nonzero(np.asarray(c.rates)[cls] == 0.0)[0]:
        assert len(set(int(v) for v in aln[:, i] if v < S)) <= 1, name
    times = [[float(c.blen[b]) * float(c.rates[cc]) for b in range(B)] for cc in range(C)]
    for cc in range(C):
        for b in range(B):
            sp.check_phi(times[cc][b])
    P = [[sp.P(times[cc][b]) for b in range(B)] for cc in range(C)]
    J = [[[sp.J(k, sp.regs[k], times[cc][b]) for k in range(K)] for b in range(B)] for cc in range(C)]
    pr = [mpf(float(p)) for p in c.probs]
    rt = [mpf(float(r)) for r in c.rates]
    variants = oe.has_variants(name) if variants is None else variants
    if variants:        # the conditional counts N = J / P (0 where P = 0: no time), unsigned registers clamped at 0
        def cond(Jm, Pm):
            N_ = [[(Jm[x][y] / Pm[x][y] if Pm[x][y] != 0 else mpf(0)) for y in range(S)] for x in range(S)]
            return [[max(v, mpf(0)) for v in row] for row in N_] if c.clamp else N_
        NC = [[[cond(J[cc][b][k], P[cc][b]) for k in range(K)] for b in range(B)] for cc in range(C)]
        N1 = [[cond(sp.J(k, sp.regs[k], float(c.blen[b])), sp.P(float(c.blen[b]))) for k in range(K)] for b in range(B)]
        var = {v: np.zeros((aln.shape[1], B, K)) for v in ("counts_a0j1", "counts_a1j0", "counts_a0j0")}
        var.update(margin_a0j1=np.zeros((aln.shape[1], B)), margin_a0j0=np.zeros((aln.shape[1], B)))

    def first_two(vals):
        """(index of the first maximum, relative gap to the second largest)"""
        best = max(range(len(vals)), key=lambda q: (vals[q], -q))
        rest = max(v for q, v in enumerate(vals) if q != best)
        return best, float((vals[best] - rest) / abs(vals[best])) if vals[best] != 0 else 0.0
    N = aln.shape[1]
    counts = np.zeros((N, B, K))
    logL, prate, rclass, clear = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
    for i in range(N):
        Lc, cnt, Dc, Uc, Upc = [], [], [], [], []
        for cc in range(C):
            D, M = [None] * nn, [None] * nn
            for n in range(nn):
                if not children[n]:
                    code = int(aln[taxon_of[n], i])
                    D[n] = [mpf(1) if (code >= S or x == code) else mpf(0) for x in range(S)]
                else:
                    D[n] = [mpf(1)] * S
                    for e in children[n]:
                        D[n] = [D[n][x] * M[e][x] for x in range(S)]
                if n != root:
                    nz = [z for z in range(S) if D[n][z] != 0]
                    M[n] = [mp.fsum(P[cc][n][x][z] * D[n][z] for z in nz) for x in range(S)]
            Lc.append(mp.fsum(sp.pi[x] * D[root][x] for x in range(S)))
            U, Up = [None] * nn, [None] * nn
            Up[root] = sp.pi
            for f in range(nn - 1, -1, -1):
                for n in children[f]:
                    u = list(Up[f])
                    for m in children[f]:
                        if m != n:
                            u = [u[x] * M[m][x] for x in range(S)]
                    U[n] = u
                    if children[n]:
                        Up[n] = [mp.fsum(P[cc][n][x][z] * u[x] for x in range(S)) for z in range(S)]
            row = []
            for b in range(B):
                nz = [y for y in range(S) if D[b][y] != 0]
                row.append([mp.fsum(U[b][x] * mp.fsum(J[cc][b][k][x][y] * D[b][y] for y in nz) for x in range(S))
                            for k in range(K)])
            cnt.append(row)
            Dc.append(D)
            Uc.append(U)
            Upc.append(Up)
        share = [pr[cc] * Lc[cc] for cc in range(C)]
        L = mp.fsum(share)
        assert L > 0 and mp.isfinite(mp.log(L)), (name, i)
        logL[i] = float(mp.log(L))
        assert np.isfinite(logL[i]), (name, i)
        prate[i] = float(mp.fsum(rt[cc] * share[cc] for cc in range(C)) / L)
        order = sorted(range(C), key=lambda cc: -share[cc])
        rclass[i] = order[0]
        # where the two best classes tie to 1e-9 (a site whose taxa are all beyond saturated branches has the same
        # likelihood under every fast class) another implementation's argmax may differ: class_clear marks the others
        clear[i] = C == 1 or share[order[0]] - share[order[1]] > mpf(10) ** -9 * share[order[0]]
        for b in range(B):
            for k in range(K):
                counts[i, b, k] = float(mp.fsum(pr[cc] * cnt[cc][b][k] for cc in range(C)) / L)
        if not variants:
            continue
        post = [None] * nn       # post[n][cc][x]: internal nodes p_c Up D / L; leaves e(x) p_c / sum e (as the reference)
        for n in range(nn):
            if children[n]:
                post[n] = [[pr[cc] * Upc[cc][n][x] * Dc[cc][n][x] / L for x in range(S)] for cc in range(C)]
            else:
                tot = mp.fsum(Dc[0][n])
                post[n] = [[Dc[0][n][x] * pr[cc] / tot for x in range(S)] for cc in range(C)]
        for b in range(B):
            f = int(parent[b])
            pxy = [mp.fsum(pr[cc] * Uc[cc][b][x] * P[cc][b][x][y] * Dc[cc][b][y] for cc in range(C))
                   for x in range(S) for y in range(S)]
            q, var["margin_a0j1"][i, b] = first_two(pxy)
            xs, gf = first_two([mp.fsum(post[f][cc][x] for cc in range(C)) for x in range(S)])
            ys, gn = first_two([mp.fsum(post[b][cc][y] for cc in range(C)) for y in range(S)] if children[b] else Dc[0][b])
            var["margin_a0j0"][i, b] = min(gf, gn)
            for k in range(K):
                var["counts_a0j1"][i, b, k] = float(N1[b][k][q // S][q % S])
                var["counts_a0j0"][i, b, k] = float(N1[b][k][xs][ys])
                var["counts_a1j0"][i, b, k] = float(mp.fsum(
                    post[f][cc][x] * mp.fsum(NC[cc][b][k][x][y] * post[b][cc][y] for y in range(S) if post[b][cc][y] != 0)
                    for cc in range(C) for x in range(S) if post[f][cc][x] != 0))
    out = dict(parent=c.parent, blen=c.blen, lot=c.lot, Q=c.Q, pi=c.pi, rates=c.rates, probs=c.probs, aln=aln, classes=cls,
               Bk=(c.Bk if c.Bk is not None else np.zeros((0, S, S))), clamp=np.array(c.clamp), counts=counts, logL=logL,
               post_rate=prate, rate_class=rclass, class_clear=clear)
    if variants:
        out.update(var)
    if S <= 7 and store_P:
        out["P"] = np.array([[to_np(P[cc][b]) for b in range(B)] for cc in range(C)])
    sp._P.clear()
    sp._J.clear()
    return {f"{name}.{k}": np.asarray(v) for k, v in out.items()}


def operators_of(gen):
    sp = spectrum(gen)
    ts = oe.operator_times(gen)
    for t in ts:
        sp.check_phi(t)
    out = {f"ops.{gen}.t": np.array(ts), f"ops.{gen}.P": np.array([to_np(sp.P(t)) for t in ts]),
           f"ops.{gen}.J": np.array([[to_np(sp.J(k, Bm, t)) for k, Bm in enumerate(sp.regs)] for t in ts])}
    sp._P.clear()
    sp._J.clear()
    return out


def write_npz(path, out):
    """fixed zip timestamps: the same results give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    only = sys.argv[1:]
    out = {}
    for gen in oe.OPERATOR_MODELS:
        if not only:
            t0 = time.time()
            out.update(operators_of(gen))
            print(f"operators of {gen} ({time.time() - t0:.0f} s)", flush=True)
    if not only:        # P at every r_c t_b of the 20-state ancestral cases, once per distinct time
        sp, ts = spectrum("protein"), oe.ancestral_times()
        out["anc.protein.t"], out["anc.protein.P"] = np.array(ts), np.array([to_np(sp.P(t)) for t in ts])
        sp._P.clear()
    for name in oe.CASES:
        if only and not any(name.startswith(o) for o in only):
            continue
        t0 = time.time()
        out.update(solve_case(name))
        print(f"{name} ({time.time() - t0:.0f} s)", flush=True)
    if only:            # a trial run of some cases: nothing is written
        sys.exit(0)
    write_npz(os.path.join(ROOT, "tests", "golden", "operator_edges.npz"), out)
