// The kernels of the plain-kernel stage, written once.  cmx_variants.hip includes this text twice, each time with
//   PLAIN_ARGS               the kernels' argument: PlainArgs, or ScaledArgs (PlainArgs and the two exponent arrays)
//   PLAIN_SCALING            the scaling policy of cmx_plain.h: NoScaling, or Exponents
//   PLAIN_OF(args)           the PlainArgs inside the argument
//   PLAIN_SCALING_OF(args)   the policy's data inside the argument
//   PLAIN_*_KERNEL           the seven entry points' names
// so that NAME<S>(PlainArgs) and scaled_NAME<S>(ScaledArgs) are the same statements, the policy's operations compiled out of
// the first (if constexpr).  Text included into the kernel, not a function the kernel calls: hipcc simplifies a function
// before it inlines it, so an inlined body is simplified twice, and its loops, registers and scalar loads then come out
// otherwise than in a kernel written out (DESIGN.md 4.5.4 has what that cost when it was tried).  No include guard.
// What each kernel computes: the opening comment of cmx_variants.hip.

template <int S>
__global__ __launch_bounds__(256) void PLAIN_INSIDE_KERNEL(const PLAIN_ARGS args) {
  using X = PLAIN_SCALING;
  const PlainArgs& a = PLAIN_OF(args);
  const X& sc = PLAIN_SCALING_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int c = blockIdx.y, nn = a.nn;
  const size_t ch = a.chunk;
  double* Dc = a.D + (size_t)c * nn * S * ch;
  double* Mc = a.M + (size_t)c * nn * S * ch;
  int32_t* ec = nullptr;
  if constexpr (X::on) ec = inside_exponents(sc) + (size_t)c * nn * ch;
  const uint32_t all = S >= 32 ? 0xffffffffu : ((1u << (S & 31)) - 1u);
  for (int n = 0; n < nn; ++n) {
    double d[S];
    int e = 0;
    if (a.first_child[n] < 0) {
      const unsigned code = a.aln[(size_t)a.taxon_of[n] * a.ld + a.site0 + j];
      if constexpr (S > 32) {   // plain path (padded states): no mask table, every code >= Sreal is an unknown
#pragma unroll
        for (int x = 0; x < S; ++x) d[x] = code < (unsigned)a.Sreal ? (double)((unsigned)x == code) : (double)(x < a.Sreal);
      } else {
        const unsigned row = code < (unsigned)(S + max_ambig(S)) ? code : (unsigned)(S + max_ambig(S) - 1);
        const uint32_t m = code < (unsigned)S ? (1u << code) : (a.masks ? a.masks[row] : all);
#pragma unroll
        for (int x = 0; x < S; ++x) d[x] = (double)((m >> x) & 1u);
      }
    } else {
#pragma unroll
      for (int x = 0; x < S; ++x) d[x] = 1.0;
      for (int k = a.first_child[n]; k >= 0; k = a.next_sib[k]) {
#pragma unroll
        for (int x = 0; x < S; ++x) d[x] *= Mc[((size_t)k * S + x) * ch + j];
        if constexpr (X::on) {
          e += ec[(size_t)k * ch + j];
          rescale<S>(d, e);
        }
      }
    }
#pragma unroll
    for (int x = 0; x < S; ++x) Dc[((size_t)n * S + x) * ch + j] = d[x];
    if constexpr (X::on) ec[(size_t)n * ch + j] = e;
    if (n != a.root) {
      const double* Pn = a.P + ((size_t)c * a.B + n) * S * S;
#pragma unroll
      for (int x = 0; x < S; ++x) {
        double s = 0.0;
#pragma unroll
        for (int z = 0; z < S; ++z) s += Pn[x * S + z] * d[z];
        Mc[((size_t)n * S + x) * ch + j] = s;
      }
    }
  }
}

template <int S>
__global__ __launch_bounds__(256) void PLAIN_OUTSIDE_KERNEL(const PLAIN_ARGS args) {
  using X = PLAIN_SCALING;
  const PlainArgs& a = PLAIN_OF(args);
  const X& sc = PLAIN_SCALING_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int c = blockIdx.y, nn = a.nn;
  const size_t ch = a.chunk;
  const double* Mc = a.M + (size_t)c * nn * S * ch;
  double* Uc = a.U + (size_t)c * nn * S * ch;
  double* Upc = a.Up + (size_t)c * nn * S * ch;
  const int32_t* edc = nullptr;
  int32_t* euc = nullptr;
  if constexpr (X::on) { edc = inside_exponents(sc) + (size_t)c * nn * ch; euc = outside_exponents(sc) + (size_t)c * nn * ch; }
#pragma unroll
  for (int x = 0; x < S; ++x) Upc[((size_t)a.root * S + x) * ch + j] = a.pi[x];
  if constexpr (X::on) euc[(size_t)a.root * ch + j] = 0;
  for (int f = nn - 1; f >= 0; --f) {
    if (a.first_child[f] < 0) continue;
    double upf[S];
#pragma unroll
    for (int x = 0; x < S; ++x) upf[x] = Upc[((size_t)f * S + x) * ch + j];
    int ef = 0;
    if constexpr (X::on) ef = euc[(size_t)f * ch + j];
    for (int n = a.first_child[f]; n >= 0; n = a.next_sib[n]) {
      double u[S];
      int e = ef;
#pragma unroll
      for (int x = 0; x < S; ++x) u[x] = upf[x];
      for (int m = a.first_child[f]; m >= 0; m = a.next_sib[m])
        if (m != n) {
#pragma unroll
          for (int x = 0; x < S; ++x) u[x] *= Mc[((size_t)m * S + x) * ch + j];
          if constexpr (X::on) {
            e += edc[(size_t)m * ch + j];
            rescale<S>(u, e);
          }
        }
#pragma unroll
      for (int x = 0; x < S; ++x) Uc[((size_t)n * S + x) * ch + j] = u[x];
      if constexpr (X::on) euc[(size_t)n * ch + j] = e;
      if (a.first_child[n] >= 0) {
        const double* Pn = a.P + ((size_t)c * a.B + n) * S * S;
#pragma unroll
        for (int z = 0; z < S; ++z) {
          double s = 0.0;
#pragma unroll
          for (int x = 0; x < S; ++x) s += Pn[x * S + z] * u[x];
          Upc[((size_t)n * S + z) * ch + j] = s;
        }
      }
    }
  }
}

template <int S>
__global__ __launch_bounds__(256) void PLAIN_PICK_KERNEL(const PLAIN_ARGS args) {
  const PlainArgs& a = PLAIN_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y, C = a.C;
  const int E = site_exponent<S>(args, j);
  double best = -__builtin_inf();
  int bidx = 0;
  for (int x = 0; x < S; ++x)
    for (int y = 0; y < S; ++y) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) {
        const double u = a.U[node_at<S>(a, c, b, x, j)];
        const double d = a.D[node_at<S>(a, c, b, y, j)];
        s += shifted(args, a.probs[c] * ((u * a.P[((size_t)c * a.B + b) * S * S + x * S + y]) * d), node_shift(args, c, b, j, E));
      }
      if (s > best) { best = s; bidx = x * S + y; }
    }
  for (int k = 0; k < a.K; ++k) a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = a.N1[((size_t)b * a.K + k) * S * S + bidx];
}

// ---- nijt.joint = no (computeSubstitutionVectorsMarginal / ...NoAveragingMarginal, CoETools.cpp:399-405).  Restated in
// oracle/oracle.c orc_map_sites_marginal (pinned to its definition by tests/test_oracle_marginal.py; parity unpinned against
// the reference, which ships no output of these variants):
//   post_n(c, x) = p_c Up_n(c, x) D_n(c, x) / L  at an internal node (DRTreeLikelihoodTools::
//   getPosteriorProbabilitiesPerStatePerRate: the likelihood re-rooted at the node; Up_root = pi), e(x) p_c / sum e at a leaf;
//   Marginal:            count(b, k) = sum_c sum_x sum_y post_f(c, x) post_n(c, y) N^k(x, y; r_c t_b)
//   NoAveragingMarginal: x*(n) = first maximum of sum_c post_n(c, x) (leaf: of e);  count(b, k) = N^k(x*(f), x*(n); t_b)
// One thread per (site, branch); same global scratch as the NoAveraging kernels above.
template <int S>
__global__ __launch_bounds__(256) void PLAIN_MARGINAL_KERNEL(const PLAIN_ARGS args) {
  const PlainArgs& a = PLAIN_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y, C = a.C, f = a.parent[b];
  const bool leaf = a.first_child[b] < 0;
  const SiteL sl = site_likelihood<S>(args, j);
  const double L = sl.L;
  double se = 0.0;
  if (leaf)
    for (int x = 0; x < S; ++x) se += a.D[node_at<S>(a, 0, b, x, j)];   // the leaf vector is the same in every class, exponent 0
  if (a.mode == PlainMode::Marginal) {
    for (int k = 0; k < a.K; ++k) {
      double v = 0.0;
      for (int c = 0; c < C; ++c) {
        const double* Nk = a.NC + (((size_t)c * a.B + b) * a.K + k) * S * S;
        const int sb = node_shift(args, c, b, j, sl.E), sf = node_shift(args, c, f, j, sl.E);
        double pn[S];
#pragma unroll
        for (int y = 0; y < S; ++y) {
          const double d = a.D[node_at<S>(a, c, b, y, j)];
          pn[y] = leaf ? d * a.probs[c] / se : shifted(args, a.Up[node_at<S>(a, c, b, y, j)] * d * a.probs[c], sb) / L;   // node_posterior, D loaded once for both arms
        }
        for (int x = 0; x < S; ++x) {
          const double pf = node_posterior<S>(args, c, f, x, j, sf, L);
          double s = 0.0;
#pragma unroll
          for (int y = 0; y < S; ++y) s += Nk[x * S + y] * pn[y];
          v += pf * s;
        }
      }
      a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = v;
    }
    return;
  }
  // PlainMode::NoAvgMarginal: marginal ancestral states of the father and of the node, first maximum over the states
  int xs = 0, ys = 0;
  double bf = -__builtin_inf(), bn = -__builtin_inf();
  for (int x = 0; x < S; ++x) {
    double sf = 0.0, sn = 0.0;
    for (int c = 0; c < C; ++c) {
      sf += node_posterior<S>(args, c, f, x, j, node_shift(args, c, f, j, sl.E), L);
      if (!leaf) sn += node_posterior<S>(args, c, b, x, j, node_shift(args, c, b, j, sl.E), L);
    }
    if (leaf) sn = a.D[node_at<S>(a, 0, b, x, j)];
    if (sf > bf) { bf = sf; xs = x; }
    if (sn > bn) { bn = sn; ys = x; }
  }
  for (int k = 0; k < a.K; ++k) a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = a.N1[((size_t)b * a.K + k) * S * S + xs * S + ys];
}

// ---- the default mapping (computeSubstitutionVectors: nijt.average = yes, nijt.joint = yes) on the same per-node vectors,
// for the alphabets the matrix-core walk does not serve (codon models, CoETools.cpp:95-100; SURVEY A.3 / A.4):
//   count(b, i, k) = sum_c p_c sum_xy U_b(i,c,x) (P o N^k)_c,b(x,y) D_n(i,c,y) / L_i
// One thread per (site, branch).
template <int S>
__global__ __launch_bounds__(256) void PLAIN_JOINT_KERNEL(const PLAIN_ARGS args) {
  const PlainArgs& a = PLAIN_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y;
  const SiteL sl = site_likelihood<S>(args, j);
  for (int k = 0; k < a.K; ++k) {
    double v = 0.0;
    for (int c = 0; c < a.C; ++c) {
      const double* PNk = a.PN + (((size_t)c * a.B + b) * a.K + k) * S * S;
      double d[S];
#pragma unroll
      for (int y = 0; y < S; ++y) d[y] = a.D[node_at<S>(a, c, b, y, j)];
      double vc = 0.0;
      for (int x = 0; x < S; ++x) {
        double s = 0.0;
#pragma unroll
        for (int y = 0; y < S; ++y) s += PNk[x * S + y] * d[y];
        vc += a.U[node_at<S>(a, c, b, x, j)] * s;
      }
      v += shifted(args, a.probs[c] * vc, node_shift(args, c, b, j, sl.E));
    }
    a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = v / sl.L;
  }
}
// site scalars: log-likelihood (ln L + E ln 2), posterior rate, rate class with the largest posterior (first maximum)
template <int S>
__global__ __launch_bounds__(256) void PLAIN_SCALARS_KERNEL(const PLAIN_ARGS args) {
  using X = PLAIN_SCALING;
  const PlainArgs& a = PLAIN_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int E = site_exponent<S>(args, j);
  double L = 0.0, pr = 0.0, best = -1.0;
  int bc = 0;
  for (int c = 0; c < a.C; ++c) {   // site_likelihood's sum, with every term kept for the rate and the class
    const double w = shifted(args, class_likelihood<S>(a, c, j), root_shift(args, c, j, E));
    L += w;
    pr += a.rates[c] * w;
    if (w > best) { best = w; bc = c; }
  }
  if constexpr (X::on) {
    if (a.logL) a.logL[a.site0 + j] = log(L) + (double)E * 0.693147180559945309417232121458;
  } else {
    if (a.logL) a.logL[a.site0 + j] = log(L);
  }
  if (a.post_rate) a.post_rate[a.site0 + j] = pr / L;
  if (a.rate_class) a.rate_class[a.site0 + j] = bc;
}

// ---- marginal ancestral state reconstruction (asr.method = marginal, CoMap/CoMap.cpp:169-197:
// LegacyMarginalAncestralStateReconstruction::getAncestralStatesForNode), on the per-node vectors of the two kernels above:
//   post_n(i, x) = sum_c p_c Up_n(i, c, x) D_n(i, c, x) / L_i   (Up_root = root frequencies)
//   state_n(i)   = first x that maximises post_n(i, x)            (VectorTools::whichMax: strict ">" scan)
// the posterior of marginal_kernel, summed in its order.  One thread per (site, internal node); states [n_inner][lds] and
// the optional posterior of the real states [n_inner][Sreal][ldp] are coalesced over sites.  L_i = 0: NaN, state 0.
template <int S>
__global__ __launch_bounds__(256) void PLAIN_ANCESTRAL_KERNEL(const PLAIN_ARGS args, const AncOut o) {
  const PlainArgs& a = PLAIN_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int q = blockIdx.y, n = o.inner[q];
  const SiteL sl = site_likelihood<S>(args, j);
  int best = 0;
  double bv = -__builtin_inf();
  for (int x = 0; x < a.Sreal; ++x) {
    double s = 0.0;
    for (int c = 0; c < a.C; ++c) s += node_posterior<S>(args, c, n, x, j, node_shift(args, c, n, j, sl.E), sl.L);
    if (o.post) o.post[((size_t)q * a.Sreal + x) * o.ldp + a.site0 + j] = s;
    if (s > bv) { bv = s; best = x; }
  }
  o.states[(size_t)q * o.lds + a.site0 + j] = (uint8_t)best;
}
