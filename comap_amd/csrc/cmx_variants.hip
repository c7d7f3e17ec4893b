// The plain kernels: what the matrix-core walk of cmx_map.hip does not serve.  NOT the hot path: one thread per
// (site, class), (site, branch) or (site, internal node), every per-node vector in a global scratch of
// [class][node][state][site] (coalesced over sites; operators are wave-uniform and come through the scalar cache).  Four uses
// share the vectors of noavg_inside_kernel / noavg_outside_kernel, which keep the name of the first:
//   1. nijt.average = no, nijt.joint = yes (PlainMode::NoAvg, noavg_pick_kernel): LegacySubstitutionMappingTools::
//      computeSubstitutionVectorsNoAveraging (call sites CoMap/CoETools.cpp:395-403 for the observed data,
//      CoMap/AnalysisTools.cpp:598-610 inside the null).  "For benchmarking only" says the reference -- but it is the only
//      way it runs nijt = Label with the MI statistic (CoETools.cpp:577-588).
//        per branch b (father f, son n), site i:  pxy(x, y) = sum_c p_c U_b(i,c,x) P_c,b(x,y) D_n(i,c,y);
//        (x*, y*) = first maximum of pxy in row-major order (MatrixTools::whichMax);  count(b, i, k) = N^k(x*, y*; t_b).
//      The algorithm is bpp-phyl's (absent from the reference tree): restated in oracle/oracle.c orc_map_sites_noavg, which
//      tests/test_oracle_noavg.py pins to the definition by brute force; this file follows that restatement loop for loop.
//   2. nijt.joint = no (PlainMode::Marginal, PlainMode::NoAvgMarginal): marginal_kernel.
//   3. alphabets other than 4 / 20 states, padded to kPlainStates: the default mapping (PlainMode::Joint, joint_kernel) and the
//      site scalars (site_scalars_kernel).  At 4 / 20 states the scalars do not depend on the option and stay the walk's.
//      By default cmx_map_wide.hip serves this use on the matrix cores, inside the same passes and with site_scalars_kernel
//      itself (launch_plain_site_scalars); joint_kernel and the inside / outside kernels at 64 states run for it under
//      cmx_debug_map_wide_plain(1) only.
//   4. marginal ancestral states (asr.method = marginal): ancestral_kernel.
// One dispatch on the state count (with_plain_states), one pass loop (plain_passes); what a change must keep: DESIGN.md 4.5.4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "cmx_device.h"

namespace cmx {

namespace {

template <int S>
__global__ __launch_bounds__(256) void noavg_inside_kernel(const PlainArgs a) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int c = blockIdx.y, nn = a.nn;
  const size_t ch = a.chunk;
  double* Dc = a.D + (size_t)c * nn * S * ch;
  double* Mc = a.M + (size_t)c * nn * S * ch;
  const uint32_t all = S >= 32 ? 0xffffffffu : ((1u << (S & 31)) - 1u);
  for (int n = 0; n < nn; ++n) {
    double d[S];
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
      for (int e = a.first_child[n]; e >= 0; e = a.next_sib[e]) {
#pragma unroll
        for (int x = 0; x < S; ++x) d[x] *= Mc[((size_t)e * S + x) * ch + j];
      }
    }
#pragma unroll
    for (int x = 0; x < S; ++x) Dc[((size_t)n * S + x) * ch + j] = d[x];
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
__global__ __launch_bounds__(256) void noavg_outside_kernel(const PlainArgs a) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int c = blockIdx.y, nn = a.nn;
  const size_t ch = a.chunk;
  const double* Mc = a.M + (size_t)c * nn * S * ch;
  double* Uc = a.U + (size_t)c * nn * S * ch;
  double* Upc = a.Up + (size_t)c * nn * S * ch;
#pragma unroll
  for (int x = 0; x < S; ++x) Upc[((size_t)a.root * S + x) * ch + j] = a.pi[x];
  for (int f = nn - 1; f >= 0; --f) {
    if (a.first_child[f] < 0) continue;
    double upf[S];
#pragma unroll
    for (int x = 0; x < S; ++x) upf[x] = Upc[((size_t)f * S + x) * ch + j];
    for (int n = a.first_child[f]; n >= 0; n = a.next_sib[n]) {
      double u[S];
#pragma unroll
      for (int x = 0; x < S; ++x) u[x] = upf[x];
      for (int m = a.first_child[f]; m >= 0; m = a.next_sib[m])
        if (m != n) {
#pragma unroll
          for (int x = 0; x < S; ++x) u[x] *= Mc[((size_t)m * S + x) * ch + j];
        }
#pragma unroll
      for (int x = 0; x < S; ++x) Uc[((size_t)n * S + x) * ch + j] = u[x];
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

// ---- what the kernels below share, floating-point operands and their order as each kernel used to spell them out
// where element x of node n, class c, site j of a per-node vector (a.D, a.M, a.U, a.Up) lies
template <int S>
__device__ __forceinline__ size_t node_at(const PlainArgs& a, int c, int n, int x, size_t j) {
  return (((size_t)c * a.nn + n) * S + x) * a.chunk + j;
}
// p_c L_c(j): class c's share of the site likelihood
template <int S>
__device__ __forceinline__ double class_likelihood(const PlainArgs& a, int c, size_t j) {
  double s = 0.0;
  for (int x = 0; x < S; ++x) s += a.pi[x] * a.D[node_at<S>(a, c, a.root, x, j)];
  return a.probs[c] * s;
}
template <int S>
__device__ __forceinline__ double site_likelihood(const PlainArgs& a, size_t j) {
  double L = 0.0;
  for (int c = 0; c < a.C; ++c) L += class_likelihood<S>(a, c, j);
  return L;
}
// class c's term of the posterior of state x at an internal node n (or the root): Up D p_c / L
template <int S>
__device__ __forceinline__ double node_posterior(const PlainArgs& a, int c, int n, int x, size_t j, double L) {
  return a.Up[node_at<S>(a, c, n, x, j)] * a.D[node_at<S>(a, c, n, x, j)] * a.probs[c] / L;
}

template <int S>
__global__ __launch_bounds__(256) void noavg_pick_kernel(const PlainArgs a) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y, C = a.C;
  double best = -__builtin_inf();
  int bidx = 0;
  for (int x = 0; x < S; ++x)
    for (int y = 0; y < S; ++y) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) {
        const double u = a.U[node_at<S>(a, c, b, x, j)];
        const double d = a.D[node_at<S>(a, c, b, y, j)];
        s += a.probs[c] * ((u * a.P[((size_t)c * a.B + b) * S * S + x * S + y]) * d);
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
__global__ __launch_bounds__(256) void marginal_kernel(const PlainArgs a) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y, C = a.C, f = a.parent[b];
  const bool leaf = a.first_child[b] < 0;
  const double L = site_likelihood<S>(a, j);
  double se = 0.0;
  if (leaf)
    for (int x = 0; x < S; ++x) se += a.D[node_at<S>(a, 0, b, x, j)];   // the leaf vector is the same in every class
  if (a.mode == PlainMode::Marginal) {
    for (int k = 0; k < a.K; ++k) {
      double v = 0.0;
      for (int c = 0; c < C; ++c) {
        const double* Nk = a.NC + (((size_t)c * a.B + b) * a.K + k) * S * S;
        double pn[S];
#pragma unroll
        for (int y = 0; y < S; ++y) {
          const double d = a.D[node_at<S>(a, c, b, y, j)];
          pn[y] = leaf ? d * a.probs[c] / se : a.Up[node_at<S>(a, c, b, y, j)] * d * a.probs[c] / L;   // node_posterior, D loaded once for both arms
        }
        for (int x = 0; x < S; ++x) {
          const double pf = node_posterior<S>(a, c, f, x, j, L);
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
      sf += node_posterior<S>(a, c, f, x, j, L);
      if (!leaf) sn += node_posterior<S>(a, c, b, x, j, L);
    }
    if (leaf) sn = a.D[node_at<S>(a, 0, b, x, j)];
    if (sf > bf) { bf = sf; xs = x; }
    if (sn > bn) { bn = sn; ys = x; }
  }
  for (int k = 0; k < a.K; ++k) a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = a.N1[((size_t)b * a.K + k) * S * S + xs * S + ys];
}

// ---- the default mapping (computeSubstitutionVectors: nijt.average = yes, nijt.joint = yes) on the same per-node vectors,
// for the alphabets the matrix-core walk does not serve (codon models, CoETools.cpp:95-100):
//   count(b, i, k) = sum_c p_c sum_xy U_b(i,c,x) (P o N^k)_c,b(x,y) D_n(i,c,y) / L_i
// One thread per (site, branch).
template <int S>
__global__ __launch_bounds__(256) void joint_kernel(const PlainArgs a) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y;
  const double L = site_likelihood<S>(a, j);
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
      v += a.probs[c] * vc;
    }
    a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = v / L;
  }
}
// site scalars of the plain path: log-likelihood, posterior rate, rate class with the largest posterior (first maximum)
template <int S>
__global__ __launch_bounds__(256) void site_scalars_kernel(const PlainArgs a) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  double L = 0.0, pr = 0.0, best = -1.0;
  int bc = 0;
  for (int c = 0; c < a.C; ++c) {   // site_likelihood's sum, with every term kept for the rate and the class
    const double w = class_likelihood<S>(a, c, j);
    L += w;
    pr += a.rates[c] * w;
    if (w > best) { best = w; bc = c; }
  }
  if (a.logL) a.logL[a.site0 + j] = log(L);
  if (a.post_rate) a.post_rate[a.site0 + j] = pr / L;
  if (a.rate_class) a.rate_class[a.site0 + j] = bc;
}

// ---- marginal ancestral state reconstruction (asr.method = marginal, CoMap/CoMap.cpp:169-197:
// LegacyMarginalAncestralStateReconstruction::getAncestralStatesForNode), on the per-node vectors of the two kernels above:
//   post_n(i, x) = sum_c p_c Up_n(i, c, x) D_n(i, c, x) / L_i   (Up_root = root frequencies)
//   state_n(i)   = first x that maximises post_n(i, x)            (VectorTools::whichMax: strict ">" scan)
// the posterior of marginal_kernel, summed in its order.  One thread per (site, internal node); states [n_inner][lds] and
// the optional posterior of the real states [n_inner][Sreal][ldp] are coalesced over sites.  L_i = 0: NaN, state 0.
struct AncOut {
  const int* inner;   // [n_inner] the internal nodes, ascending
  uint8_t* states; size_t lds;
  double* post; size_t ldp;   // NULL: states only
};

template <int S>
__global__ __launch_bounds__(256) void ancestral_kernel(const PlainArgs a, const AncOut o) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int q = blockIdx.y, n = o.inner[q];
  const double L = site_likelihood<S>(a, j);
  int best = 0;
  double bv = -__builtin_inf();
  for (int x = 0; x < a.Sreal; ++x) {
    double s = 0.0;
    for (int c = 0; c < a.C; ++c) s += node_posterior<S>(a, c, n, x, j, L);
    if (o.post) o.post[((size_t)q * a.Sreal + x) * o.ldp + a.site0 + j] = s;
    if (s > bv) { bv = s; best = x; }
  }
  o.states[(size_t)q * o.lds + a.site0 + j] = (uint8_t)best;
}

// computeNormForSite over the (branch-major) counts: sqrt(sum_b (sum_k count)^2), branches in order
__global__ __launch_bounds__(256) void counts_norm_kernel(const double* __restrict__ counts, size_t ldc, int B, int K, size_t n,
                                                          double* __restrict__ norm) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double nrm = 0.0;
  for (int b = 0; b < B; ++b) {
    double tot = 0.0;
    for (int k = 0; k < K; ++k) tot += counts[((size_t)b * K + k) * ldc + j];
    nrm += tot * tot;
  }
  norm[j] = sqrt(nrm);
}

// the one dispatch on the device state count: f(std::integral_constant<int, S>) for the three sizes the kernels are built for
template <class F>
hipError_t with_plain_states(int S, F f) {
  if (S == 20) return f(std::integral_constant<int, 20>{});
  if (S == 4) return f(std::integral_constant<int, 4>{});
  if (S == kPlainStates) return f(std::integral_constant<int, kPlainStates>{});
  return hipErrorInvalidValue;
}

// the one pass loop: D, M, U, Up carved from the scratch (plain_node_doubles), then a.chunk sites per pass: the inside kernel,
// on the plain path the site scalars that are asked for, and -- only if `outside` -- the outside kernel and what
// `rest(a, gx)` launches on the finished vectors of the pass (gx: workgroups of 256 sites)
template <int S, class F>
void plain_passes(PlainArgs a, size_t nsites_total, double* scratch, bool outside, hipStream_t stream, F rest) {
  const size_t per = plain_node_doubles(S, a.C, a.nn, a.chunk) / 4;
  a.D = scratch; a.M = scratch + per; a.U = scratch + 2 * per; a.Up = scratch + 3 * per;
  for (a.site0 = 0; a.site0 < nsites_total; a.site0 += a.chunk) {
    a.nsites = std::min(a.chunk, nsites_total - a.site0);
    const unsigned gx = (unsigned)((a.nsites + 255) / 256);
    hipLaunchKernelGGL(noavg_inside_kernel<S>, dim3(gx, a.C), dim3(256), 0, stream, a);
    if constexpr (S == kPlainStates)
      if (a.logL || a.post_rate || a.rate_class) hipLaunchKernelGGL(site_scalars_kernel<S>, dim3(gx), dim3(256), 0, stream, a);
    if (!outside) continue;
    hipLaunchKernelGGL(noavg_outside_kernel<S>, dim3(gx, a.C), dim3(256), 0, stream, a);
    rest(a, gx);
  }
}

}  // namespace

size_t plain_node_doubles(int S, int C, int nn, size_t chunk) { return 4 * (size_t)C * nn * S * chunk; }
size_t plain_sites_per_pass(int S, int C, int nn, size_t nsites, size_t budget_bytes, bool balanced) {
  const size_t per_site = sizeof(double) * plain_node_doubles(S, C, nn, 1);
  const size_t most = std::max<size_t>(256, budget_bytes / per_site / 256 * 256);
  if (!balanced) return std::max<size_t>(256, std::min(nsites, most));
  const size_t passes = (nsites + most - 1) / most;
  return std::min(nsites, ((nsites + passes - 1) / passes + 255) / 256 * 256);
}

// the mapping: per pass the kernel of a.mode if counts are asked for, then the norms of all sites (which need the counts)
hipError_t launch_plain_map(PlainArgs a, size_t nsites_total, double* scratch, double* d_norm, hipStream_t stream) {
  return with_plain_states(a.S, [&](auto states) {
    constexpr int S = decltype(states)::value;
    void (*mode_kernel)(PlainArgs) = nullptr;
    switch (a.mode) {
      case PlainMode::NoAvg: mode_kernel = noavg_pick_kernel<S>; break;
      case PlainMode::Marginal:
      case PlainMode::NoAvgMarginal: mode_kernel = marginal_kernel<S>; break;
      case PlainMode::Joint:   // (at 4 / 20 states the matrix-core walk's, not built here)
        if constexpr (S == kPlainStates) mode_kernel = joint_kernel<S>;
    }
    if (!mode_kernel) return hipErrorInvalidValue;
    plain_passes<S>(a, nsites_total, scratch, a.counts != nullptr, stream, [&](const PlainArgs& pass, unsigned gx) {
      hipLaunchKernelGGL(mode_kernel, dim3(gx, pass.B), dim3(256), 0, stream, pass);
    });
    if (d_norm && a.counts) return launch_counts_norm(a.counts, a.ldc, a.B, a.K, nsites_total, d_norm, stream);
    return hipGetLastError();
  });
}

hipError_t launch_plain_site_scalars(const PlainArgs& pass, hipStream_t stream) {
  if (pass.S != kPlainStates) return hipErrorInvalidValue;
  hipLaunchKernelGGL(site_scalars_kernel<kPlainStates>, dim3((unsigned)((pass.nsites + 255) / 256)), dim3(256), 0, stream, pass);
  return hipGetLastError();
}

hipError_t launch_counts_norm(const double* d_counts, size_t ldc, int B, int K, size_t n, double* d_norm, hipStream_t stream) {
  hipLaunchKernelGGL(counts_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_counts, ldc, B, K, n, d_norm);
  return hipGetLastError();
}

// asr.method = marginal: the inside and outside kernels of the mapping, unchanged, then ancestral_kernel per pass (a's model
// and alignment fields as the mapping fills them; no mapping output)
hipError_t launch_ancestral(PlainArgs a, size_t nsites_total, double* scratch, const int* d_inner, int n_inner, uint8_t* d_states,
                            size_t lds, double* d_post, size_t ldp, hipStream_t stream) {
  a.counts = nullptr; a.logL = a.post_rate = nullptr; a.rate_class = nullptr;
  const AncOut o{d_inner, d_states, lds, d_post, ldp};
  return with_plain_states(a.S, [&](auto states) {
    plain_passes<decltype(states)::value>(a, nsites_total, scratch, true, stream, [&](const PlainArgs& pass, unsigned gx) {
      hipLaunchKernelGGL(ancestral_kernel<decltype(states)::value>, dim3(gx, n_inner), dim3(256), 0, stream, pass, o);
    });
    return hipGetLastError();
  });
}

}  // namespace cmx
