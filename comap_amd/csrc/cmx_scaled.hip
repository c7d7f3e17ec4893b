// The plain kernels of cmx_variants.hip with per-site likelihood scaling (cmx_set_likelihood_scaling): the
// same threads, the same per-node vectors in the same global scratch, and beside them one int32 exponent per (class, node,
// site) for the inside vector (eD: D, shared by M = P D) and one for the outside vector (eU: U, shared by Up).  The true value
// of a stored element is  stored * 2^exponent.  NOT the hot path; it exists so that a tree beyond fp64's range (the reference
// warns above ~500 sequences, CoMap/CoETools.cpp:235-262) maps at all.
//   - a vector is rescaled after EVERY factor of its product (a node may have any number of children; one node's product
//     alone can underflow): m = max over the states; 0 < m < kRescaleBelow: every element times 2^-ilogb(m), exponent +=
//     ilogb(m).  Only powers of two, no log / exp: where nothing falls below the threshold every exponent is 0 and the
//     arithmetic is the unscaled kernels' (up to FMA contraction around the ldexp of a class term).
//   - every sum over the rate classes (L, the rate class, the posterior rate, the counts, noavg's pxy, the posteriors)
//     brings its terms to the exponent E of the site likelihood with ldexp, in the unscaled order.  E = the largest root
//     exponent among the classes whose share of the likelihood is positive (a class the data are impossible under stops
//     rescaling and would otherwise hold an exponent the others vanish against).  A term 1 074 binades below the largest
//     vanishes, which is correct.
//   - L = 0 in every class (data impossible under the model): logL = -inf, NaN counts, ancestral state 0, as unscaled.
// Kernels for 4, 20 and kPlainStates states, all four mapping options, the site scalars and the ancestral states.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <type_traits>

#include "cmx_device.h"

namespace cmx {

namespace {

// PlainArgs and the two exponent arrays, [C][nn][chunk] each, carved from the caller's second scratch
struct ScaledArgs {
  PlainArgs p;
  int32_t *eD, *eU;
};

constexpr double kRescaleBelow = 0x1p-256;   // a vector whose largest element is below this is brought back to [1, 2)

template <int S>
__device__ __forceinline__ void rescale(double (&v)[S], int& e) {
  double m = v[0];
#pragma unroll
  for (int x = 1; x < S; ++x) m = v[x] > m ? v[x] : m;
  if (m > 0.0 && m < kRescaleBelow) {
    const int k = ilogb(m);
#pragma unroll
    for (int x = 0; x < S; ++x) v[x] = ldexp(v[x], -k);
    e += k;
  }
}

__device__ __forceinline__ size_t exp_at(const ScaledArgs& a, int c, int n, size_t j) {
  return ((size_t)c * a.p.nn + n) * a.p.chunk + j;
}
template <int S>
__device__ __forceinline__ size_t node_at(const PlainArgs& a, int c, int n, int x, size_t j) {
  return (((size_t)c * a.nn + n) * S + x) * a.chunk + j;
}

template <int S>
__global__ __launch_bounds__(256) void scaled_inside_kernel(const ScaledArgs sa) {
  const PlainArgs& a = sa.p;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int c = blockIdx.y, nn = a.nn;
  const size_t ch = a.chunk;
  double* Dc = a.D + (size_t)c * nn * S * ch;
  double* Mc = a.M + (size_t)c * nn * S * ch;
  int32_t* ec = sa.eD + (size_t)c * nn * ch;
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
        e += ec[(size_t)k * ch + j];
        rescale<S>(d, e);
      }
    }
#pragma unroll
    for (int x = 0; x < S; ++x) Dc[((size_t)n * S + x) * ch + j] = d[x];
    ec[(size_t)n * ch + j] = e;
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
__global__ __launch_bounds__(256) void scaled_outside_kernel(const ScaledArgs sa) {
  const PlainArgs& a = sa.p;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int c = blockIdx.y, nn = a.nn;
  const size_t ch = a.chunk;
  const double* Mc = a.M + (size_t)c * nn * S * ch;
  double* Uc = a.U + (size_t)c * nn * S * ch;
  double* Upc = a.Up + (size_t)c * nn * S * ch;
  const int32_t* edc = sa.eD + (size_t)c * nn * ch;
  int32_t* euc = sa.eU + (size_t)c * nn * ch;
#pragma unroll
  for (int x = 0; x < S; ++x) Upc[((size_t)a.root * S + x) * ch + j] = a.pi[x];
  euc[(size_t)a.root * ch + j] = 0;
  for (int f = nn - 1; f >= 0; --f) {
    if (a.first_child[f] < 0) continue;
    double upf[S];
#pragma unroll
    for (int x = 0; x < S; ++x) upf[x] = Upc[((size_t)f * S + x) * ch + j];
    const int ef = euc[(size_t)f * ch + j];
    for (int n = a.first_child[f]; n >= 0; n = a.next_sib[n]) {
      double u[S];
      int e = ef;
#pragma unroll
      for (int x = 0; x < S; ++x) u[x] = upf[x];
      for (int m = a.first_child[f]; m >= 0; m = a.next_sib[m])
        if (m != n) {
#pragma unroll
          for (int x = 0; x < S; ++x) u[x] *= Mc[((size_t)m * S + x) * ch + j];
          e += edc[(size_t)m * ch + j];
          rescale<S>(u, e);
        }
#pragma unroll
      for (int x = 0; x < S; ++x) Uc[((size_t)n * S + x) * ch + j] = u[x];
      euc[(size_t)n * ch + j] = e;
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

// ---- the class sums.  p_c L_c(j) as stored (true value: times 2^eD[c][root][j])
template <int S>
__device__ __forceinline__ double class_likelihood(const PlainArgs& a, int c, size_t j) {
  double s = 0.0;
  for (int x = 0; x < S; ++x) s += a.pi[x] * a.D[node_at<S>(a, c, a.root, x, j)];
  return a.probs[c] * s;
}
// the site likelihood L * 2^E: E from the classes with a positive share, the terms summed in class order at that exponent
struct SiteL { double L; int E; };
template <int S>
__device__ __forceinline__ int site_exponent(const ScaledArgs& sa, size_t j) {
  int E = INT_MIN;
  for (int c = 0; c < sa.p.C; ++c)
    if (class_likelihood<S>(sa.p, c, j) > 0.0) E = max(E, sa.eD[exp_at(sa, c, sa.p.root, j)]);
  return E == INT_MIN ? 0 : E;
}
template <int S>
__device__ __forceinline__ SiteL site_likelihood(const ScaledArgs& sa, size_t j) {
  SiteL r{0.0, site_exponent<S>(sa, j)};
  for (int c = 0; c < sa.p.C; ++c) r.L += ldexp(class_likelihood<S>(sa.p, c, j), sa.eD[exp_at(sa, c, sa.p.root, j)] - r.E);
  return r;
}
// what brings a product of an outside and an inside element of node n, class c, to the site likelihood's exponent
__device__ __forceinline__ int node_shift(const ScaledArgs& sa, int c, int n, size_t j, int E) {
  return sa.eU[exp_at(sa, c, n, j)] + sa.eD[exp_at(sa, c, n, j)] - E;
}
// class c's term of the posterior of state x at an internal node n (or the root): Up D p_c / L
template <int S>
__device__ __forceinline__ double node_posterior(const ScaledArgs& sa, int c, int n, int x, size_t j, int shift, double L) {
  const PlainArgs& a = sa.p;
  return ldexp(a.Up[node_at<S>(a, c, n, x, j)] * a.D[node_at<S>(a, c, n, x, j)] * a.probs[c], shift) / L;
}

template <int S>
__global__ __launch_bounds__(256) void scaled_noavg_pick_kernel(const ScaledArgs sa) {
  const PlainArgs& a = sa.p;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y, C = a.C;
  const int E = site_exponent<S>(sa, j);
  double best = -__builtin_inf();
  int bidx = 0;
  for (int x = 0; x < S; ++x)
    for (int y = 0; y < S; ++y) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) {
        const double u = a.U[node_at<S>(a, c, b, x, j)];
        const double d = a.D[node_at<S>(a, c, b, y, j)];
        s += ldexp(a.probs[c] * ((u * a.P[((size_t)c * a.B + b) * S * S + x * S + y]) * d), node_shift(sa, c, b, j, E));
      }
      if (s > best) { best = s; bidx = x * S + y; }
    }
  for (int k = 0; k < a.K; ++k) a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = a.N1[((size_t)b * a.K + k) * S * S + bidx];
}

template <int S>
__global__ __launch_bounds__(256) void scaled_marginal_kernel(const ScaledArgs sa) {
  const PlainArgs& a = sa.p;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y, C = a.C, f = a.parent[b];
  const bool leaf = a.first_child[b] < 0;
  const SiteL sl = site_likelihood<S>(sa, j);
  const double L = sl.L;
  double se = 0.0;
  if (leaf)
    for (int x = 0; x < S; ++x) se += a.D[node_at<S>(a, 0, b, x, j)];   // the leaf vector is the same in every class, exponent 0
  if (a.mode == PlainMode::Marginal) {
    for (int k = 0; k < a.K; ++k) {
      double v = 0.0;
      for (int c = 0; c < C; ++c) {
        const double* Nk = a.NC + (((size_t)c * a.B + b) * a.K + k) * S * S;
        const int sb = node_shift(sa, c, b, j, sl.E), sf = node_shift(sa, c, f, j, sl.E);
        double pn[S];
#pragma unroll
        for (int y = 0; y < S; ++y) {
          const double d = a.D[node_at<S>(a, c, b, y, j)];
          pn[y] = leaf ? d * a.probs[c] / se : ldexp(a.Up[node_at<S>(a, c, b, y, j)] * d * a.probs[c], sb) / L;
        }
        for (int x = 0; x < S; ++x) {
          const double pf = node_posterior<S>(sa, c, f, x, j, sf, L);
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
      sf += node_posterior<S>(sa, c, f, x, j, node_shift(sa, c, f, j, sl.E), L);
      if (!leaf) sn += node_posterior<S>(sa, c, b, x, j, node_shift(sa, c, b, j, sl.E), L);
    }
    if (leaf) sn = a.D[node_at<S>(a, 0, b, x, j)];
    if (sf > bf) { bf = sf; xs = x; }
    if (sn > bn) { bn = sn; ys = x; }
  }
  for (int k = 0; k < a.K; ++k) a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = a.N1[((size_t)b * a.K + k) * S * S + xs * S + ys];
}

// the default mapping: count(b, i, k) = sum_c p_c sum_xy U_b(i,c,x) (P o N^k)_c,b(x,y) D_n(i,c,y) / L_i
template <int S>
__global__ __launch_bounds__(256) void scaled_joint_kernel(const ScaledArgs sa) {
  const PlainArgs& a = sa.p;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y;
  const SiteL sl = site_likelihood<S>(sa, j);
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
      v += ldexp(a.probs[c] * vc, node_shift(sa, c, b, j, sl.E));
    }
    a.counts[((size_t)b * a.K + k) * a.ldc + a.site0 + j] = v / sl.L;
  }
}

// log-likelihood ln(L) + E ln 2, posterior rate, rate class with the largest posterior (first maximum)
template <int S>
__global__ __launch_bounds__(256) void scaled_site_scalars_kernel(const ScaledArgs sa) {
  const PlainArgs& a = sa.p;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int E = site_exponent<S>(sa, j);
  double L = 0.0, pr = 0.0, best = -1.0;
  int bc = 0;
  for (int c = 0; c < a.C; ++c) {
    const double w = ldexp(class_likelihood<S>(a, c, j), sa.eD[exp_at(sa, c, a.root, j)] - E);
    L += w;
    pr += a.rates[c] * w;
    if (w > best) { best = w; bc = c; }
  }
  if (a.logL) a.logL[a.site0 + j] = log(L) + (double)E * 0.693147180559945309417232121458;
  if (a.post_rate) a.post_rate[a.site0 + j] = pr / L;
  if (a.rate_class) a.rate_class[a.site0 + j] = bc;
}

struct AncOut {
  const int* inner;   // [n_inner] the internal nodes, ascending
  uint8_t* states; size_t lds;
  double* post; size_t ldp;   // NULL: states only
};

template <int S>
__global__ __launch_bounds__(256) void scaled_ancestral_kernel(const ScaledArgs sa, const AncOut o) {
  const PlainArgs& a = sa.p;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int q = blockIdx.y, n = o.inner[q];
  const SiteL sl = site_likelihood<S>(sa, j);
  int best = 0;
  double bv = -__builtin_inf();
  for (int x = 0; x < a.Sreal; ++x) {
    double s = 0.0;
    for (int c = 0; c < a.C; ++c) s += node_posterior<S>(sa, c, n, x, j, node_shift(sa, c, n, j, sl.E), sl.L);
    if (o.post) o.post[((size_t)q * a.Sreal + x) * o.ldp + a.site0 + j] = s;
    if (s > bv) { bv = s; best = x; }
  }
  o.states[(size_t)q * o.lds + a.site0 + j] = (uint8_t)best;
}

template <class F>
hipError_t with_scaled_states(int S, F f) {
  if (S == 20) return f(std::integral_constant<int, 20>{});
  if (S == 4) return f(std::integral_constant<int, 4>{});
  if (S == kPlainStates) return f(std::integral_constant<int, kPlainStates>{});
  return hipErrorInvalidValue;
}

// the pass loop of cmx_variants.hip's plain_passes with the exponents: the vectors carved from `scratch` as there, eD and eU
// from `exps` (plain_exponent_ints); the site scalars that are asked for at every state count
template <int S, class F>
void scaled_passes(PlainArgs p, size_t nsites_total, double* scratch, int32_t* exps, bool outside, hipStream_t stream, F rest) {
  const size_t per = plain_node_doubles(S, p.C, p.nn, p.chunk) / 4;
  p.D = scratch; p.M = scratch + per; p.U = scratch + 2 * per; p.Up = scratch + 3 * per;
  ScaledArgs a{p, exps, exps + plain_exponent_ints(p.C, p.nn, p.chunk) / 2};
  for (a.p.site0 = 0; a.p.site0 < nsites_total; a.p.site0 += a.p.chunk) {
    a.p.nsites = std::min(a.p.chunk, nsites_total - a.p.site0);
    const unsigned gx = (unsigned)((a.p.nsites + 255) / 256);
    hipLaunchKernelGGL(scaled_inside_kernel<S>, dim3(gx, p.C), dim3(256), 0, stream, a);
    if (p.logL || p.post_rate || p.rate_class) hipLaunchKernelGGL(scaled_site_scalars_kernel<S>, dim3(gx), dim3(256), 0, stream, a);
    if (!outside) continue;
    hipLaunchKernelGGL(scaled_outside_kernel<S>, dim3(gx, p.C), dim3(256), 0, stream, a);
    rest(a, gx);
  }
}

}  // namespace

size_t plain_exponent_ints(int C, int nn, size_t chunk) { return 2 * (size_t)C * nn * chunk; }

hipError_t launch_scaled_map(PlainArgs a, size_t nsites_total, double* scratch, int32_t* exps, double* d_norm, hipStream_t stream) {
  return with_scaled_states(a.S, [&](auto states) {
    constexpr int S = decltype(states)::value;
    void (*mode_kernel)(ScaledArgs) = nullptr;
    switch (a.mode) {
      case PlainMode::NoAvg: mode_kernel = scaled_noavg_pick_kernel<S>; break;
      case PlainMode::Marginal:
      case PlainMode::NoAvgMarginal: mode_kernel = scaled_marginal_kernel<S>; break;
      case PlainMode::Joint: mode_kernel = scaled_joint_kernel<S>; break;
    }
    if (!mode_kernel) return hipErrorInvalidValue;
    scaled_passes<S>(a, nsites_total, scratch, exps, a.counts != nullptr, stream, [&](const ScaledArgs& pass, unsigned gx) {
      hipLaunchKernelGGL(mode_kernel, dim3(gx, pass.p.B), dim3(256), 0, stream, pass);
    });
    if (d_norm && a.counts) return launch_counts_norm(a.counts, a.ldc, a.B, a.K, nsites_total, d_norm, stream);
    return hipGetLastError();
  });
}

hipError_t launch_scaled_ancestral(PlainArgs a, size_t nsites_total, double* scratch, int32_t* exps, const int* d_inner, int n_inner,
                                   uint8_t* d_states, size_t lds, double* d_post, size_t ldp, hipStream_t stream) {
  a.counts = nullptr; a.logL = a.post_rate = nullptr; a.rate_class = nullptr;
  const AncOut o{d_inner, d_states, lds, d_post, ldp};
  return with_scaled_states(a.S, [&](auto states) {
    constexpr int S = decltype(states)::value;
    scaled_passes<S>(a, nsites_total, scratch, exps, true, stream, [&](const ScaledArgs& pass, unsigned gx) {
      hipLaunchKernelGGL(scaled_ancestral_kernel<S>, dim3(gx, n_inner), dim3(256), 0, stream, pass, o);
    });
    return hipGetLastError();
  });
}

}  // namespace cmx
