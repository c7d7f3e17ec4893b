// What the translation units of the wide mapping share (cmx_map_wide.hip: 64 device states without and with likelihood
// scaling; cmx_map_wide20.hip: 20 states with it): which sites and states a lane holds, the loads and stores of a vector, the
// product on v_mfma_f64_16x16x4_f64, the leaf gather, the exponents' rescale in this layout, and the host's pass loop.  The
// opening comment of cmx_map_wide.hip has the layout and the rules; the kernels are cmx_map_wide_kernels.inc.  Everything
// here is in the including unit's own namespace, like the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "cmx_plain.h"
#include "cmx_plain_passes.h"

namespace cmx {
namespace {

constexpr int kTileSites = 16;      // sites of a wave
// waves of a workgroup.  The waves share nothing, and a pass is small where the tree is large (1 024 sites at 64 taxa and four
// classes: 256 wave-tasks), so one wave per workgroup lets the dispatcher spread a pass over as many CUs as it has tiles.
constexpr int kTileWaves = 1;
typedef double d4 __attribute__((ext_vector_type(4)));

// the packed operators of a shape: doubles of one, (where an element lies: wide_op_offset, cmx_layout.h)
constexpr int wide_op_doubles(int S) { return S == 20 ? kWide20Rows * 20 : kPlainStates * kPlainStates; }

// which sites and states a lane holds
struct WideLane {
  int hi;        // lane >> 4: state 4 i + hi in register i
  int lane;
  size_t j;      // site of the pass
  bool live;     // j < a.nsites
  size_t at0;    // element (class, node 0, state hi, site j) of a per-node vector
};

template <int S>
__device__ __forceinline__ bool wide_lane(const PlainArgs& a, WideLane& w) {
  w.lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t t0 = ((size_t)blockIdx.x * kTileWaves + wave) * kTileSites;
  if (t0 >= a.nsites) return false;
  w.hi = w.lane >> 4;
  w.j = t0 + (w.lane & 15);
  w.live = w.j < a.nsites;
  w.at0 = ((size_t)blockIdx.y * a.nn * S + w.hi) * a.chunk + w.j;
  return true;
}
// node n's vector: register i at v[wide_at(..) + i * 4 * chunk]
template <int S>
__device__ __forceinline__ size_t wide_at(const PlainArgs& a, const WideLane& w, int n) { return w.at0 + (size_t)n * S * a.chunk; }

// (one branch around all the loads of a vector, so that they are in flight together)
template <int R>
__device__ __forceinline__ void wide_load(const double* __restrict__ v, size_t at, size_t ch, bool live, double idle, double (&x)[R]) {
#pragma unroll
  for (int i = 0; i < R; ++i) x[i] = idle;
  if (live) {
#pragma unroll
    for (int i = 0; i < R; ++i) x[i] = v[at + (size_t)i * 4 * ch];
  }
}
template <int R>
__device__ __forceinline__ void wide_store(double* __restrict__ v, size_t at, size_t ch, bool live, const double (&x)[R]) {
  if (live) {
#pragma unroll
    for (int i = 0; i < R; ++i) v[at + (size_t)i * 4 * ch] = x[i];
  }
}
template <int R>
__device__ __forceinline__ void wide_times(const double* __restrict__ v, size_t at, size_t ch, bool live, double (&x)[R]) {
  double m[R];
  wide_load(v, at, ch, live, 1.0, m);
#pragma unroll
  for (int i = 0; i < R; ++i) x[i] *= m[i];
}

// y = Op x for the 16 sites of the wave; op: the packed operator at this lane's element of step (0, 0).  The panels'
// accumulators are independent, so consecutive instructions never wait for each other's result.
template <int S>
__device__ __forceinline__ void wide_product(const double* __restrict__ op, const double (&x)[S / 4], double (&y)[S / 4]) {
  constexpr int kRegs = S / 4, kPanels = (S + 15) / 16;
  d4 acc[kPanels];
#pragma unroll
  for (int p = 0; p < kPanels; ++p) acc[p] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < kRegs; ++i) {
#pragma unroll
    for (int p = 0; p < kPanels; ++p) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[wide_op_offset(16 * p, 4 * i, S)], x[i], acc[p], 0, 0, 0);
  }
#pragma unroll
  for (int p = 0; p < kPanels; ++p) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (4 * p + q < kRegs) y[4 * p + q] = acc[p][q];
  }
}

// A leaf whose 16 symbols are all states: Op times a one-hot vector is column `code` of Op, gathered instead of multiplied.  0 + p
// is what the matrix instruction computes there (a -0 in the operator comes out as +0 in both), so a site has the same bits
// whichever way its tile goes.  op0: the packed operator's first double.
template <int S>
__device__ __forceinline__ void wide_column(const double* __restrict__ op0, unsigned code, int hi, double (&y)[S / 4]) {
#pragma unroll
  for (int i = 0; i < S / 4; ++i) y[i] = 0.0 + op0[wide_op_offset(4 * i + hi, (int)code, S)];
}
// a leaf's symbol (a site behind the last one: state 0, whose column is finite), and whether the whole tile is resolved
__device__ __forceinline__ bool wide_leaf_codes(const PlainArgs& a, const WideLane& w, int taxon, unsigned& code) {
  code = w.live ? a.aln[(size_t)taxon * a.ld + a.site0 + w.j] : 0u;
  return __all(code < (unsigned)a.Sreal);
}

// ---- Exponents.  e: the array at (class, node 0, this lane's site); the four lanes of a site read the same word
__device__ __forceinline__ int wide_exponent(const int32_t* e, size_t at, bool live) { return live ? e[at] : 0; }
__device__ __forceinline__ void wide_exponent_store(int32_t* e, size_t at, bool live, int v) {
  if (live) e[at] = v;
}
// rescale (cmx_plain.h) in this layout, per column of the tile
template <int R>
__device__ __forceinline__ void wide_rescale(double (&v)[R], int& e) {
  double m = v[0];
#pragma unroll
  for (int i = 1; i < R; ++i) m = v[i] > m ? v[i] : m;
  double t = __shfl_xor(m, 16, 64);
  m = t > m ? t : m;
  t = __shfl_xor(m, 32, 64);
  m = t > m ? t : m;
  const bool small = m > 0.0 && m < kRescaleBelow;
  if (__any(small)) {
    const int k = small ? ilogb(m) : 0;
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = ldexp(v[i], -k);
    e += k;
  }
}

// the four entry points of one (shape, policy)
template <class A>
struct WideKernels {
  void (*inside)(A, WideOps);
  void (*outside)(A, WideOps, double*);
  void (*likelihood)(A, double*);
  void (*counts)(A, const double*, const double*);
};
inline PlainArgs wide_args(const PlainPass& p, const PlainArgs*) { return p.a; }
inline ScaledArgs wide_args(const PlainPass& p, const ScaledArgs*) { return ScaledArgs{p.a, {p.eD, p.eU}}; }

// the plain stage's pass loop (plain_passes, cmx_plain_passes.h) with the wide kernels: per pass the inside kernel, the site
// scalars that are asked for (the stage's own kernel) and -- if counts are asked for -- the likelihood, the outside kernel
// and the class sum; then the norms of all sites
template <class A>
hipError_t wide_passes(const WideKernels<A>& kn, const PlainArgs& a, const WideOps& o, size_t nsites_total, double* scratch, int32_t* exps,
                       double* part, double* d_norm, hipStream_t stream) {
  double* lik = part + (size_t)a.C * a.B * a.K * a.chunk;
  const auto grid = [](const PlainPass& p) {
    const size_t tiles = (p.a.nsites + kTileSites - 1) / kTileSites;
    return dim3((unsigned)((tiles + kTileWaves - 1) / kTileWaves), p.a.C);
  };
  const hipError_t e = plain_passes(
      a, nsites_total, scratch, exps, a.counts != nullptr,
      [&](const PlainPass& p) { hipLaunchKernelGGL(kn.inside, grid(p), dim3(kTileWaves * 64), 0, stream, wide_args(p, (const A*)nullptr), o); },
      [&](const PlainPass& p) { return p.eD ? launch_scaled_site_scalars(p.a, p.eD, p.eU, stream) : launch_plain_site_scalars(p.a, stream); },
      [&](const PlainPass& p) {
        const A args = wide_args(p, (const A*)nullptr);
        hipLaunchKernelGGL(kn.likelihood, dim3(p.gx), dim3(256), 0, stream, args, lik);
        hipLaunchKernelGGL(kn.outside, grid(p), dim3(kTileWaves * 64), 0, stream, args, o, part);
        hipLaunchKernelGGL(kn.counts, dim3(p.gx, p.a.B), dim3(256), 0, stream, args, (const double*)part, (const double*)lik);
      });
  if (e != hipSuccess) return e;
  if (d_norm && a.counts) return launch_counts_norm(a.counts, a.ldc, a.B, a.K, nsites_total, d_norm, stream);
  return hipGetLastError();
}

}  // namespace
}  // namespace cmx
