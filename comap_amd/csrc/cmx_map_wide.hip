// The default mapping (computeSubstitutionVectors: nijt.average = yes, nijt.joint = yes) and the root vectors of the site
// scalars for the alphabets the matrix-core walk of cmx_map.hip does not serve (2 .. 64 states other than 4 / 20: codon
// models, CoETools.cpp:95-100), states padded to kPlainStates = 64, without likelihood scaling.  The arithmetic and the pass
// structure are the plain stage's (cmx_variants.hip: noavg_inside_kernel, noavg_outside_kernel, joint_kernel; per-node
// vectors [class][node][state][chunk] in the same scratch); the three 64 x 64 by 64 x sites products run on
// v_mfma_f64_16x16x4_f64:
//   inside   D_n = prod_{children e} M_e  (leaf: indicator / unknown = 1 on the real states),   M_n = P_{c,n} D_n
//   outside  U_n = Up_f o prod_{siblings m != n} M_m,   Up_n = P_{c,n}^T U_n,   Up_root = pi
//   counts   count(b, k) = [ sum_c p_c sum_x U_b(x) ((P o N^k)_{c,b} D_b)(x) ] / L
// One wave owns 16 sites of one rate class and follows first_child / next_sib as the plain kernels do.  Column = site, k = row
// = state (cmx_map.hip "The 64-site protein walk" has the measured layout): a vector of 64 states is 16 registers per lane,
// register i of lane l = state 4 i + (l >> 4) of site l & 15.  Register q of output panel p holds state 16 p + 4 q + (l >> 4) =
// register 4 p + q of the same layout, so a product's result is the next product's input as it stands.  A product is 4 panels
// x 16 k-steps = 64 instructions; its A operands are 64 consecutive doubles each (cmx_layout.h: wide_op_offset).
// A lane reads back from the scratch only what it stored itself (M of the children, Up of the father), so the kernels need no
// barrier; U stays in registers (the count contraction sits in the outside kernel), D of every node and Up of the internal
// nodes reach memory.  Sites behind the call's last one (a partial tile) load nothing from the scratch, store nothing and hold
// finite values.  A leaf whose tile is fully resolved gathers its symbols' columns of the operator instead of multiplying.
// Classes run in different waves: per-class partial counts go to [C][B*K][chunk] and wide_counts_kernel sums them in the
// order c = 0 .. C-1, then divides by L, as joint_kernel does.  No atomics; a site's results depend on its column alone.
#include <hip/hip_runtime.h>

#include <atomic>

#include "cmx_plain.h"
#include "cmx_plain_passes.h"

namespace cmx {

static std::atomic<int> g_map_wide_plain{0};   // cmx_debug_map_wide_plain
int map_wide_plain(int on) {
  const int was = g_map_wide_plain.load();
  if (on >= 0) g_map_wide_plain.store(on ? 1 : 0);
  return was;
}

size_t wide_part_doubles(int C, int B, int K, size_t chunk) { return ((size_t)C * B * K + 1) * chunk; }

namespace {

constexpr int S = kPlainStates;
constexpr int kRegs = S / 4;        // registers of a vector per lane
constexpr int kTileSites = 16;      // sites of a wave
// waves of a workgroup.  The waves share nothing, and a pass is small where the tree is large (1 024 sites at 64 taxa and four
// classes: 256 wave-tasks), so one wave per workgroup lets the dispatcher spread a pass over as many CUs as it has tiles.
constexpr int kTileWaves = 1;
typedef double d4 __attribute__((ext_vector_type(4)));

// which sites and states a lane holds
struct WideLane {
  int hi;        // lane >> 4: state 4 i + hi in register i
  int lane;
  size_t j;      // site of the pass
  bool live;     // j < a.nsites
  size_t at0;    // element (class, node 0, state hi, site j) of a per-node vector
};

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
__device__ __forceinline__ size_t wide_at(const PlainArgs& a, const WideLane& w, int n) { return w.at0 + (size_t)n * S * a.chunk; }

// (one branch around all sixteen loads, so that they are in flight together)
__device__ __forceinline__ void wide_load(const double* __restrict__ v, size_t at, size_t ch, bool live, double idle, double (&x)[kRegs]) {
#pragma unroll
  for (int i = 0; i < kRegs; ++i) x[i] = idle;
  if (live) {
#pragma unroll
    for (int i = 0; i < kRegs; ++i) x[i] = v[at + (size_t)i * 4 * ch];
  }
}
__device__ __forceinline__ void wide_store(double* __restrict__ v, size_t at, size_t ch, bool live, const double (&x)[kRegs]) {
  if (live) {
#pragma unroll
    for (int i = 0; i < kRegs; ++i) v[at + (size_t)i * 4 * ch] = x[i];
  }
}
__device__ __forceinline__ void wide_times(const double* __restrict__ v, size_t at, size_t ch, bool live, double (&x)[kRegs]) {
  double m[kRegs];
  wide_load(v, at, ch, live, 1.0, m);
#pragma unroll
  for (int i = 0; i < kRegs; ++i) x[i] *= m[i];
}

// y = Op x for the 16 sites of the wave; op: the packed operator (wide_op_offset) at this lane's element of step (0, 0).  The four
// panels' accumulators are independent, so consecutive instructions never wait for each other's result.
__device__ __forceinline__ void wide_product(const double* __restrict__ op, const double (&x)[kRegs], double (&y)[kRegs]) {
  d4 acc[S / 16];
#pragma unroll
  for (int p = 0; p < S / 16; ++p) acc[p] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < kRegs; ++i) {
#pragma unroll
    for (int p = 0; p < S / 16; ++p) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[wide_op_offset(16 * p, 4 * i)], x[i], acc[p], 0, 0, 0);
  }
#pragma unroll
  for (int p = 0; p < S / 16; ++p) {
#pragma unroll
    for (int q = 0; q < 4; ++q) y[4 * p + q] = acc[p][q];
  }
}

// A leaf whose 16 symbols are all states: Op times a one-hot vector is column `code` of Op, gathered instead of multiplied.  0 + p
// is what the matrix instruction computes there (a -0 in the operator comes out as +0 in both), so a site has the same bits
// whichever way its tile goes.  op0: the packed operator's first double.
__device__ __forceinline__ void wide_column(const double* __restrict__ op0, unsigned code, int hi, double (&y)[kRegs]) {
#pragma unroll
  for (int i = 0; i < kRegs; ++i) y[i] = 0.0 + op0[wide_op_offset(4 * i + hi, (int)code)];
}
// a leaf's symbol (a site behind the last one: state 0, whose column is finite), and whether the whole tile is resolved
__device__ __forceinline__ bool wide_leaf_codes(const PlainArgs& a, const WideLane& w, int taxon, unsigned& code) {
  code = w.live ? a.aln[(size_t)taxon * a.ld + a.site0 + w.j] : 0u;
  return __all(code < (unsigned)a.Sreal);
}

__global__ __launch_bounds__(kTileWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void wide_inside_kernel(const PlainArgs a, const WideOps o) {
  WideLane w;
  if (!wide_lane(a, w)) return;
  const int c = blockIdx.y;
  const size_t ch = a.chunk;
  const cmx_cint first_child = (cmx_cint)a.first_child, next_sib = (cmx_cint)a.next_sib, taxon_of = (cmx_cint)a.taxon_of;
  const double* opP = o.P + (size_t)c * a.B * S * S;
  const size_t lane_at = wide_op_offset(w.lane & 15, w.hi);
  for (int n = 0; n < a.nn; ++n) {
    double d[kRegs];
    unsigned code = 0;
    bool resolved = false;
    if (first_child[n] < 0) {   // every code >= Sreal is an unknown
      resolved = wide_leaf_codes(a, w, taxon_of[n], code);
#pragma unroll
      for (int i = 0; i < kRegs; ++i) {
        const unsigned x = 4 * i + w.hi;
        d[i] = code < (unsigned)a.Sreal ? (double)(x == code) : (double)(x < (unsigned)a.Sreal);
      }
    } else {
#pragma unroll
      for (int i = 0; i < kRegs; ++i) d[i] = 1.0;
      for (int e = first_child[n]; e >= 0; e = next_sib[e]) wide_times(a.M, wide_at(a, w, e), ch, w.live, d);
    }
    wide_store(a.D, wide_at(a, w, n), ch, w.live, d);
    if (n != a.root) {
      double m[kRegs];
      if (resolved) wide_column(opP + (size_t)n * S * S, code, w.hi, m);
      else wide_product(opP + (size_t)n * S * S + lane_at, d, m);
      wide_store(a.M, wide_at(a, w, n), ch, w.live, m);
    }
  }
}

// part: [C][B*K][chunk] class c's sum_x U_b(x) ((P o N^k)_{c,b} D_b)(x)
__global__ __launch_bounds__(kTileWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void wide_outside_kernel(const PlainArgs a, const WideOps o, double* __restrict__ part) {
  WideLane w;
  if (!wide_lane(a, w)) return;
  const int c = blockIdx.y;
  const size_t ch = a.chunk;
  const cmx_cint first_child = (cmx_cint)a.first_child, next_sib = (cmx_cint)a.next_sib, taxon_of = (cmx_cint)a.taxon_of;
  const size_t lane_at = wide_op_offset(w.lane & 15, w.hi);
  const double* opPT = o.PT + (size_t)c * a.B * S * S + lane_at;
  const double* opPN = o.PN + (size_t)c * a.B * a.K * S * S;
  double* partc = part + (size_t)c * a.B * a.K * ch + w.j;
  for (int f = a.nn - 1; f >= 0; --f) {
    if (first_child[f] < 0) continue;
    double upf[kRegs];
    if (f == a.root) {
#pragma unroll
      for (int i = 0; i < kRegs; ++i) upf[i] = a.pi[4 * i + w.hi];
    } else {
      wide_load(a.Up, wide_at(a, w, f), ch, w.live, 1.0, upf);
    }
    for (int n = first_child[f]; n >= 0; n = next_sib[n]) {
      double u[kRegs];
#pragma unroll
      for (int i = 0; i < kRegs; ++i) u[i] = upf[i];
      for (int m = first_child[f]; m >= 0; m = next_sib[m])
        if (m != n) wide_times(a.M, wide_at(a, w, m), ch, w.live, u);
      if (first_child[n] >= 0) {
        double up[kRegs];
        wide_product(opPT + (size_t)n * S * S, u, up);
        wide_store(a.Up, wide_at(a, w, n), ch, w.live, up);
      }
      double d[kRegs];
      unsigned code = 0;
      const bool resolved = first_child[n] < 0 && wide_leaf_codes(a, w, taxon_of[n], code);
      if (!resolved) wide_load(a.D, wide_at(a, w, n), ch, w.live, 1.0, d);
      for (int k = 0; k < a.K; ++k) {
        double t[kRegs];
        if (resolved) wide_column(opPN + ((size_t)n * a.K + k) * S * S, code, w.hi, t);
        else wide_product(opPN + ((size_t)n * a.K + k) * S * S + lane_at, d, t);
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < kRegs; ++i) s += u[i] * t[i];
        s += __shfl_xor(s, 16, 64);   // the four state groups of a site: (0 + 1) + (2 + 3) in every lane
        s += __shfl_xor(s, 32, 64);
        if (w.live && w.hi == 0) partc[((size_t)n * a.K + k) * ch] = s;
      }
    }
  }
}

// the site likelihood (site_likelihood, cmx_plain.h), once per site for wide_counts_kernel
__global__ __launch_bounds__(256) void wide_likelihood_kernel(const PlainArgs a, double* __restrict__ lik) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  lik[j] = site_likelihood<S>(a, j).L;
}

// class terms in the order c = 0 .. C-1, then the division by L (joint_kernel's order); one thread per (site, branch)
__global__ __launch_bounds__(256) void wide_counts_kernel(const PlainArgs a, const double* __restrict__ part, const double* __restrict__ lik) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y;
  const double L = lik[j];
  for (int k = 0; k < a.K; ++k) {
    const size_t row = (size_t)b * a.K + k;
    double v = 0.0;
    for (int c = 0; c < a.C; ++c) v += a.probs[c] * part[((size_t)c * a.B * a.K + row) * a.chunk + j];
    a.counts[row * a.ldc + a.site0 + j] = v / L;
  }
}

}  // namespace

// the plain stage's pass loop (plain_passes, cmx_plain_passes.h) with the wide kernels: per pass the inside kernel, the site
// scalars that are asked for (site_scalars_kernel itself) and -- if counts are asked for -- the likelihood, the outside kernel
// and the class sum; then the norms of all sites
hipError_t launch_wide_map(PlainArgs a, const WideOps& o, size_t nsites_total, double* scratch, double* part, double* d_norm,
                           hipStream_t stream) {
  if (a.S != S || a.mode != PlainMode::Joint) return hipErrorInvalidValue;
  double* lik = part + (size_t)a.C * a.B * a.K * a.chunk;
  const auto grid = [](const PlainPass& p) {
    const size_t tiles = (p.a.nsites + kTileSites - 1) / kTileSites;
    return dim3((unsigned)((tiles + kTileWaves - 1) / kTileWaves), p.a.C);
  };
  const hipError_t e = plain_passes(
      a, nsites_total, scratch, nullptr, a.counts != nullptr,
      [&](const PlainPass& p) { hipLaunchKernelGGL(wide_inside_kernel, grid(p), dim3(kTileWaves * 64), 0, stream, p.a, o); },
      [&](const PlainPass& p) { return launch_plain_site_scalars(p.a, stream); },
      [&](const PlainPass& p) {
        hipLaunchKernelGGL(wide_likelihood_kernel, dim3(p.gx), dim3(256), 0, stream, p.a, lik);
        hipLaunchKernelGGL(wide_outside_kernel, grid(p), dim3(kTileWaves * 64), 0, stream, p.a, o, part);
        hipLaunchKernelGGL(wide_counts_kernel, dim3(p.gx, p.a.B), dim3(256), 0, stream, p.a, (const double*)part, (const double*)lik);
      });
  if (e != hipSuccess) return e;
  if (d_norm && a.counts) return launch_counts_norm(a.counts, a.ldc, a.B, a.K, nsites_total, d_norm, stream);
  return hipGetLastError();
}

}  // namespace cmx
