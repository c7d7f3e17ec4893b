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
//      cmx_debug_map_wide_plain(1) only.  Under likelihood scaling the same holds at 20 states too (cmx_map_wide20.hip,
//      launch_scaled_site_scalars, cmx_debug_map_scaled_plain).
//   4. marginal ancestral states (asr.method = marginal): ancestral_kernel.
// Every kernel is written once, in cmx_plain_kernels.inc, over a scaling policy (cmx_plain.h); this file includes that text
// twice, which gives each kernel two entry points: NAME<S>(PlainArgs) runs it without scaling, scaled_NAME<S>(ScaledArgs)
// with the exponents of a context with per-site likelihood scaling
// (cmx_set_likelihood_scaling, DESIGN.md 4.5.5: a tree beyond fp64's range -- the reference warns above ~500 sequences,
// CoMap/CoETools.cpp:235-262 -- maps at all).  The scaled entries serve every mode, the site scalars and the ancestral states
// at 4, 20 and kPlainStates states.  One dispatch on the state count (with_plain_states), one pass loop (plain_passes,
// cmx_plain_passes.h); what a change must keep: DESIGN.md 4.5.4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "cmx_plain.h"
#include "cmx_plain_passes.h"

namespace cmx {

namespace {

// what ancestral_kernel writes
struct AncOut {
  const int* inner;   // [n_inner] the internal nodes, ascending
  uint8_t* states; size_t lds;
  double* post; size_t ldp;   // NULL: states only
};

#define PLAIN_ARGS PlainArgs
#define PLAIN_SCALING NoScaling
#define PLAIN_OF(args) args
#define PLAIN_SCALING_OF(args) NoScaling{}
#define PLAIN_INSIDE_KERNEL noavg_inside_kernel
#define PLAIN_OUTSIDE_KERNEL noavg_outside_kernel
#define PLAIN_PICK_KERNEL noavg_pick_kernel
#define PLAIN_MARGINAL_KERNEL marginal_kernel
#define PLAIN_JOINT_KERNEL joint_kernel
#define PLAIN_SCALARS_KERNEL site_scalars_kernel
#define PLAIN_ANCESTRAL_KERNEL ancestral_kernel
#include "cmx_plain_kernels.inc"
#undef PLAIN_ARGS
#undef PLAIN_SCALING
#undef PLAIN_OF
#undef PLAIN_SCALING_OF
#undef PLAIN_INSIDE_KERNEL
#undef PLAIN_OUTSIDE_KERNEL
#undef PLAIN_PICK_KERNEL
#undef PLAIN_MARGINAL_KERNEL
#undef PLAIN_JOINT_KERNEL
#undef PLAIN_SCALARS_KERNEL
#undef PLAIN_ANCESTRAL_KERNEL

#define PLAIN_ARGS ScaledArgs
#define PLAIN_SCALING Exponents
#define PLAIN_OF(args) args.p
#define PLAIN_SCALING_OF(args) args.e
#define PLAIN_INSIDE_KERNEL scaled_inside_kernel
#define PLAIN_OUTSIDE_KERNEL scaled_outside_kernel
#define PLAIN_PICK_KERNEL scaled_noavg_pick_kernel
#define PLAIN_MARGINAL_KERNEL scaled_marginal_kernel
#define PLAIN_JOINT_KERNEL scaled_joint_kernel
#define PLAIN_SCALARS_KERNEL scaled_site_scalars_kernel
#define PLAIN_ANCESTRAL_KERNEL scaled_ancestral_kernel
#include "cmx_plain_kernels.inc"

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

// one launch on the vectors of a pass: the scaled entry point if the pass carries exponents, workgroups of 256 sites
template <class... Extra>
void launch_entry(void (*unscaled)(PlainArgs, Extra...), void (*scaled)(ScaledArgs, Extra...), const PlainPass& p, unsigned gy,
                  hipStream_t stream, Extra... extra) {
  if (p.eD) hipLaunchKernelGGL(scaled, dim3(p.gx, gy), dim3(256), 0, stream, ScaledArgs{p.a, {p.eD, p.eU}}, extra...);
  else hipLaunchKernelGGL(unscaled, dim3(p.gx, gy), dim3(256), 0, stream, p.a, extra...);
}

// the stage's own passes (plain_passes, cmx_plain_passes.h): the inside kernel; the site scalars, unscaled on the plain path only;
// the outside kernel and what `rest(pass)` launches on the finished vectors
template <int S, class F>
hipError_t stage_passes(const PlainArgs& a, size_t nsites_total, double* scratch, int32_t* exps, bool outside, hipStream_t stream, F rest) {
  return plain_passes(
      a, nsites_total, scratch, exps, outside,
      [&](const PlainPass& p) { launch_entry(noavg_inside_kernel<S>, scaled_inside_kernel<S>, p, p.a.C, stream); },
      [&](const PlainPass& p) {
        if (p.eD) hipLaunchKernelGGL(scaled_site_scalars_kernel<S>, dim3(p.gx), dim3(256), 0, stream, ScaledArgs{p.a, {p.eD, p.eU}});
        else if constexpr (S == kPlainStates) hipLaunchKernelGGL(site_scalars_kernel<S>, dim3(p.gx), dim3(256), 0, stream, p.a);
        return hipSuccess;
      },
      [&](const PlainPass& p) {
        launch_entry(noavg_outside_kernel<S>, scaled_outside_kernel<S>, p, p.a.C, stream);
        rest(p);
      });
}

}  // namespace

size_t plain_node_doubles(int S, int C, int nn, size_t chunk) { return 4 * (size_t)C * nn * S * chunk; }
size_t plain_exponent_ints(int C, int nn, size_t chunk) { return 2 * (size_t)C * nn * chunk; }
size_t plain_sites_per_pass(int S, int C, int nn, size_t nsites, size_t budget_bytes, bool balanced) {
  const size_t per_site = sizeof(double) * plain_node_doubles(S, C, nn, 1);
  const size_t most = std::max<size_t>(256, budget_bytes / per_site / 256 * 256);
  if (!balanced) return std::max<size_t>(256, std::min(nsites, most));
  const size_t passes = (nsites + most - 1) / most;
  return std::min(nsites, ((nsites + passes - 1) / passes + 255) / 256 * 256);
}

// the mapping: per pass the kernel of a.mode if counts are asked for, then the norms of all sites (which need the counts)
hipError_t launch_plain_map(PlainArgs a, size_t nsites_total, double* scratch, int32_t* exps, double* d_norm, hipStream_t stream) {
  return with_plain_states(a.S, [&](auto states) {
    constexpr int S = decltype(states)::value;
    void (*unscaled)(PlainArgs) = nullptr;
    void (*scaled)(ScaledArgs) = nullptr;
    switch (a.mode) {
      case PlainMode::NoAvg: unscaled = noavg_pick_kernel<S>; scaled = scaled_noavg_pick_kernel<S>; break;
      case PlainMode::Marginal:
      case PlainMode::NoAvgMarginal: unscaled = marginal_kernel<S>; scaled = scaled_marginal_kernel<S>; break;
      case PlainMode::Joint:   // (unscaled at 4 / 20 states the matrix-core walk's, not built here)
        scaled = scaled_joint_kernel<S>;
        if constexpr (S == kPlainStates) unscaled = joint_kernel<S>;
    }
    if (exps ? !scaled : !unscaled) return hipErrorInvalidValue;
    const hipError_t e = stage_passes<S>(a, nsites_total, scratch, exps, a.counts != nullptr, stream,
                                         [&](const PlainPass& p) { launch_entry(unscaled, scaled, p, p.a.B, stream); });
    if (e != hipSuccess) return e;
    if (d_norm && a.counts) return launch_counts_norm(a.counts, a.ldc, a.B, a.K, nsites_total, d_norm, stream);
    return hipGetLastError();
  });
}

hipError_t launch_plain_site_scalars(const PlainArgs& pass, hipStream_t stream) {
  if (pass.S != kPlainStates) return hipErrorInvalidValue;
  hipLaunchKernelGGL(site_scalars_kernel<kPlainStates>, dim3((unsigned)((pass.nsites + 255) / 256)), dim3(256), 0, stream, pass);
  return hipGetLastError();
}

hipError_t launch_scaled_site_scalars(const PlainArgs& pass, int32_t* eD, int32_t* eU, hipStream_t stream) {
  const dim3 grid((unsigned)((pass.nsites + 255) / 256));
  const ScaledArgs args{pass, {eD, eU}};
  if (pass.S == kPlainStates) hipLaunchKernelGGL(scaled_site_scalars_kernel<kPlainStates>, grid, dim3(256), 0, stream, args);
  else if (pass.S == 20) hipLaunchKernelGGL(scaled_site_scalars_kernel<20>, grid, dim3(256), 0, stream, args);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_counts_norm(const double* d_counts, size_t ldc, int B, int K, size_t n, double* d_norm, hipStream_t stream) {
  hipLaunchKernelGGL(counts_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_counts, ldc, B, K, n, d_norm);
  return hipGetLastError();
}

// asr.method = marginal: the inside and outside kernels of the mapping, unchanged, then ancestral_kernel per pass (a's model
// and alignment fields as the mapping fills them; no mapping output)
hipError_t launch_ancestral(PlainArgs a, size_t nsites_total, double* scratch, int32_t* exps, const int* d_inner, int n_inner,
                            uint8_t* d_states, size_t lds, double* d_post, size_t ldp, hipStream_t stream) {
  a.counts = nullptr; a.logL = a.post_rate = nullptr; a.rate_class = nullptr;
  const AncOut o{d_inner, d_states, lds, d_post, ldp};
  return with_plain_states(a.S, [&](auto states) {
    constexpr int S = decltype(states)::value;
    const hipError_t e = stage_passes<S>(a, nsites_total, scratch, exps, true, stream, [&](const PlainPass& p) {
      launch_entry(ancestral_kernel<S>, scaled_ancestral_kernel<S>, p, (unsigned)n_inner, stream, o);
    });
    return e != hipSuccess ? e : hipGetLastError();
  });
}

}  // namespace cmx
