// The 20-state shape of the wide mapping under likelihood scaling: the kernels of cmx_map_wide_kernels.inc at 20 device
// states with the Exponents policy (the opening comment of cmx_map_wide.hip has the layout and the rules).  A translation
// unit of its own: built beside the 64-state kernels in one unit, hipcc gave the unscaled wide_outside_kernel other text
// than its parent's.
#include "cmx_map_wide.h"

namespace cmx {

namespace {

#define WIDE_S 20
#define WIDE_ARGS ScaledArgs
#define WIDE_OF(args) args.p
#define WIDE_SCALING_OF(args) args.e
#define WIDE_INSIDE_KERNEL wide20_scaled_inside_kernel
#define WIDE_OUTSIDE_KERNEL wide20_scaled_outside_kernel
#define WIDE_LIKELIHOOD_KERNEL wide20_scaled_likelihood_kernel
#define WIDE_COUNTS_KERNEL wide20_scaled_counts_kernel
#include "cmx_map_wide_kernels.inc"

}  // namespace

hipError_t launch_wide20_scaled_map(const PlainArgs& a, const WideOps& o, size_t nsites_total, double* scratch, int32_t* exps, double* part,
                                    double* d_norm, hipStream_t stream) {
  if (a.S != 20 || a.mode != PlainMode::Joint || !exps) return hipErrorInvalidValue;
  const WideKernels<ScaledArgs> kn{wide20_scaled_inside_kernel, wide20_scaled_outside_kernel, wide20_scaled_likelihood_kernel, wide20_scaled_counts_kernel};
  return wide_passes(kn, a, o, nsites_total, scratch, exps, part, d_norm, stream);
}

}  // namespace cmx
