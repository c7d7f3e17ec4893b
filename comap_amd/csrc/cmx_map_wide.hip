// The default mapping (computeSubstitutionVectors: nijt.average = yes, nijt.joint = yes) and the root vectors of the site
// scalars on v_mfma_f64_16x16x4_f64, inside the plain stage's pass structure, for
//   - the alphabets the matrix-core walk of cmx_map.hip does not serve (2 .. 64 states other than 4 / 20: codon models,
//     CoETools.cpp:95-100), states padded to kPlainStates = 64, without and with per-site likelihood scaling;
//   - 20-state models under likelihood scaling (cmx_set_likelihood_scaling), where the walk is not used.
// The arithmetic and the pass structure are the plain stage's (cmx_variants.hip: noavg_inside_kernel, noavg_outside_kernel,
// joint_kernel; per-node vectors [class][node][state][chunk] in the same scratch); the three S x S by S x sites products run
// on the matrix instruction:
//   inside   D_n = prod_{children e} M_e  (leaf: indicator / unknown = 1 on the real states),   M_n = P_{c,n} D_n
//   outside  U_n = Up_f o prod_{siblings m != n} M_m,   Up_n = P_{c,n}^T U_n,   Up_root = pi
//   counts   count(b, k) = [ sum_c p_c sum_x U_b(x) ((P o N^k)_{c,b} D_b)(x) ] / L
// One wave owns 16 sites of one rate class and follows first_child / next_sib as the plain kernels do.  Column = site, k = row
// = state (cmx_map.hip "The 64-site protein walk" has the measured layout): a vector of S states is S / 4 registers per lane,
// register i of lane l = state 4 i + (l >> 4) of site l & 15.  Register q of output panel p holds state 16 p + 4 q + (l >> 4) =
// register 4 p + q of the same layout, so a product's result is the next product's input as it stands.
//   64 states: 16 registers, a product is 4 panels x 16 k-steps = 64 instructions, operators packed by wide_op_offset.
//   20 states:  5 registers (every one valid in every lane), 2 panels x 5 k-steps = 10 instructions, operators packed by
//               wide20_op_offset as 32 x 20 with rows 20 .. 31 zero: the accumulator registers of states 20 .. 31 come out
//               zero and are never read, loaded or stored.  Leaves read the caller's ambiguity table (a.masks).
// Each step's A operand is 64 consecutive doubles (cmx_layout.h).
// A lane reads back from the scratch only what it stored itself (M of the children, Up of the father), so the kernels need no
// barrier; U stays in registers (the count contraction sits in the outside kernel), D of every node and Up of the internal
// nodes reach memory.  Sites behind the call's last one (a partial tile) load nothing from the scratch, store nothing and hold
// finite values.  A leaf whose tile is fully resolved gathers its symbols' columns of the operator instead of multiplying.
// Classes run in different waves: per-class partial counts go to [C][B*K][chunk] and the class-sum kernel adds them in the
// order c = 0 .. C-1, then divides by L, as joint_kernel does.  No atomics; a site's results depend on its column alone.
//
// Likelihood scaling (the Exponents policy of cmx_plain.h, whose rule this restates): eD per (class, node, site) shared by D
// and M, eU shared by U and Up, in the stage's [C][nn][chunk] arrays.  A node's exponent starts as the sum of its children's, an
// outside exponent as eU[father] + sum eD[sibling], eU[root] = 0.  After every factor of a product the vector's largest
// element m -- the maximum of a lane's registers, then of the site's four lanes by __shfl_xor 16 and 32; a maximum has no
// order -- is looked at: 0 < m < kRescaleBelow: every element times 2^-ilogb(m), exponent += ilogb(m).  The rescale is per
// column (k = 0 where a column does not rescale, ldexp(v, 0) is exact) behind a wave-uniform __any, so a tile in which no
// column rescales runs the unscaled instructions.  Padded states hold 0, never 1 (a 1 would block every rescale); the idle
// columns of a partial tile hold 1.0 and exponent 0 and touch no memory.  All four lanes of a site hold the same exponent and
// store the identical word, so each reads back a word it stored itself: no barrier for the exponents either.  eU of every
// node reaches memory (the class sum needs it).  The likelihood kernel stores L and its exponent E; the class sum is
// scaled_joint_kernel's statement, v += shifted(probs[c] * part, eU + eD - E); the site scalars are
// scaled_site_scalars_kernel itself (launch_scaled_site_scalars).  The kernels are written once, over the state shape and the
// policy, in cmx_map_wide_kernels.inc; this unit builds them at 64 states without and with the exponents, cmx_map_wide20.hip
// at 20 states with them (why a unit of its own: its opening comment), and cmx_map_wide.h holds what the two share.
#include <hip/hip_runtime.h>

#include <atomic>

#include "cmx_map_wide.h"

namespace cmx {

static std::atomic<int> g_map_wide_plain{0};   // cmx_debug_map_wide_plain
int map_wide_plain(int on) {
  const int was = g_map_wide_plain.load();
  if (on >= 0) g_map_wide_plain.store(on ? 1 : 0);
  return was;
}
static std::atomic<int> g_map_scaled_plain{0};   // cmx_debug_map_scaled_plain
int map_scaled_plain(int on) {
  const int was = g_map_scaled_plain.load();
  if (on >= 0) g_map_scaled_plain.store(on ? 1 : 0);
  return was;
}

size_t wide_part_doubles(int C, int B, int K, size_t chunk) { return ((size_t)C * B * K + 1) * chunk; }
size_t wide_scaled_part_bytes(int C, int B, int K, size_t chunk) {
  return wide_part_doubles(C, B, K, chunk) * sizeof(double) + chunk * sizeof(int32_t);
}

namespace {

#define WIDE_S kPlainStates
#define WIDE_ARGS PlainArgs
#define WIDE_OF(args) args
#define WIDE_SCALING_OF(args) NoScaling{}
#define WIDE_INSIDE_KERNEL wide_inside_kernel
#define WIDE_OUTSIDE_KERNEL wide_outside_kernel
#define WIDE_LIKELIHOOD_KERNEL wide_likelihood_kernel
#define WIDE_COUNTS_KERNEL wide_counts_kernel
#include "cmx_map_wide_kernels.inc"
#undef WIDE_ARGS
#undef WIDE_OF
#undef WIDE_SCALING_OF
#undef WIDE_INSIDE_KERNEL
#undef WIDE_OUTSIDE_KERNEL
#undef WIDE_LIKELIHOOD_KERNEL
#undef WIDE_COUNTS_KERNEL

#define WIDE_ARGS ScaledArgs
#define WIDE_OF(args) args.p
#define WIDE_SCALING_OF(args) args.e
#define WIDE_INSIDE_KERNEL wide_scaled_inside_kernel
#define WIDE_OUTSIDE_KERNEL wide_scaled_outside_kernel
#define WIDE_LIKELIHOOD_KERNEL wide_scaled_likelihood_kernel
#define WIDE_COUNTS_KERNEL wide_scaled_counts_kernel
#include "cmx_map_wide_kernels.inc"

}  // namespace

// exps null: the unscaled kernels (a.S == kPlainStates; part: wide_part_doubles doubles).  exps: the scaled ones at kPlainStates
// or 20 states (part: wide_scaled_part_bytes bytes, the likelihoods' exponents behind the likelihoods).
hipError_t launch_wide_map(PlainArgs a, const WideOps& o, size_t nsites_total, double* scratch, int32_t* exps, double* part,
                           double* d_norm, hipStream_t stream) {
  if (a.mode != PlainMode::Joint) return hipErrorInvalidValue;
  if (!exps) {
    if (a.S != kPlainStates) return hipErrorInvalidValue;
    const WideKernels<PlainArgs> kn{wide_inside_kernel, wide_outside_kernel, wide_likelihood_kernel, wide_counts_kernel};
    return wide_passes(kn, a, o, nsites_total, scratch, exps, part, d_norm, stream);
  }
  if (a.S == kPlainStates) {
    const WideKernels<ScaledArgs> kn{wide_scaled_inside_kernel, wide_scaled_outside_kernel, wide_scaled_likelihood_kernel, wide_scaled_counts_kernel};
    return wide_passes(kn, a, o, nsites_total, scratch, exps, part, d_norm, stream);
  }
  if (a.S == 20) return launch_wide20_scaled_map(a, o, nsites_total, scratch, exps, part, d_norm, stream);
  return hipErrorInvalidValue;
}

}  // namespace cmx
