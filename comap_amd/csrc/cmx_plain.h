// What the kernels of the plain-kernel stage share (cmx_plain_kernels.inc in cmx_variants.hip; cmx_map_wide.hip for the site
// likelihood): where an element of a per-node vector lies, the class sums, and the scaling policy the kernels are written
// over.  Device code.
//   NoScaling   holds nothing; each operation below is the identity and is compiled out, so an unscaled kernel has no
//               exponent load, no rescale and no ldexp.
//   Exponents   per-site likelihood scaling (cmx_set_likelihood_scaling): beside the per-node vectors one
//               int32 exponent per (class, node, site) for the inside vector (eD: D, shared by M = P D) and one for the
//               outside vector (eU: U, shared by Up).  The true value of a stored element is  stored * 2^exponent.
//   - a vector is rescaled after EVERY factor of its product (a node may have any number of children; one node's product
//     alone can underflow): m = max over the states; 0 < m < kRescaleBelow: every element times 2^-ilogb(m), exponent +=
//     ilogb(m).  Only powers of two, no log / exp: where nothing falls below the threshold every exponent is 0 and the
//     arithmetic is NoScaling's (up to FMA contraction around the ldexp of a class term).
//   - every sum over the rate classes (L, the rate class, the posterior rate, the counts, noavg's pxy, the posteriors)
//     brings its terms to the exponent E of the site likelihood with ldexp, in the unscaled order.  E = the largest root
//     exponent among the classes whose share of the likelihood is positive (a class the data are impossible under stops
//     rescaling and would otherwise hold an exponent the others vanish against).  A term 1 074 binades below the largest
//     vanishes, which is correct.
//   - L = 0 in every class (data impossible under the model): logL = -inf, NaN counts, ancestral state 0, in both policies.
#pragma once
#include <climits>
#include <type_traits>

#include "cmx_device.h"

namespace cmx {

struct NoScaling {
  static constexpr bool on = false;
};
struct Exponents {
  static constexpr bool on = true;
  int32_t *eD, *eU;   // [C][nn][chunk] each, carved from the caller's second scratch by the pass loop
};

// (for a kernel whose policy is not a template parameter: its discarded `if constexpr` arms are still checked)
template <class X>
__device__ __forceinline__ int32_t* inside_exponents(const X& sc) {
  if constexpr (X::on) return sc.eD;
  else return nullptr;
}
template <class X>
__device__ __forceinline__ int32_t* outside_exponents(const X& sc) {
  if constexpr (X::on) return sc.eU;
  else return nullptr;
}

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

// where element x of node n, class c, site j of a per-node vector (a.D, a.M, a.U, a.Up) lies, and the node's exponent
template <int S>
__device__ __forceinline__ size_t node_at(const PlainArgs& a, int c, int n, int x, size_t j) {
  return (((size_t)c * a.nn + n) * S + x) * a.chunk + j;
}
__device__ __forceinline__ size_t exp_at(const PlainArgs& a, int c, int n, size_t j) { return ((size_t)c * a.nn + n) * a.chunk + j; }

// ---- the kernels' argument.  Unscaled: PlainArgs itself.  Scaled: PlainArgs and the two exponent arrays (in this
// translation unit's own namespace, like the kernels that take it).  The helpers below take either, whole: a helper that got
// the exponent arrays through a second reference came out of hipcc with other registers than the kernels had before.
namespace {
struct ScaledArgs {
  PlainArgs p;
  Exponents e;
};
}  // namespace
__device__ __forceinline__ const PlainArgs& plain_of(const PlainArgs& a) { return a; }
__device__ __forceinline__ const PlainArgs& plain_of(const ScaledArgs& sa) { return sa.p; }
template <class A>
using ScalingOf = std::conditional_t<std::is_same_v<A, PlainArgs>, NoScaling, Exponents>;

// a class term brought to another exponent
template <class A>
__device__ __forceinline__ double shifted(const A&, double v, int shift) {
  if constexpr (ScalingOf<A>::on) return ldexp(v, shift);
  else return v;
}
// what brings class c's share of the likelihood, or a product of an outside and an inside element of its node n, to the
// site likelihood's exponent E
template <class A>
__device__ __forceinline__ int root_shift(const A& args, int c, size_t j, int E) {
  if constexpr (ScalingOf<A>::on) return args.e.eD[exp_at(args.p, c, args.p.root, j)] - E;
  else return 0;
}
template <class A>
__device__ __forceinline__ int node_shift(const A& args, int c, int n, size_t j, int E) {
  if constexpr (ScalingOf<A>::on) return args.e.eU[exp_at(args.p, c, n, j)] + args.e.eD[exp_at(args.p, c, n, j)] - E;
  else return 0;
}

// ---- the class sums.  p_c L_c(j): class c's share of the site likelihood as stored (true value: times 2^eD[c][root][j])
template <int S>
__device__ __forceinline__ double class_likelihood(const PlainArgs& a, int c, size_t j) {
  double s = 0.0;
  for (int x = 0; x < S; ++x) s += a.pi[x] * a.D[node_at<S>(a, c, a.root, x, j)];
  return a.probs[c] * s;
}
// the site likelihood L * 2^E: E from the classes with a positive share, the terms summed in class order at that exponent
struct SiteL { double L; int E; };
template <int S, class A>
__device__ __forceinline__ int site_exponent(const A& args, size_t j) {
  if constexpr (ScalingOf<A>::on) {
    int E = INT_MIN;
    for (int c = 0; c < args.p.C; ++c)
      if (class_likelihood<S>(args.p, c, j) > 0.0) E = max(E, args.e.eD[exp_at(args.p, c, args.p.root, j)]);
    return E == INT_MIN ? 0 : E;
  } else {
    return 0;
  }
}
template <int S, class A>
__device__ __forceinline__ SiteL site_likelihood(const A& args, size_t j) {
  SiteL r{0.0, site_exponent<S>(args, j)};
  for (int c = 0; c < plain_of(args).C; ++c) r.L += shifted(args, class_likelihood<S>(plain_of(args), c, j), root_shift(args, c, j, r.E));
  return r;
}
// class c's term of the posterior of state x at an internal node n (or the root): Up D p_c / L, shift = node_shift of (c, n)
template <int S, class A>
__device__ __forceinline__ double node_posterior(const A& args, int c, int n, int x, size_t j, int shift, double L) {
  const PlainArgs& a = plain_of(args);
  return shifted(args, a.Up[node_at<S>(a, c, n, x, j)] * a.D[node_at<S>(a, c, n, x, j)] * a.probs[c], shift) / L;
}

}  // namespace cmx
