// The kernels of the wide mapping, written once over the state shape and the scaling policy.  cmx_map_wide.hip includes this
// text once per (shape, policy) it builds, each time with
//   WIDE_S                  device states: kPlainStates (16 registers per vector, 4 panels x 16 k-steps) or 20 (5 registers,
//                           2 panels x 5 k-steps; the registers of states 20 .. 31 are constant zero, never loaded or stored)
//   WIDE_ARGS               the kernels' argument: PlainArgs, or ScaledArgs (PlainArgs and the two exponent arrays)
//   WIDE_OF(args)           the PlainArgs inside the argument
//   WIDE_SCALING_OF(args)   the policy's data inside the argument (cmx_plain.h: NoScaling, Exponents)
//   WIDE_*_KERNEL           the four entry points' names
// Text included into the kernel, not a function the kernel calls (cmx_plain_kernels.inc has why).  No include guard.
// What each kernel computes, the layout and the exponents' rule: the opening comment of cmx_map_wide.hip.

__global__ __launch_bounds__(kTileWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void WIDE_INSIDE_KERNEL(const WIDE_ARGS args, const WideOps o) {
  constexpr int S = WIDE_S, kRegs = S / 4;
  using X = ScalingOf<WIDE_ARGS>;
  const PlainArgs& a = WIDE_OF(args);
  const X& sc = WIDE_SCALING_OF(args);
  WideLane w;
  if (!wide_lane<S>(a, w)) return;
  const int c = blockIdx.y;
  const size_t ch = a.chunk;
  const cmx_cint first_child = (cmx_cint)a.first_child, next_sib = (cmx_cint)a.next_sib, taxon_of = (cmx_cint)a.taxon_of;
  const double* opP = o.P + (size_t)c * a.B * wide_op_doubles(S);
  const size_t lane_at = wide_op_offset(w.lane & 15, w.hi, S);
  int32_t* ec = nullptr;   // eD of (class, node 0, this lane's site)
  if constexpr (X::on) ec = inside_exponents(sc) + (size_t)c * a.nn * ch + w.j;
  for (int n = 0; n < a.nn; ++n) {
    double d[kRegs];
    unsigned code = 0;
    bool resolved = false;
    int e = 0;
    if (first_child[n] < 0) {
      resolved = wide_leaf_codes(a, w, taxon_of[n], code);
      if constexpr (S > 32) {   // padded states, no mask table: every code >= Sreal is an unknown
#pragma unroll
        for (int i = 0; i < kRegs; ++i) {
          const unsigned x = 4 * i + w.hi;
          d[i] = code < (unsigned)a.Sreal ? (double)(x == code) : (double)(x < (unsigned)a.Sreal);
        }
      } else {                  // the caller's ambiguity table, rows clamped as the plain inside kernel does
        const unsigned row = code < (unsigned)(S + max_ambig(S)) ? code : (unsigned)(S + max_ambig(S) - 1);
        const uint32_t m = code < (unsigned)S ? (1u << (code & 31)) : (a.masks ? a.masks[row] : (1u << (S & 31)) - 1u);
#pragma unroll
        for (int i = 0; i < kRegs; ++i) d[i] = (double)((m >> (4 * i + w.hi)) & 1u);
      }
    } else {
#pragma unroll
      for (int i = 0; i < kRegs; ++i) d[i] = 1.0;
      for (int k = first_child[n]; k >= 0; k = next_sib[k]) {
        wide_times(a.M, wide_at<S>(a, w, k), ch, w.live, d);
        if constexpr (X::on) {
          e += wide_exponent(ec, (size_t)k * ch, w.live);
          wide_rescale(d, e);
        }
      }
    }
    wide_store(a.D, wide_at<S>(a, w, n), ch, w.live, d);
    if constexpr (X::on) wide_exponent_store(ec, (size_t)n * ch, w.live, e);
    if (n != a.root) {
      double m[kRegs];
      if (resolved) wide_column<S>(opP + (size_t)n * wide_op_doubles(S), code, w.hi, m);
      else wide_product<S>(opP + (size_t)n * wide_op_doubles(S) + lane_at, d, m);
      wide_store(a.M, wide_at<S>(a, w, n), ch, w.live, m);
    }
  }
}

// part: [C][B*K][chunk] class c's sum_x U_b(x) ((P o N^k)_{c,b} D_b)(x), as stored: times 2^(eU + eD) of (c, b) under Exponents
__global__ __launch_bounds__(kTileWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void WIDE_OUTSIDE_KERNEL(const WIDE_ARGS args, const WideOps o, double* __restrict__ part) {
  constexpr int S = WIDE_S, kRegs = S / 4;
  using X = ScalingOf<WIDE_ARGS>;
  const PlainArgs& a = WIDE_OF(args);
  const X& sc = WIDE_SCALING_OF(args);
  WideLane w;
  if (!wide_lane<S>(a, w)) return;
  const int c = blockIdx.y;
  const size_t ch = a.chunk;
  const cmx_cint first_child = (cmx_cint)a.first_child, next_sib = (cmx_cint)a.next_sib, taxon_of = (cmx_cint)a.taxon_of;
  const size_t lane_at = wide_op_offset(w.lane & 15, w.hi, S);
  const double* opPT = o.PT + (size_t)c * a.B * wide_op_doubles(S) + lane_at;
  const double* opPN = o.PN + (size_t)c * a.B * a.K * wide_op_doubles(S);
  double* partc = part + (size_t)c * a.B * a.K * ch + w.j;
  const int32_t* edc = nullptr;
  int32_t* euc = nullptr;
  if constexpr (X::on) {
    edc = inside_exponents(sc) + (size_t)c * a.nn * ch + w.j;
    euc = outside_exponents(sc) + (size_t)c * a.nn * ch + w.j;
    wide_exponent_store(euc, (size_t)a.root * ch, w.live, 0);
  }
  for (int f = a.nn - 1; f >= 0; --f) {
    if (first_child[f] < 0) continue;
    double upf[kRegs];
    int ef = 0;
    if (f == a.root) {
#pragma unroll
      for (int i = 0; i < kRegs; ++i) upf[i] = a.pi[4 * i + w.hi];
    } else {
      wide_load(a.Up, wide_at<S>(a, w, f), ch, w.live, 1.0, upf);
      if constexpr (X::on) ef = wide_exponent(euc, (size_t)f * ch, w.live);
    }
    for (int n = first_child[f]; n >= 0; n = next_sib[n]) {
      double u[kRegs];
      int e = ef;
#pragma unroll
      for (int i = 0; i < kRegs; ++i) u[i] = upf[i];
      for (int m = first_child[f]; m >= 0; m = next_sib[m])
        if (m != n) {
          wide_times(a.M, wide_at<S>(a, w, m), ch, w.live, u);
          if constexpr (X::on) {
            e += wide_exponent(edc, (size_t)m * ch, w.live);
            wide_rescale(u, e);
          }
        }
      if constexpr (X::on) wide_exponent_store(euc, (size_t)n * ch, w.live, e);
      if (first_child[n] >= 0) {
        double up[kRegs];
        wide_product<S>(opPT + (size_t)n * wide_op_doubles(S), u, up);
        wide_store(a.Up, wide_at<S>(a, w, n), ch, w.live, up);
      }
      double d[kRegs];
      unsigned code = 0;
      const bool resolved = first_child[n] < 0 && wide_leaf_codes(a, w, taxon_of[n], code);
      if (!resolved) wide_load(a.D, wide_at<S>(a, w, n), ch, w.live, 1.0, d);
      for (int k = 0; k < a.K; ++k) {
        double t[kRegs];
        if (resolved) wide_column<S>(opPN + ((size_t)n * a.K + k) * wide_op_doubles(S), code, w.hi, t);
        else wide_product<S>(opPN + ((size_t)n * a.K + k) * wide_op_doubles(S) + lane_at, d, t);
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

// the site likelihood (site_likelihood, cmx_plain.h), once per site for the class sum: L to lik[chunk] and, under Exponents,
// its exponent E to the int32s behind them
__global__ __launch_bounds__(256) void WIDE_LIKELIHOOD_KERNEL(const WIDE_ARGS args, double* __restrict__ lik) {
  constexpr int S = WIDE_S;
  using X = ScalingOf<WIDE_ARGS>;
  const PlainArgs& a = WIDE_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  if constexpr (X::on) {
    const SiteL sl = site_likelihood<S>(args, j);
    lik[j] = sl.L;
    reinterpret_cast<int32_t*>(lik + a.chunk)[j] = sl.E;
  } else {
    lik[j] = site_likelihood<S>(a, j).L;
  }
}

// class terms in the order c = 0 .. C-1, each brought to the site's exponent, then the division by L (joint_kernel's
// statement); one thread per (site, branch)
__global__ __launch_bounds__(256) void WIDE_COUNTS_KERNEL(const WIDE_ARGS args, const double* __restrict__ part, const double* __restrict__ lik) {
  using X = ScalingOf<WIDE_ARGS>;
  const PlainArgs& a = WIDE_OF(args);
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nsites) return;
  const int b = blockIdx.y;
  const double L = lik[j];
  int E = 0;
  if constexpr (X::on) E = reinterpret_cast<const int32_t*>(lik + a.chunk)[j];
  for (int k = 0; k < a.K; ++k) {
    const size_t row = (size_t)b * a.K + k;
    double v = 0.0;
    for (int c = 0; c < a.C; ++c) {
      if constexpr (X::on) v += shifted(args, a.probs[c] * part[((size_t)c * a.B * a.K + row) * a.chunk + j], node_shift(args, c, b, j, E));
      else v += a.probs[c] * part[((size_t)c * a.B * a.K + row) * a.chunk + j];
    }
    a.counts[row * a.ldc + a.site0 + j] = v / L;
  }
}
