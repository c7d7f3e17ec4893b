// Probe of v_mfma_f64_16x16x4_f64 on gfx950 for the mapping walk's 20x20 products.
// (a) lane maps: A = one-hot in lane la, B = one-hot in lane lb, for all 64 x 64 pairs: the product must appear exactly
//     where  A lane = (row la & 15, k la >> 4),  B lane = (k lb >> 4, col lb & 15),  D (lane, reg) = (col lane & 15,
//     row (lane >> 4) + 4 reg)  say, and nowhere else.
// (b) one 20x20 product of a packed operator (cmx_layout.h) with a 64-site vector in the walk's layout, forward and
//     transposed, two ways: 25 tile steps of v_mfma_f64_4x4x4_4b per site group in the walk's order, and five chained
//     16x16x4 (states 0..15) plus five 4x4x4_4b (states 16..19) per site group with the same order of input tiles.
//     The 20 x 64 results are compared as bytes, and against a host sum in long double for sanity.
// hipcc --offload-arch=gfx950 -O2 -Icomap_amd/csrc scripts/probe_mfma_f64_16x16x4.hip -o build/probe_mfma16 && build/probe_mfma16
// Exit status 0: maps confirmed and all bytes equal.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cmx_layout.h"

typedef double d4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

__global__ void onehot_kernel(double* d /* [64 * 64][64 lanes][4] */) {
  const int l = threadIdx.x, la = blockIdx.x >> 6, lb = blockIdx.x & 63;
  const d4 r = __builtin_amdgcn_mfma_f64_16x16x4f64(l == la ? 2.0 : 0.0, l == lb ? 3.0 : 0.0, (d4){0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
  for (int q = 0; q < 4; ++q) d[((size_t)blockIdx.x * 64 + l) * 4 + q] = r[q];
}

constexpr int S = 20, NB = 5, NG = 4;
// x, y: [sb][g][lane]: state 4 sb + (lane >> 4) of site 16 g + (lane & 15).  One block of 64 lanes per (transposed, trial).
template <bool TR>
__device__ void product_both(const double* mat, const double* x, double* y4, double* y16) {
  const int l = threadIdx.x;
  const uint8_t* buf = reinterpret_cast<const uint8_t*>(mat);
  double xv[NB][NG], a[NB][NG];
  for (int sb = 0; sb < NB; ++sb)
    for (int g = 0; g < NG; ++g) xv[sb][g] = x[(sb * NG + g) * 64 + l];
  // the walk's 25 tile steps: step q = output tile q / NB, input tile q % NB, stored tile (o, i) or (i, o)
  const uint8_t* tile0 = buf + cmx::mfma_a_tile_offset(l, TR);
  for (int o = 0; o < NB; ++o)
    for (int i = 0; i < NB; ++i) {
      const double m = *reinterpret_cast<const double*>(tile0 + (TR ? i * NB + o : o * NB + i) * 128);
      for (int g = 0; g < NG; ++g) a[o][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(m, xv[i][g], i == 0 ? 0.0 : a[o][g], 0, 0, 0);
    }
  for (int sb = 0; sb < NB; ++sb)
    for (int g = 0; g < NG; ++g) y4[(sb * NG + g) * 64 + l] = a[sb][g];
  // mixed: states 0..15 of a site group are the four results of a chain of five 16x16x4, states 16..19 five 4x4x4_4b
  d4 acc[NG];
  double t4[NG];
  for (int i = 0; i < NB; ++i) {
    const double m16 = *reinterpret_cast<const double*>(buf + cmx::mfma16_a_offset(l, i, TR, S));
    const double m4 = *reinterpret_cast<const double*>(tile0 + (TR ? i * NB + 4 : 4 * NB + i) * 128);
    for (int g = 0; g < NG; ++g) {
      acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(m16, xv[i][g], i == 0 ? (d4){0.0, 0.0, 0.0, 0.0} : acc[g], 0, 0, 0);
      t4[g] = __builtin_amdgcn_mfma_f64_4x4x4f64(m4, xv[i][g], i == 0 ? 0.0 : t4[g], 0, 0, 0);
    }
  }
  for (int g = 0; g < NG; ++g) {
    for (int sb = 0; sb < 4; ++sb) y16[(sb * NG + g) * 64 + l] = acc[g][sb];
    y16[(4 * NG + g) * 64 + l] = t4[g];
  }
}
__global__ void product_kernel(const double* mat, const double* x, double* y4, double* y16) {
  const size_t t = blockIdx.x >> 1, n = (size_t)S * 64;
  if (blockIdx.x & 1) product_both<true>(mat + t * S * S, x + t * n, y4 + blockIdx.x * n, y16 + blockIdx.x * n);
  else product_both<false>(mat + t * S * S, x + t * n, y4 + blockIdx.x * n, y16 + blockIdx.x * n);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd01() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}
// mixed sign, magnitudes over 2^-span .. 2^span
static double rnd_mixed(int span) { return (rnd01() < 0.5 ? -1.0 : 1.0) * std::ldexp(1.0 + rnd01(), (int)(rnd01() * (2 * span + 1)) - span); }

int main() {
  int bad = 0;
  {  // (a)
    const size_t n = (size_t)64 * 64 * 64 * 4;
    double* d;
    CK(hipMalloc(&d, n * 8));
    hipLaunchKernelGGL(onehot_kernel, dim3(64 * 64), dim3(64), 0, 0, d);
    CK(hipDeviceSynchronize());
    std::vector<double> h(n);
    CK(hipMemcpy(h.data(), d, n * 8, hipMemcpyDeviceToHost));
    size_t wrong = 0, hits = 0;
    for (int la = 0; la < 64; ++la)
      for (int lb = 0; lb < 64; ++lb) {
        const int row = la & 15, col = lb & 15;
        const bool meet = (la >> 4) == (lb >> 4);
        for (int l = 0; l < 64; ++l)
          for (int q = 0; q < 4; ++q) {
            const bool here = meet && (l & 15) == col && (l >> 4) + 4 * q == row;
            const double v = h[(((size_t)la * 64 + lb) * 64 + l) * 4 + q];
            if (v != (here ? 6.0 : 0.0)) {
              if (wrong++ < 8) printf("  A lane %d, B lane %d: D lane %d reg %d = %g, expected %g\n", la, lb, l, q, v, here ? 6.0 : 0.0);
            }
            hits += v != 0.0;
          }
      }
    printf("(a) lane maps A (row l&15, k l>>4), B (k l>>4, col l&15), D (col l&15, row (l>>4) + 4 reg): %zu products seen, "
           "%zu of %zu values off\n", hits, wrong, n);
    bad |= wrong != 0 || hits != 64 * 16;
    CK(hipFree(d));
  }
  {  // (b)
    constexpr int T = 64;   // trials; the odd ones carry wide magnitudes
    const size_t nm = (size_t)T * S * S, nx = (size_t)T * S * 64, ny = 2 * nx;
    std::vector<double> M(nm), P(nm), X(nx), Y4(ny), Y16(ny);
    for (int t = 0; t < T; ++t) {
      const int span = (t & 1) ? 40 : 3;
      for (int k = 0; k < S * S; ++k) M[(size_t)t * S * S + k] = rnd_mixed(span);
      for (int k = 0; k < S * 64; ++k) X[(size_t)t * S * 64 + k] = rnd_mixed(span);
      for (int tl = 0; tl < NB * NB; ++tl)   // pack_blocks
        for (int k = 0; k < 16; ++k) P[(size_t)t * S * S + tl * 16 + k] = M[(size_t)t * S * S + (4 * (tl / NB) + k / 4) * S + 4 * (tl % NB) + k % 4];
    }
    double *dm, *dx, *d4p, *d16p;
    CK(hipMalloc(&dm, nm * 8)); CK(hipMalloc(&dx, nx * 8)); CK(hipMalloc(&d4p, ny * 8)); CK(hipMalloc(&d16p, ny * 8));
    CK(hipMemcpy(dm, P.data(), nm * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dx, X.data(), nx * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d4p, 0xff, ny * 8)); CK(hipMemset(d16p, 0x7f, ny * 8));
    hipLaunchKernelGGL(product_kernel, dim3(2 * T), dim3(64), 0, 0, dm, dx, d4p, d16p);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(Y4.data(), d4p, ny * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(Y16.data(), d16p, ny * 8, hipMemcpyDeviceToHost));
    for (int tr = 0; tr < 2; ++tr) {
      size_t diff = 0, diff_hi = 0, total = 0;
      double worst = 0.0;
      for (int t = 0; t < T; ++t) {
        const double *m = &M[(size_t)t * S * S], *x = &X[(size_t)t * S * 64];
        const size_t base = ((size_t)2 * t + tr) * S * 64;
        for (int sb = 0; sb < NB; ++sb)
          for (int g = 0; g < NG; ++g)
            for (int l = 0; l < 64; ++l, ++total) {
              const size_t at = base + (sb * NG + g) * 64 + l;
              if (std::memcmp(&Y4[at], &Y16[at], 8) != 0) {
                ++diff;
                diff_hi += sb == 4;
                if (diff <= 4) printf("  trial %d state %d site %d: %.17g (4x4x4_4b) vs %.17g (mixed)\n", t, 4 * sb + (l >> 4), 16 * g + (l & 15), Y4[at], Y16[at]);
              }
              const int st = 4 * sb + (l >> 4), site = 16 * g + (l & 15);
              long double ref = 0.0L, mag = 0.0L;
              for (int z = 0; z < S; ++z) {
                const long double p = (long double)(tr ? m[z * S + st] : m[st * S + z]) * x[((z / 4) * NG + g) * 64 + 16 * (z % 4) + (site & 15)];
                ref += p; mag += fabsl(p);
              }
              const double e = (double)(fabsl((long double)Y16[at] - ref) / mag);
              if (e > worst) worst = e;
            }
      }
      printf("(b) %s product, %d trials: %zu of %zu results differ as bytes (%zu of them in states 16..19); "
             "mixed form against a long double sum: worst |err| / sum |terms| = %.3g\n", tr ? "transposed" : "forward", T, diff, total, diff_hi, worst);
      bad |= diff != 0 || !(worst < 20 * 2.3e-16);
    }
  }
  printf(bad ? "PROBE FAILED\n" : "probe ok: maps confirmed, both forms give the same bytes\n");
  return bad ? 1 : 0;
}
