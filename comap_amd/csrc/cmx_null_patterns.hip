// The fused null's distinct columns.  A third of the sites the target's null maps repeat a column mapped
// earlier in the same launch (Gamma with alpha = 0.5: the slowest class's columns are mostly constant), and a column's
// counts, norm, posterior rate and rate class depend on the column alone.  So a pass of the null:
//   null_pattern_key_kernel   one thread per simulated site g: 64-bit hash of its column + a site-major byte copy
//   radix sort of (hash, g)   stable: in a run of equal hashes the smallest g comes first
//   null_pattern_flag_kernel  a sorted element starts a run when its hash or its column bytes differ from its predecessor's
//                             (a hash collision costs deduplication, never correctness)
//   two scans                 run head of every sorted element (max); number of run heads up to g (sum, over g)
//   null_pattern_assign_kernel  pattern of every site, first site of every pattern: patterns numbered in first-occurrence
//                             order, so a mapping wave's 64 patterns stay on nearby columns (the symbol reads coalesce)
// then map_kernel<S, kModeNullPatterns> maps each pattern once, its wave writing the counts of its 16 NG patterns as one tile
// of the table ([B*K][row] doubles, the block the class-sum epilogue fills), and null_pattern_pairs_kernel scores the pairs
// from the tiles with the null mode's own pair_stat_strided and minima (Correlation / Covariance: null_pattern_moments_kernel
// once per pattern, then pair_stat_moments, one pass per pair).
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "cmx_device.h"
#include "cmx_pairstat.h"

namespace cmx {

namespace {

constexpr int kPatThreads = 256;

__device__ __forceinline__ uint64_t pat_mix(uint64_t h, uint64_t x) {
  h ^= x * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  return h * 0xBF58476D1CE4E5B9ull;
}

__device__ __forceinline__ uint64_t pat_final(uint64_t h) {   // MurmurHash3's fmix64
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

__global__ __launch_bounds__(kPatThreads) void null_pattern_key_kernel(const uint8_t* __restrict__ sup, int T, size_t rep_ram, size_t n,
                                                                       int rowb, int hash_bits, uint64_t* __restrict__ key,
                                                                       uint32_t* __restrict__ gidx, uint8_t* __restrict__ col) {
  const size_t g = (size_t)blockIdx.x * kPatThreads + threadIdx.x;
  if (g >= n) return;
  const size_t rh = g / rep_ram, j = g - rh * rep_ram;
  const uint8_t* src = sup + rh * (size_t)T * rep_ram + j;   // taxon t at src[t * rep_ram]: a wave reads 64 neighbouring bytes
  uint4* dst = reinterpret_cast<uint4*>(col + g * (size_t)rowb);
  uint64_t h = 0x243F6A8885A308D3ull ^ (uint64_t)T;
  for (int t0 = 0; t0 < rowb; t0 += 16) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int t = t0 + u;
      const uint32_t b = t < T ? (uint32_t)src[(size_t)t * rep_ram] : 0u;
      w[u >> 2] |= b << (8 * (u & 3));
    }
    dst[t0 >> 4] = make_uint4(w[0], w[1], w[2], w[3]);
    h = pat_mix(h, (uint64_t)w[0] | ((uint64_t)w[1] << 32));
    h = pat_mix(h, (uint64_t)w[2] | ((uint64_t)w[3] << 32));
  }
  h = pat_final(h);
  if (hash_bits < 64) h &= (1ull << hash_bits) - 1;
  key[g] = h;
  gidx[g] = (uint32_t)g;
}

// the same keys, indices and packed columns, four neighbouring sites per thread: a taxon's four symbols are one 32-bit load
// (a wave reads 256 contiguous bytes per taxon instead of 64) and the columns are transposed in registers.  Needs
// rep_ram % 4 == 0 and a 4-byte aligned alignment buffer: a thread's sites then lie in one replicate and batch.
__global__ __launch_bounds__(kPatThreads) void null_pattern_key4_kernel(const uint8_t* __restrict__ sup, int T, size_t rep_ram, size_t n,
                                                                        int rowb, int hash_bits, uint64_t* __restrict__ key,
                                                                        uint32_t* __restrict__ gidx, uint8_t* __restrict__ col) {
  const size_t g = ((size_t)blockIdx.x * kPatThreads + threadIdx.x) * 4;
  if (g >= n) return;
  const size_t rh = g / rep_ram, j = g - rh * rep_ram, ld4 = rep_ram / 4;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(sup + rh * (size_t)T * rep_ram + j);   // taxon t at src[t * ld4]
  uint64_t h[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) h[s] = 0x243F6A8885A308D3ull ^ (uint64_t)T;
  for (int t0 = 0; t0 < rowb; t0 += 16) {
    uint32_t v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = t0 + u < T ? src[(size_t)(t0 + u) * ld4] : 0u;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int u = 0; u < 16; ++u) w[u >> 2] |= ((v[u] >> (8 * s)) & 0xffu) << (8 * (u & 3));
      reinterpret_cast<uint4*>(col + (g + s) * (size_t)rowb)[t0 >> 4] = make_uint4(w[0], w[1], w[2], w[3]);
      h[s] = pat_mix(h[s], (uint64_t)w[0] | ((uint64_t)w[1] << 32));
      h[s] = pat_mix(h[s], (uint64_t)w[2] | ((uint64_t)w[3] << 32));
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    uint64_t f = pat_final(h[s]);
    if (hash_bits < 64) f &= (1ull << hash_bits) - 1;
    key[g + s] = f;
    gidx[g + s] = (uint32_t)(g + s);
  }
}

__global__ __launch_bounds__(kPatThreads) void null_pattern_flag_kernel(size_t n, const uint64_t* __restrict__ key_s,
                                                                        const uint32_t* __restrict__ g_s, const uint8_t* __restrict__ col,
                                                                        int rowb, uint32_t* __restrict__ head, uint32_t* __restrict__ first) {
  const size_t i = (size_t)blockIdx.x * kPatThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = g_s[i];
  bool starts = i == 0;
  if (!starts) {
    starts = key_s[i] != key_s[i - 1];
    if (!starts) {   // equal hashes: the columns themselves decide, byte for byte
      const uint4* x = reinterpret_cast<const uint4*>(col + (size_t)g * rowb);
      const uint4* y = reinterpret_cast<const uint4*>(col + (size_t)g_s[i - 1] * rowb);
      for (int c = 0; c < rowb / 16; ++c) {
        const uint4 a = x[c], b = y[c];
        if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) { starts = true; break; }
      }
    }
  }
  head[i] = starts ? (uint32_t)i : 0u;
  first[g] = starts ? 1u : 0u;
}

__global__ __launch_bounds__(kPatThreads) void null_pattern_assign_kernel(size_t n, const uint32_t* __restrict__ g_s,
                                                                          const uint32_t* __restrict__ head, const uint32_t* __restrict__ incl,
                                                                          uint32_t* __restrict__ pat_of, uint32_t* __restrict__ rep_site,
                                                                          unsigned long long* __restrict__ total) {
  const size_t i = (size_t)blockIdx.x * kPatThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = g_s[i], hi = head[i];
  const uint32_t p = incl[g_s[hi]] - 1u;
  pat_of[g] = p;
  if (hi == (uint32_t)i) rep_site[p] = g;
  if (i == n - 1) *total += incl[n - 1];   // (stream order: the previous pass's add is done)
}

// Correlation / Covariance: what pair_stat_strided's first pass and two of its second-pass sums give for one operand, once per
// pattern.  Lane = pattern: the lanes of a wave read neighbouring doubles of a tile's rows.  (In the mapping kernel's epilogue
// the same loop cost 5.3 ms and six spilled registers)
// Up to kMomentRows branches the column is held in registers, so every count is fetched once; the sums are pattern_moments'.
constexpr int kMomentRows = 128;
__global__ __launch_bounds__(kPatThreads) void null_pattern_moments_kernel(int B, int K, const double* __restrict__ counts, uint32_t tile_sites,
                                                                           uint32_t tile_row, const uint32_t* __restrict__ npat,
                                                                           double* __restrict__ pat_mean, double* __restrict__ pat_ss) {
  const size_t p = (size_t)blockIdx.x * kPatThreads + threadIdx.x;
  if (p >= *npat) return;
  const double* c = counts + (p / tile_sites) * ((size_t)B * K * tile_row) + p % tile_sites;
  double m = 0, ss = 0;
  if (B <= kMomentRows) {
    const size_t ld = (size_t)K * tile_row;
    double x[kMomentRows];
#pragma unroll
    for (int b = 0; b < kMomentRows; ++b) x[b] = c[(size_t)(b < B ? b : 0) * ld];
#pragma unroll
    for (int b = 0; b < kMomentRows; ++b)
      if (b < B) m += x[b];
    m /= B;
#pragma unroll
    for (int b = 0; b < kMomentRows; ++b)
      if (b < B) {
        const double dx = x[b] - m;
        ss = __builtin_fma(dx, dx, ss);
      }
  } else {
    pattern_moments(B, K, c, (size_t)tile_row, m, ss);
  }
  pat_mean[p] = m;
  pat_ss[p] = ss;
}

// pair q = (rep, j): sites g0 = 2 rep rep_ram + j (batch 0) and g1 = g0 + rep_ram (batch 1); the minima take batch 0 first,
// then "<", as map_kernel's null mode does (AnalysisTools.cpp:643-652)
__global__ __launch_bounds__(kPatThreads) void null_pattern_pairs_kernel(int kind, double param, int B, int K, const double* __restrict__ counts,
                                                                         uint32_t tile_sites, uint32_t tile_row,
                                                                         const double* __restrict__ pat_mean, const double* __restrict__ pat_ss,
                                                                         const double* __restrict__ post_rate,
                                                                         const int32_t* __restrict__ rate_class, const double* __restrict__ norm,
                                                                         const uint32_t* __restrict__ pat_of, size_t rep_ram, size_t npairs,
                                                                         const double* __restrict__ mean, double* __restrict__ stat,
                                                                         int32_t* __restrict__ rcmin, double* __restrict__ prmin,
                                                                         double* __restrict__ nmin) {
  const size_t q = (size_t)blockIdx.x * kPatThreads + threadIdx.x;
  if (q >= npairs) return;
  const size_t r = q / rep_ram, j = q - r * rep_ram, g0 = 2 * r * rep_ram + j;
  const uint32_t pa = pat_of[g0], pb = pat_of[g0 + rep_ram];
  // pattern p: column p % tile_sites of tile p / tile_sites, row stride tile_row -- the operands map_kernel's null mode
  // gives pair_stat_strided from its two count blocks
  const size_t tile = (size_t)B * K * tile_row;
  const double* ca = counts + (pa / tile_sites) * tile + pa % tile_sites;
  const double* cb = counts + (pb / tile_sites) * tile + pb % tile_sites;
  if (pat_mean)   // Correlation / Covariance: every count is read once
    stat[q] = pair_stat_moments(kind, B, K, ca, (size_t)tile_row, pat_mean[pa], pat_ss[pa], cb, (size_t)tile_row, pat_mean[pb], pat_ss[pb]);
  else
    stat[q] = pair_stat_strided(kind, param, B, K, ca, (size_t)tile_row, cb, (size_t)tile_row, mean);
  if (rcmin) {
    const int32_t a = rate_class[pa], b = rate_class[pb];
    rcmin[q] = b < a ? b : a;
  }
  if (prmin) {
    const double a = post_rate[pa], b = post_rate[pb];
    prmin[q] = b < a ? b : a;
  }
  if (nmin) {
    const double a = norm[pa], b = norm[pb];
    nmin[q] = b < a ? b : a;
  }
}

inline unsigned pat_grid(size_t n) { return (unsigned)((n + kPatThreads - 1) / kPatThreads); }

}  // namespace

size_t null_pattern_row_bytes(int T) { return ((size_t)T + 15) / 16 * 16; }

hipError_t null_pattern_tmp_bytes(size_t n, int hash_bits, size_t* bytes) {
  size_t a = 0, b = 0, c = 0;
  const int bits = hash_bits < 1 || hash_bits > 64 ? 64 : hash_bits;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                           n, 0, bits, (hipStream_t)0);
  if (e != hipSuccess) return e;
  e = rocprim::inclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, n, rocprim::maximum<uint32_t>(), (hipStream_t)0);
  if (e != hipSuccess) return e;
  e = rocprim::inclusive_scan(nullptr, c, (uint32_t*)nullptr, (uint32_t*)nullptr, n, rocprim::plus<uint32_t>(), (hipStream_t)0);
  *bytes = std::max(a, std::max(b, c));
  return e;
}

hipError_t launch_null_patterns(const uint8_t* d_sup, int T, size_t rep_ram, size_t n, int hash_bits, const NullPatternBufs& b,
                                hipStream_t stream) {
  const int rowb = (int)null_pattern_row_bytes(T);
  const int bits = hash_bits < 1 || hash_bits > 64 ? 64 : hash_bits;
  if (rep_ram % 4 == 0 && reinterpret_cast<uintptr_t>(d_sup) % 4 == 0)
    hipLaunchKernelGGL(null_pattern_key4_kernel, dim3(pat_grid(n / 4)), dim3(kPatThreads), 0, stream, d_sup, T, rep_ram, n, rowb, bits,
                       b.key, b.g, b.col);
  else
    hipLaunchKernelGGL(null_pattern_key_kernel, dim3(pat_grid(n)), dim3(kPatThreads), 0, stream, d_sup, T, rep_ram, n, rowb, bits, b.key,
                       b.g, b.col);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t tb = b.tmp_bytes;
  if ((e = rocprim::radix_sort_pairs(b.tmp, tb, b.key, b.key_s, b.g, b.g_s, n, 0, bits, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(null_pattern_flag_kernel, dim3(pat_grid(n)), dim3(kPatThreads), 0, stream, n, b.key_s, b.g_s, b.col, rowb, b.head,
                     b.incl);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = b.tmp_bytes;
  if ((e = rocprim::inclusive_scan(b.tmp, tb, b.head, b.head, n, rocprim::maximum<uint32_t>(), stream)) != hipSuccess) return e;
  tb = b.tmp_bytes;
  if ((e = rocprim::inclusive_scan(b.tmp, tb, b.incl, b.incl, n, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(null_pattern_assign_kernel, dim3(pat_grid(n)), dim3(kPatThreads), 0, stream, n, b.g_s, b.head, b.incl, b.pat_of,
                     b.rep_site, b.total);
  return hipGetLastError();
}

hipError_t launch_null_pattern_moments(int B, int K, const double* counts, int tile_sites, int tile_row, const uint32_t* npat,
                                       size_t cap, double* pat_mean, double* pat_ss, hipStream_t stream) {
  if (tile_sites < 1 || tile_row < tile_sites || !npat || !pat_mean || !pat_ss) return hipErrorInvalidValue;
  hipLaunchKernelGGL(null_pattern_moments_kernel, dim3(pat_grid(cap)), dim3(kPatThreads), 0, stream, B, K, counts, (uint32_t)tile_sites,
                     (uint32_t)tile_row, npat, pat_mean, pat_ss);
  return hipGetLastError();
}

hipError_t launch_null_pattern_pairs(const Stat& st, const double* counts, int tile_sites, int tile_row, const double* pat_mean,
                                     const double* pat_ss, const SiteCols& pat, const uint32_t* pat_of, size_t rep_ram, size_t npairs,
                                     const PairOut& out, hipStream_t stream) {
  if (tile_sites < 1 || tile_row < tile_sites || (pat_mean != nullptr) != (pat_ss != nullptr)) return hipErrorInvalidValue;
  if (pat_mean && st.kind != CMX_STAT_CORRELATION && st.kind != CMX_STAT_COVARIANCE) return hipErrorInvalidValue;
  hipLaunchKernelGGL(null_pattern_pairs_kernel, dim3(pat_grid(npairs)), dim3(kPatThreads), 0, stream, st.kind, st.param, st.B, st.K, counts,
                     (uint32_t)tile_sites, (uint32_t)tile_row, pat_mean, pat_ss, pat.pr, pat.rc, pat.nm, pat_of, rep_ram, npairs,
                     st.d_mean, out.stat, out.rcmin, out.prmin, out.nmin);
  return hipGetLastError();
}

}  // namespace cmx
