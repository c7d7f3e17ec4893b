// Sliding-window conditional p-values (the "exact procedure" of `test`, R/CoMapFunctions.R:168-215): for a pair
// (s, m) count the null entries with Nmin in (m - ws, m + ws), and among them those with a statistic >= s.  An orthogonal range
// count per pair: the null is kept as a wavelet matrix over the entries in Nmin order, whose symbols are the entries' ranks in
// statistic order.  A query is three binary searches and two rank queries per level, O(log nnull) whatever the window holds;
// every count is an integer.
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "cmx_device.h"

namespace cmx {

// ------------------------------------------------------------------------------------------------ build
// doubles as radix keys: ascending keys = ascending values (-0 before +0, which compare equal: any order of the two serves the
// searches below); all ones is no finite value, no infinity: the key of a dropped entry, behind every kept one
__device__ __forceinline__ uint64_t window_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double window_unkey(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}
constexpr uint64_t kWindowDropped = ~0ull;

__global__ void window_nmin_keys_kernel(const double* __restrict__ stat, const double* __restrict__ nmin, size_t n, uint64_t* __restrict__ key,
                                        uint32_t* __restrict__ idx, WindowHead* __restrict__ head) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (e < n) {
    const double s = stat[e], m = nmin[e];
    keep = s == s && m == m;
    key[e] = keep ? window_key(m) : kWindowDropped;
    idx[e] = (uint32_t)e;
  }
  const unsigned long long kept = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&head->nkept, (uint32_t)__popcll(kept));
}

// position p of the Nmin order holds entry perm[p]: its Nmin, and the key of its statistic
__global__ void window_stat_keys_kernel(const double* __restrict__ stat, const double* __restrict__ nmin, const uint32_t* __restrict__ perm, size_t n,
                                        double* __restrict__ sorted_nmin, uint64_t* __restrict__ key, uint32_t* __restrict__ pos) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double s = stat[perm[p]], m = nmin[perm[p]];
  sorted_nmin[p] = m;
  key[p] = s == s && m == m ? window_key(s) : kWindowDropped;
  pos[p] = (uint32_t)p;
}

// ws <- (max(sim[, rateName]) - min(sim[, rateName])) * window / 2 (CoMapFunctions.R:172), one operation at a time
__global__ void window_head_kernel(const double* __restrict__ sorted_nmin, double window, WindowHead* __restrict__ head) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t nk = head->nkept;
  head->pad = 0;
  if (nk == 0) { head->ws = 0.0; head->nmin_min = head->nmin_max = __builtin_nan(""); return; }
  const double lo = sorted_nmin[0], hi = sorted_nmin[nk - 1];
  head->nmin_min = lo;
  head->nmin_max = hi;
  head->ws = __ddiv_rn(__dmul_rn(__dsub_rn(hi, lo), window), 2.0);
}

// rank r of the statistic order sits at position pos[r] of the Nmin order: the sequence the levels are cut from
__global__ void window_ranks_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ pos, size_t n, double* __restrict__ sorted_stat,
                                    uint32_t* __restrict__ seq) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  sorted_stat[r] = window_unkey(key[r]);
  seq[pos[r]] = (uint32_t)r;
}

// one level: bit `bit` of every symbol, 32 to a unit, and each unit's number of ones (units beyond the sequence are empty)
__global__ void window_level_bits_kernel(const uint32_t* __restrict__ seq, size_t n, int bit, size_t units, uint2* __restrict__ level,
                                         uint32_t* __restrict__ cnt) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool one = e < n && ((seq[e] >> bit) & 1u);
  const unsigned long long m = __ballot(one);
  const size_t u = e >> 5;
  if ((threadIdx.x & 31) == 0 && u < units) {
    const uint32_t w = (uint32_t)(m >> (threadIdx.x & 32));
    level[u].y = w;
    cnt[u] = (uint32_t)__popc(w);
  }
}
__global__ void window_level_ones_kernel(const uint32_t* __restrict__ ones, size_t n, size_t units, uint2* __restrict__ level,
                                         uint32_t* __restrict__ zeros) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  level[u].x = ones[u];
  if (u == units - 1) *zeros = (uint32_t)n - ones[u];   // (the last unit is empty: the ones before it are all of them)
}

static unsigned window_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_window_build(const double* d_null_stat, const double* d_null_nmin, size_t n, double window, WindowBuild& b, double* d_nmin,
                               double* d_stat, uint2* d_levels, uint32_t* d_zeros, WindowHead* d_head, hipStream_t stream) {
  const int L = window_levels(n);
  const size_t units = window_units(n);
  hipError_t e = hipSuccess;
  if (b.tmp == nullptr) {   // the largest temporary of the rocPRIM calls below
    size_t t1 = 0, t2 = 0, t3 = 0;
    e = rocprim::radix_sort_pairs(nullptr, t1, b.key_a, b.key_b, b.val_a, b.val_b, n, 0, 64, stream);
    if (e == hipSuccess) e = rocprim::radix_sort_keys(nullptr, t2, b.seq_a, b.seq_b, n, 0, 1, stream);
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, t3, b.cnt, b.ones, 0u, units, rocprim::plus<uint32_t>(), stream);
    b.tmp_bytes = std::max(t1, std::max(t2, t3));
    return e;
  }
  e = hipMemsetAsync(d_head, 0, sizeof(WindowHead), stream);
  if (e != hipSuccess) return e;
  const unsigned nb = window_blocks(n);
  size_t tb = b.tmp_bytes;
  // entries by Nmin (stable: equal values keep the caller's order), then their ranks by statistic
  hipLaunchKernelGGL(window_nmin_keys_kernel, dim3(nb), dim3(256), 0, stream, d_null_stat, d_null_nmin, n, b.key_a, b.val_a, d_head);
  e = rocprim::radix_sort_pairs(b.tmp, tb, b.key_a, b.key_b, b.val_a, b.val_b, n, 0, 64, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(window_stat_keys_kernel, dim3(nb), dim3(256), 0, stream, d_null_stat, d_null_nmin, b.val_b, n, d_nmin, b.key_a, b.val_a);
  hipLaunchKernelGGL(window_head_kernel, dim3(1), dim3(64), 0, stream, d_nmin, window, d_head);
  tb = b.tmp_bytes;
  e = rocprim::radix_sort_pairs(b.tmp, tb, b.key_a, b.key_b, b.val_a, b.val_b, n, 0, 64, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(window_ranks_kernel, dim3(nb), dim3(256), 0, stream, b.key_b, b.val_b, n, d_stat, b.seq_a);
  // the levels, highest bit first; after each the sequence is partitioned by that bit, zeros first, stably
  uint32_t *cur = b.seq_a, *nxt = b.seq_b;
  for (int l = 0; l < L; ++l) {
    const int bit = L - 1 - l;
    uint2* level = d_levels + (size_t)l * units;
    hipLaunchKernelGGL(window_level_bits_kernel, dim3(window_blocks(units * 32)), dim3(256), 0, stream, cur, n, bit, units, level, b.cnt);
    tb = b.tmp_bytes;
    e = rocprim::exclusive_scan(b.tmp, tb, b.cnt, b.ones, 0u, units, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(window_level_ones_kernel, dim3(window_blocks(units)), dim3(256), 0, stream, b.ones, n, units, level, d_zeros + l);
    if (l + 1 < L) {
      tb = b.tmp_bytes;
      e = rocprim::radix_sort_keys(b.tmp, tb, cur, nxt, n, bit, bit + 1, stream);
      if (e != hipSuccess) return e;
      std::swap(cur, nxt);
    }
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ queries
__device__ __forceinline__ uint32_t window_count_lt(const double* __restrict__ v, uint32_t n, double x) {   // #{v < x}
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t window_count_le(const double* __restrict__ v, uint32_t n, double x) {   // #{v <= x}
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the positions [lo, hi) of the kept entries with nmin > m - ws and nmin < m + ws (CoMapFunctions.R:182); hi <= lo: none
__device__ __forceinline__ void window_bounds(const WindowIndex& ix, double m, uint32_t* lo, uint32_t* hi) {
  *lo = *hi = 0;
  if (m != m) return;
  const uint32_t nk = ix.head->nkept;
  const double ws = ix.head->ws;
  *lo = window_count_le(ix.nmin, nk, m - ws);
  *hi = window_count_lt(ix.nmin, nk, m + ws);
  if (*hi < *lo) *hi = *lo;
}
__device__ __forceinline__ uint32_t window_ones_before(const uint2* __restrict__ level, uint32_t pos) {
  const uint2 u = level[pos >> 5];
  return u.x + (uint32_t)__popc(u.y & ((1u << (pos & 31)) - 1u));
}
// the entries at [lo, hi) whose rank is < r, r < n
__device__ __forceinline__ uint32_t window_ranks_below(const WindowIndex& ix, uint32_t lo, uint32_t hi, uint32_t r) {
  uint32_t below = 0;
  for (int l = 0; l < ix.L && lo < hi; ++l) {
    const uint2* level = ix.levels + (size_t)l * ix.units;
    const uint32_t lo1 = window_ones_before(level, lo), hi1 = window_ones_before(level, hi);
    if ((r >> (ix.L - 1 - l)) & 1u) {
      below += (hi - hi1) - (lo - lo1);
      const uint32_t z = ix.zeros[l];
      lo = z + lo1;
      hi = z + hi1;
    } else {
      lo -= lo1;
      hi -= hi1;
    }
  }
  return below;
}
// sum(d[, statName] >= stat), with lower <= stat (CoMapFunctions.R:201, 206), among the entries at [lo, hi); s is no NaN
__device__ __forceinline__ uint32_t window_count(const WindowIndex& ix, uint32_t lo, uint32_t hi, double s, bool lower) {
  if (hi <= lo) return 0;
  const uint32_t nk = ix.head->nkept;
  const uint32_t r = lower ? window_count_le(ix.stat, nk, s) : window_count_lt(ix.stat, nk, s);
  const uint32_t below = r >= nk ? hi - lo : window_ranks_below(ix, lo, hi, r);   // (every position below nk holds a rank below nk)
  return lower ? below : hi - lo - below;
}

__global__ void window_test_kernel(const WindowIndex ix, const double* __restrict__ stat, const double* __restrict__ nmin, size_t nq,
                                   const cmx_window_params p, double* __restrict__ pvalue, uint32_t* __restrict__ count, uint32_t* __restrict__ nobs) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const double s = stat[q], m = nmin[q];
  uint32_t lo, hi;
  window_bounds(ix, m, &lo, &hi);
  const uint32_t no = hi - lo, c = s == s ? window_count(ix, lo, hi, s, p.lower != 0) : 0u;
  if (count) count[q] = c;
  if (nobs) nobs[q] = no;
  if (pvalue) {
    double pv = __builtin_nan("");
    if (m < p.conserved_nmin) pv = 1.0;   // the threshold for conserved sites comes first (CoMapFunctions.R:183-187)
    else if (m == m && no >= p.min_nobs && s == s) pv = (double)(c + 1u) / (double)(no + 1u);
    pvalue[q] = pv;
  }
}

hipError_t launch_window_test(const WindowIndex& ix, const double* d_stat, const double* d_nmin, size_t nq, const cmx_window_params& p,
                              double* d_pvalue, uint32_t* d_count, uint32_t* d_nobs, hipStream_t stream) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(window_test_kernel, dim3(window_blocks(nq)), dim3(256), 0, stream, ix, d_stat, d_nmin, nq, p, d_pvalue, d_count, d_nobs);
  return hipGetLastError();
}

__global__ void window_site_bounds_kernel(const WindowIndex ix, const double* __restrict__ norm, size_t n, uint32_t* __restrict__ lo,
                                          uint32_t* __restrict__ hi) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t l, h;
  window_bounds(ix, norm[i], &l, &h);
  lo[i] = l;
  hi[i] = h;
}
hipError_t launch_window_site_bounds(const WindowIndex& ix, const double* d_norm, size_t n, uint32_t* d_lo, uint32_t* d_hi, hipStream_t stream) {
  hipLaunchKernelGGL(window_site_bounds_kernel, dim3(window_blocks(n)), dim3(256), 0, stream, ix, d_norm, n, d_lo, d_hi);
  return hipGetLastError();
}

// pair_compact_kernel's grid and positions; the window of a pair is that of the site with the smaller norm (Nmin as
// pair_rows_kernel writes it: norm_i < norm_j ? norm_i : norm_j)
static_assert(sizeof(cmx_pair_window) == 16, "one 16-byte store per pair");
__global__ void pair_window_kernel(const double* __restrict__ stat, size_t ldo, size_t n, const double* __restrict__ norm, const WindowIndex ix,
                                   const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, int lower, cmx_pair_window* __restrict__ out,
                                   size_t capacity, size_t irow0, size_t row_begin) {
  const size_t i = irow0 + blockIdx.y, j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j <= i || j >= n) return;
  const size_t at = (i - row_begin) * (n - 1) - (i * (i - 1) - row_begin * (row_begin - 1)) / 2 + (j - i - 1);
  if (at >= capacity) return;
  const size_t k = norm[i] < norm[j] ? i : j;
  const uint32_t l = lo[k], h = hi[k];
  cmx_pair_window r;
  r.stat = stat[(size_t)blockIdx.y * ldo + j];
  r.nobs = h - l;
  r.count = r.stat == r.stat ? window_count(ix, l, h, r.stat, lower != 0) : 0xffffffffu;
  out[at] = r;
}
hipError_t launch_pair_window(const double* d_stat, size_t ldo, size_t n, const double* d_norm, const WindowIndex& ix, const uint32_t* d_lo,
                              const uint32_t* d_hi, int lower, cmx_pair_window* d_out, size_t capacity, hipStream_t stream, size_t irow0,
                              size_t nrows, size_t row_begin) {
  hipLaunchKernelGGL(pair_window_kernel, dim3(window_blocks(n), (unsigned)nrows), dim3(256), 0, stream, d_stat, ldo, n, d_norm, ix, d_lo, d_hi, lower,
                     d_out, capacity, irow0, row_begin);
  return hipGetLastError();
}

}  // namespace cmx
