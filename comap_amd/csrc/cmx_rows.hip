// From pair statistics to output rows (CoMap/CoETools.cpp:650-724, 786-828): the null as a lookup table, the p-values read
// from it, the filtered pair rows in the reference's (i, j) order.  The only one of the stage files that uses rocPRIM.
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "cmx_device.h"
#include "cmx_lanes.h"

namespace cmx {

// ------------------------------------------------------------------------------------------------ p-values
__global__ void max_reduce_kernel(const double* __restrict__ x, size_t n, double* out) {
  __shared__ double sm[256];
  double v = -__builtin_inf();
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) v = x[i] > v ? x[i] : v;
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = sm[threadIdx.x + s] > sm[threadIdx.x] ? sm[threadIdx.x + s] : sm[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sm[0];
}

hipError_t launch_max_reduce(const double* d_x, size_t n, double* d_out, hipStream_t stream) {
  hipLaunchKernelGGL(max_reduce_kernel, dim3(1), dim3(256), 0, stream, d_x, n, d_out);
  return hipGetLastError();
}

// Domain(0, maxnorm, n)::getIndex (CoMap/Domain.cpp:46-59, 113-122) with the reference's operation order and no
// fused multiply-add, so that class indices are bit-exact.  -1 == OutOfRangeException.
__device__ __forceinline__ int domain_index(double maxi, int n, double x) {
  const double mini = 0.0;
  const double w = __ddiv_rn(__dsub_rn(maxi, mini), (double)n);
  if (x < mini || x >= __dadd_rn(mini, __dmul_rn((double)n, w))) return -1;
  for (int i = 1; i < n + 1; ++i)
    if (x < __dadd_rn(mini, __dmul_rn((double)i, w))) return i - 1;
  return -1;
}

__global__ void null_classify_kernel(const double* __restrict__ stat, const double* __restrict__ nmin, size_t nnull,
                                     const double* __restrict__ maxnorm, int nclasses, uint32_t* __restrict__ cls,
                                     uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[65];
  for (int i = threadIdx.x; i <= nclasses; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nnull; q += (size_t)gridDim.x * blockDim.x) {
    const int c = (stat[q] != stat[q]) ? -1 : domain_index(*maxnorm, nclasses, nmin[q]);
    const uint32_t cc = c < 0 ? (uint32_t)nclasses : (uint32_t)c;
    cls[q] = cc;
    atomicAdd(&lh[cc], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= nclasses; i += blockDim.x)
    if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

hipError_t launch_null_classify(const double* d_stat, const double* d_nmin, size_t nnull, const double* d_maxnorm,
                                int nclasses, uint32_t* d_cls, uint32_t* d_hist, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * (nclasses + 1), stream);
  if (e != hipSuccess) return e;
  if (nnull == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((nnull + 255) / 256, 1024);
  hipLaunchKernelGGL(null_classify_kernel, dim3(blocks), dim3(256), 0, stream, d_stat, d_nmin, nnull, d_maxnorm,
                     nclasses, d_cls, d_hist);
  return hipGetLastError();
}

// stable LSD: sort by statistic, then by class -> classes contiguous, each ascending (CoETools.cpp:650-652)
hipError_t sort_null_by_class(void* d_tmp, size_t& tmp_bytes, double* d_stat_in, double* d_stat_tmp, uint32_t* d_cls_in,
                              uint32_t* d_cls_tmp, size_t n, hipStream_t stream) {
  size_t b1 = tmp_bytes, b2 = tmp_bytes;   // d_tmp == nullptr: each call only reports the temporary it needs
  hipError_t e = rocprim::radix_sort_pairs(d_tmp, b1, d_stat_in, d_stat_tmp, d_cls_in, d_cls_tmp, n, 0, 64, stream);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(d_tmp, b2, d_cls_tmp, d_cls_in, d_stat_tmp, d_stat_in, n, 0, 8, stream);
  if (d_tmp == nullptr) tmp_bytes = b1 > b2 ? b1 : b2;
  return e;
}

// p = (nsim - #{null < stat} + 1) / (nsim + 1), strict '<' (CoETools.cpp:712-717); the reference scans linearly,
// the sorted class makes it a lower bound.  The bin of the statistic (equal-width bins in its value, one per eight sorted
// values of the class) bounds the search to the handful of values inside that bin: two loads for the bin and about four
// for the search, where a binary search over a class of 10^6 values sends twenty divergent loads per pair through the
// vector cache.  null_bin is monotone in v, in the table's construction and here alike, so the count is the same.
__device__ __forceinline__ uint32_t null_bin(double v, const NullClass& c) {
  const double x = (v - c.lo) * c.scale;
  if (!(x > 0.0)) return 0u;             // below the first bin, or not a number
  return x >= (double)(c.nb - 1) ? c.nb - 1 : (uint32_t)x;
}
// the null values of the pair's norm class that are < st (CoETools.cpp:712-717) and the class's size; false: the smaller
// norm lies outside the Domain (NA, CoETools.cpp:718-720)
__device__ __forceinline__ bool null_below(const NullTable& nt, double ni, double nj, double st, uint32_t* below, uint32_t* ns) {
  const double mn = ni < nj ? ni : nj;
  const int cat = domain_index(*nt.maxnorm, nt.nclasses, mn);
  if (cat < 0) return false;
  const NullClass c = nt.cls[cat];
  uint32_t l2 = c.off, h2 = c.off + c.ns;
  if (c.nb > 1) {
    const uint32_t* bs = nt.bins + c.boff + null_bin(st, c);
    l2 = bs[0];
    h2 = bs[1];
  }
  while (l2 < h2) {
    const uint32_t mid = (l2 + h2) >> 1;
    if (nt.sorted[mid] < st) l2 = mid + 1; else h2 = mid;
  }
  *below = l2 - c.off;
  *ns = c.ns;
  return true;
}
__device__ __forceinline__ void null_pvalue(const NullTable& nt, double ni, double nj, double st, double* pvalue, int32_t* nsim) {
  uint32_t below, ns;
  if (!null_below(nt, ni, nj, st, &below, &ns)) { *pvalue = __builtin_nan(""); *nsim = 0; return; }
  *pvalue = (double)(ns - below + 1) / (double)(ns + 1);
  *nsim = (int32_t)ns;
}
__global__ void pvalue_kernel(const double* __restrict__ stat, size_t ldo, const double* __restrict__ norms, size_t n, const NullTable nt,
                              double* __restrict__ pvalue, int32_t* __restrict__ nsim, size_t irow0) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = irow0 + blockIdx.y;          // row of the full matrix; the arrays hold rows irow0 ..
  if (j >= n) return;
  const size_t o = (size_t)blockIdx.y * ldo + j;
  if (j <= i) { pvalue[o] = __builtin_nan(""); nsim[o] = 0; return; }
  null_pvalue(nt, norms[i], norms[j], stat[o], pvalue + o, nsim + o);
}

hipError_t launch_pvalues(const double* d_stat, size_t ldo, const double* d_norms, size_t n, const NullTable& nt, double* d_pvalue,
                          int32_t* d_nsim, size_t irow0, size_t nrows, hipStream_t stream) {
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)nrows);
  hipLaunchKernelGGL(pvalue_kernel, grid, dim3(256), 0, stream, d_stat, ldo, d_norms, n, nt, d_pvalue, d_nsim, irow0);
  return hipGetLastError();
}

// class offsets and bin ranges: the bins span the class's values between its 1/64 and 63/64 quantiles (the tails fall
// into the first and last bin), so that a few extreme values do not stretch them
__global__ void null_classes_kernel(const double* __restrict__ sorted, const uint32_t* __restrict__ hist, int nclasses,
                                    NullClass* __restrict__ cls) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t o = 0;
  for (int k = 0; k < nclasses; ++k) {
    NullClass c;
    c.off = o; c.ns = hist[k]; c.nb = 1; c.boff = (o >> kNullBinShift) + 2 * (uint32_t)k; c.lo = 0.0; c.scale = 0.0;
    if (c.ns >= 64) {
      const double qlo = sorted[o + (c.ns >> 6)], qhi = sorted[o + c.ns - 1 - (c.ns >> 6)];
      const uint32_t nb = c.ns >> kNullBinShift;
      const double scale = (double)nb / (qhi - qlo);
      if (qhi > qlo && scale > 0.0 && scale < 1.0e300 && qlo > -1.0e300) { c.nb = nb; c.lo = qlo; c.scale = scale; }
    }
    cls[k] = c;
    o += c.ns;
  }
}
// bins[b] = first position of the class whose value's bin is >= b, for b = 0 .. nb (bins[nb] = the class's end): one
// thread per bin searches the class (a thread per sorted value filling the bins up to its own is cheaper on a smooth
// null and serial on one with gaps)
__global__ void null_bins_kernel(const double* __restrict__ sorted, const NullClass* __restrict__ cls, uint32_t* __restrict__ bins) {
  const NullClass c = cls[blockIdx.y];
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (c.nb <= 1 || b > c.nb) return;
  uint32_t lo = c.off, hi = c.off + c.ns;
  if (b == 0) hi = lo;
  if (b == c.nb) lo = hi;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (null_bin(sorted[mid], c) < b) lo = mid + 1; else hi = mid;
  }
  bins[c.boff + b] = lo;
}
hipError_t launch_null_index(const double* d_sorted, const uint32_t* d_hist, int nclasses, size_t nnull, NullClass* d_cls,
                             uint32_t* d_bins, hipStream_t stream) {
  hipLaunchKernelGGL(null_classes_kernel, dim3(1), dim3(64), 0, stream, d_sorted, d_hist, nclasses, d_cls);
  if (nnull)   // (the classes' sizes live on the device: the grid covers the largest number of bins any class can have)
    hipLaunchKernelGGL(null_bins_kernel, dim3((unsigned)((nnull >> kNullBinShift) / 256 + 1), (unsigned)nclasses), dim3(256), 0, stream,
                       d_sorted, d_cls, d_bins);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ compacted pair rows
// CoETools.cpp:672-724 as two passes of kPairRowSegs waves per row i: count the pairs (i, j > i) that pass the filters,
// exclusive scan of the counts (rocPRIM), then write the rows at their final position -- the reference's (i, j) order.
__device__ __forceinline__ bool pair_passes(const cmx_pair_filters& f, int ci, double ri, int cj, double rj, double st) {
  if (cj < f.min_rate_class || rj < f.min_rate) return false;
  if (f.max_rate_class_diff >= 0 && abs(cj - ci) > f.max_rate_class_diff) return false;
  if (f.max_rate_diff >= 0.0 && fabs(rj - ri) > f.max_rate_diff) return false;
  return !(fabs(st) < f.min_statistic);
}
static_assert(sizeof(cmx_pair_row) == 48 && offsetof(cmx_pair_row, stat) == 8 && offsetof(cmx_pair_row, rc_min) == 16 &&
                  offsetof(cmx_pair_row, nsim) == 20 && offsetof(cmx_pair_row, pr_min) == 24 &&
                  offsetof(cmx_pair_row, n_min) == 32 && offsetof(cmx_pair_row, pvalue) == 40,
              "pair_rows_kernel packs a row as three 16-byte words");
template <bool WRITE>
__global__ __launch_bounds__(64) void pair_rows_kernel(const double* __restrict__ stat, size_t ldo,
                                                       const double* __restrict__ pvalue, const int32_t* __restrict__ nsim,
                                                       size_t n, const int32_t* __restrict__ rc, const double* __restrict__ pr,
                                                       const double* __restrict__ norm, cmx_pair_filters f,
                                                       unsigned long long* __restrict__ rowcount /* counts, then offsets */,
                                                       cmx_pair_row* __restrict__ rows, size_t capacity, size_t irow0,
                                                       const unsigned long long* __restrict__ base, const NullTable nt) {
  // stat / pvalue / nsim hold rows irow0 .. of the full matrix (local row = blockIdx.x / kPairRowSegs); rows are appended
  // after *base.  A row's columns i + 1 .. n - 1 are cut into kPairRowSegs runs of whole 64-column steps, one wave each
  // (one wave per row leaves a 1677-row block of the 25000-site job at 6 waves per CU, all waiting on their loads); the
  // counting pass counts per run, so the runs of a row, and the rows, still land in (i, j) order.
  const size_t il = blockIdx.x / kPairRowSegs, i = irow0 + il;
  const int lane = threadIdx.x;
  const int ci = rc[i];
  const double ri = pr[i];
  const size_t seg = ((n - i - 1 + kPairRowSegs - 1) / kPairRowSegs + 63) / 64 * 64;
  const size_t jb = i + 1 + (blockIdx.x % kPairRowSegs) * seg, je = jb + seg < n ? jb + seg : n;
  unsigned long long run = WRITE ? rowcount[blockIdx.x] + (base ? *base : 0ull) : 0ull;
  const bool row_ok = !(ci < f.min_rate_class || ri < f.min_rate);
  // the passing pairs of one 64-column step are packed in LDS and leave as one contiguous run of 16-byte stores (a
  // 48-byte row per lane is a 48-byte-strided store otherwise); a rows buffer that is not 16-byte aligned gets the rows
  // one per lane
  __shared__ cmx_i4 stage[WRITE ? 64 * 3 : 1];
  const bool packed = ((uintptr_t)rows & 15) == 0;
  if (row_ok)
    for (size_t j0 = jb; j0 < je; j0 += 64) {
      const size_t j = j0 + lane;
      bool ok = false;
      double st = 0.0;
      if (j < je) {
        st = stat[il * ldo + j];
        ok = pair_passes(f, ci, ri, rc[j], pr[j], st);
      }
      const unsigned long long m = __ballot(ok);
      if (WRITE && m && run < capacity) {
        const int slot = __popcll(m & ((1ull << lane) - 1ull));
        if (ok) {
          cmx_pair_row r;
          r.i = (int32_t)i; r.j = (int32_t)j; r.stat = st;
          r.rc_min = ci < rc[j] ? ci : rc[j];
          r.pr_min = ri < pr[j] ? ri : pr[j];
          r.n_min = norm[i] < norm[j] ? norm[i] : norm[j];
          r.pvalue = pvalue ? pvalue[il * ldo + j] : __builtin_nan("");
          r.nsim = nsim ? nsim[il * ldo + j] : 0;
          if (nt.sorted) null_pvalue(nt, norm[i], norm[j], st, &r.pvalue, &r.nsim);   // only for the pairs that are written
          if (packed) {
            const long long s8 = __double_as_longlong(r.stat), p8 = __double_as_longlong(r.pr_min),
                            n8 = __double_as_longlong(r.n_min), v8 = __double_as_longlong(r.pvalue);
            stage[3 * slot + 0] = cmx_i4{r.i, r.j, (int)s8, (int)(s8 >> 32)};
            stage[3 * slot + 1] = cmx_i4{r.rc_min, r.nsim, (int)p8, (int)(p8 >> 32)};
            stage[3 * slot + 2] = cmx_i4{(int)n8, (int)(n8 >> 32), (int)v8, (int)(v8 >> 32)};
          } else if (run + slot < capacity) {
            rows[run + slot] = r;
          }
        }
        if (packed) {
          const unsigned long long room = capacity - run, cnt = (unsigned long long)__popcll(m);
          const int nq = 3 * (int)(cnt < room ? cnt : room);
          cmx_i4* dst = reinterpret_cast<cmx_i4*>(rows + run);
#pragma unroll
          for (int q = lane; q < 192; q += 64)
            if (q < nq) dst[q] = stage[q];
        }
      }
      run += __popcll(m);
    }
  if (!WRITE && lane == 0) rowcount[blockIdx.x] = run;
}

__global__ void pair_rows_total_kernel(const unsigned long long* __restrict__ offsets, const unsigned long long* __restrict__ last_count,
                                       size_t n, unsigned long long* __restrict__ total, const unsigned long long* __restrict__ base) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *total = (base ? *base : 0ull) + offsets[n - 1] + *last_count;
}

// What launch_pair_rows and launch_inter_rows share, over nruns runs (d_rowcount: nruns + 1 words): count per run, exclusive
// scan of the counts (rocPRIM), write the rows at their final position, total.  d_tmp == nullptr: the scan's temporary size.
template <class CountPass, class WritePass>
static hipError_t two_pass_rows(size_t nruns, unsigned long long* d_rowcount, void* d_tmp, size_t& tmp_bytes, unsigned long long* d_count,
                                const unsigned long long* d_base, hipStream_t stream, CountPass count_pass, WritePass write_pass) {
  if (d_tmp == nullptr)
    return rocprim::exclusive_scan(nullptr, tmp_bytes, d_rowcount, d_rowcount, 0ull, nruns, rocprim::plus<unsigned long long>(), stream);
  count_pass();
  // keep the last run's count (the scan overwrites it) to form the total
  hipError_t e = hipMemcpyAsync(d_rowcount + nruns, d_rowcount + nruns - 1, sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(d_tmp, tmp_bytes, d_rowcount, d_rowcount, 0ull, nruns, rocprim::plus<unsigned long long>(), stream);
  if (e != hipSuccess) return e;
  write_pass();
  // (after the writes: d_count may be the very word d_base points to)
  hipLaunchKernelGGL(pair_rows_total_kernel, dim3(1), dim3(64), 0, stream, d_rowcount, d_rowcount + nruns, nruns, d_count, d_base);
  return hipGetLastError();
}

// nrows rows irow0 .. irow0 + nrows - 1 of an n-column matrix.  d_base (device, may be null): number of rows already in
// d_rows -- this block's rows are appended behind them and *d_count becomes the new total, so that consecutive row blocks
// fill one array in the reference's (i, j) order.
hipError_t launch_pair_rows(const double* d_stat, size_t ldo, const double* d_pvalue, const int32_t* d_nsim, size_t n, const SiteCols& s,
                            const cmx_pair_filters& f, RowScan& scan, cmx_pair_row* d_rows, size_t capacity, unsigned long long* d_count,
                            size_t irow0, size_t nrows, const unsigned long long* d_base, const NullTable* d_inline_null,
                            hipStream_t stream) {
  // d_inline_null: the write pass looks the p-values up itself (no dense p-value / Nsim block, no pvalue_kernel)
  const NullTable nt = d_inline_null ? *d_inline_null : NullTable{nullptr, nullptr, nullptr, nullptr, 0};
  const size_t nruns = nrows * kPairRowSegs;
  auto pass = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)nruns), dim3(64), 0, stream, d_stat, ldo, d_pvalue, d_nsim, n, s.rc, s.pr, s.nm, f,
                       scan.rowcount, d_rows, capacity, irow0, d_base, nt);
  };
  return two_pass_rows(nruns, scan.rowcount, scan.tmp, scan.tmp_bytes, d_count, d_base, stream, [&] { pass(pair_rows_kernel<false>); },
                       [&] { pass(pair_rows_kernel<true>); });
}

// ---- compact pair records (round 4): the unfiltered pair loop of CoETools.cpp:672-724 as 16 bytes per pair -- the statistic,
// the number of null values below it and the size of its null class -- at the pair's position in (i, j) order.  Without
// filters that position is arithmetic (no counting pass, no scan), and everything else a statistics.txt row holds (i, j,
// RCmin, PRmin, Nmin, the p-value's quotient) is a function of per-site arrays the host already has:
// cmx_expand_compact_rows rebuilds the 48-byte rows bit for bit.  A third of the bytes cross PCIe.
static_assert(sizeof(cmx_pair_compact) == 16, "one 16-byte store per pair");
__global__ void pair_compact_kernel(const double* __restrict__ stat, size_t ldo, size_t n, const double* __restrict__ norm, const NullTable nt,
                                    cmx_pair_compact* __restrict__ out, size_t capacity, size_t irow0, size_t row_begin) {
  const size_t i = irow0 + blockIdx.y, j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j <= i || j >= n) return;
  // pairs of the rows [row_begin, i) come first
  const size_t at = (i - row_begin) * (n - 1) - (i * (i - 1) - row_begin * (row_begin - 1)) / 2 + (j - i - 1);
  if (at >= capacity) return;
  cmx_pair_compact r;
  r.stat = stat[(size_t)blockIdx.y * ldo + j];
  r.below = 0xffffffffu;   // NA (or no null given): PValue NaN, Nsim 0
  r.nsim = 0;
  if (nt.sorted) {
    uint32_t below, ns;
    if (null_below(nt, norm[i], norm[j], r.stat, &below, &ns)) { r.below = below; r.nsim = ns; }
  }
  out[at] = r;
}
hipError_t launch_pair_compact(const double* d_stat, size_t ldo, size_t n, const double* d_norm, const NullTable* nt, cmx_pair_compact* d_out,
                               size_t capacity, hipStream_t stream, size_t irow0, size_t nrows, size_t row_begin) {
  const NullTable t = nt ? *nt : NullTable{nullptr, nullptr, nullptr, nullptr, 0};
  hipLaunchKernelGGL(pair_compact_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)nrows), dim3(256), 0, stream, d_stat, ldo, n, d_norm, t,
                     d_out, capacity, irow0, row_begin);
  return hipGetLastError();
}

// ---- rows of the inter-gene statistics file: CoETools::computeInterStats' pair loop (CoMap/CoETools.cpp:786-828) on the
// device, the same two passes as pair_rows_kernel.  Row i of data set 1 against columns [0, n2) of data set 2, or against
// column i alone (independant_comparisons, :796-797).  Filters: min rate class / rate per data set, max differences per
// pair, |stat| >= statistic.min.  Nmin = min(norm1[i], norm2[j]); with f.reference_norm_quirk the reference's own column,
// min(norms1[i], norms2[i]) (:803 reads norms2[i]; beyond the second data set's end the index is clamped where the
// reference reads out of bounds).
__device__ __forceinline__ bool inter_passes(const cmx_inter_filters& f, int ci, double ri, int cj, double rj, double st) {
  if (cj < f.min_rate_class2 || rj < f.min_rate2) return false;
  if (f.max_rate_class_diff >= 0 && abs(cj - ci) > f.max_rate_class_diff) return false;
  if (f.max_rate_diff >= 0.0 && fabs(rj - ri) > f.max_rate_diff) return false;
  return !(fabs(st) < f.min_statistic);
}
template <bool WRITE>
__global__ __launch_bounds__(64) void inter_rows_kernel(const double* __restrict__ stat, size_t ldo, size_t n2,
                                                        const int32_t* __restrict__ rc1, const double* __restrict__ pr1,
                                                        const double* __restrict__ nm1, const int32_t* __restrict__ rc2,
                                                        const double* __restrict__ pr2, const double* __restrict__ nm2,
                                                        cmx_inter_filters f, unsigned long long* __restrict__ rowcount,
                                                        cmx_pair_row* __restrict__ rows, size_t capacity, size_t irow0,
                                                        const unsigned long long* __restrict__ base) {
  const size_t il = blockIdx.x, i = irow0 + il;
  const int lane = threadIdx.x;
  const int ci = rc1[i];
  const double ri = pr1[i];
  unsigned long long run = WRITE ? rowcount[il] + (base ? *base : 0ull) : 0ull;
  const bool diag = f.independent_comparisons != 0;
  const size_t jb = diag ? i : 0, je = diag ? i + 1 : n2;
  if (!(ci < f.min_rate_class1 || ri < f.min_rate1))
    for (size_t j0 = jb; j0 < je; j0 += 64) {
      const size_t j = j0 + lane;
      bool ok = false;
      double st = 0.0;
      if (j < je) {
        st = diag ? stat[il] : stat[il * ldo + j];
        ok = inter_passes(f, ci, ri, rc2[j], pr2[j], st);
      }
      const unsigned long long m = __ballot(ok);
      if (WRITE && ok) {
        const unsigned long long pos = run + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < capacity) {
          cmx_pair_row r;
          r.i = (int32_t)i; r.j = (int32_t)j; r.stat = st;
          r.rc_min = ci < rc2[j] ? ci : rc2[j];
          r.pr_min = ri < pr2[j] ? ri : pr2[j];
          const double nj = nm2[f.reference_norm_quirk ? (i < n2 ? i : n2 - 1) : j];
          r.n_min = nm1[i] < nj ? nm1[i] : nj;
          r.pvalue = __builtin_nan("");
          r.nsim = 0;
          rows[pos] = r;
        }
      }
      run += __popcll(m);
    }
  if (!WRITE && lane == 0) rowcount[il] = run;
}

// rows irow0 .. irow0 + nrows - 1 of data set 1; d_stat: [nrows][ldo] (or [nrows] for independant comparisons); d_base
// / d_count as in launch_pair_rows
hipError_t launch_inter_rows(const double* d_stat, size_t ldo, size_t n2, const SiteCols& s1, const SiteCols& s2, const cmx_inter_filters& f,
                             RowScan& scan, cmx_pair_row* d_rows, size_t capacity, unsigned long long* d_count, size_t irow0, size_t nrows,
                             const unsigned long long* d_base, hipStream_t stream) {
  auto pass = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)nrows), dim3(64), 0, stream, d_stat, ldo, n2, s1.rc, s1.pr, s1.nm, s2.rc, s2.pr, s2.nm, f,
                       scan.rowcount, d_rows, capacity, irow0, d_base);
  };
  return two_pass_rows(nrows, scan.rowcount, scan.tmp, scan.tmp_bytes, d_count, d_base, stream, [&] { pass(inter_rows_kernel<false>); },
                       [&] { pass(inter_rows_kernel<true>); });
}

}  // namespace cmx
