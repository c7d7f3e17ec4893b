// pair_gram_kernel (fp64 throughout): all-pairs statistic as X.X^T on v_mfma_f64_16x16x4_f64 with per-statistic epilogues
//   (CoMap/Statistics.h:164-329; loops CoMap/CoETools.cpp:672-692, 786-810).
#include <algorithm>

#include "cmx_device.h"
#include "cmx_pairstat.h"

namespace cmx {

typedef double d4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ pair statistics
// prep: X[b][i] (Bp rows, zero padded) and per-site scalars s (sum of squares) and r (row sum of indicators)
//   Correlation / Covariance: X = type-0 count - mean;  Cosinus: X = type-0 count;  Compensation: X = per-branch total;
//   Cosubstitution: X = [total >= 1];  DiscreteMI: X = [total >= threshold], r = sum X, s = NaN flag when a total leaves [0, 10000)
// w (normalised branch weights, or null; Correlation, Compensation, Cosinus, Covariance, EuclidianDistance only):
// X_b = weight_factor(kind, w_b) * (the value above), the mean of Correlation / Covariance is sum w x; the launcher then
// scores Correlation with the Cosinus epilogue and Covariance with the scalar product's (no (B-1) factors: DESIGN A.7, weighted)
__global__ void pair_prep_kernel(int kind, double param, const double* __restrict__ counts, size_t n, size_t ldc, int B,
                                 int K, double* __restrict__ X, size_t ldx, int Bp, double* __restrict__ sv,
                                 double* __restrict__ rv, const double* __restrict__ mvec /* [B] or null */, size_t blk,
                                 const double* __restrict__ w) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // blk > 0: the sites are `blk`-site blocks side by side (replicates of the clustering null); every block gets its own
  // [Bp][ldx] operand so that a block's rows stay ldx * 8 bytes apart (not the whole batch's row length: 128 rows
  // 4 MB apart thrash the TLB and land on one L2 channel)
  if (blk) X += (i / blk) * ((size_t)Bp * ldx) - (i / blk) * blk;
  if (w) {
    const bool centred = kind == CMX_STAT_CORRELATION || kind == CMX_STAT_COVARIANCE;
    double mean = 0.0;
    if (centred)
      for (int b = 0; b < B; ++b) mean += w[b] * (counts[(size_t)b * K * ldc + i] - (mvec ? mvec[b] : 0.0));
    double s = 0.0, r = 0.0;
    for (int b = 0; b < B; ++b) {
      double v;
      if (centred) v = counts[(size_t)b * K * ldc + i] - (mvec ? mvec[b] : 0.0) - mean;
      else if (kind == CMX_STAT_COSINUS) v = counts[(size_t)b * K * ldc + i];
      else {
        v = 0.0;
        for (int k = 0; k < K; ++k) v += counts[((size_t)b * K + k) * ldc + i];
      }
      v *= weight_factor(kind, w[b]);
      X[(size_t)b * ldx + i] = v;
      s += v * v;
      r += v;
    }
    for (int b = B; b < Bp; ++b) X[(size_t)b * ldx + i] = 0.0;
    sv[i] = s;
    rv[i] = r;
    return;
  }
  double mean = 0.0;
  if (kind == CMX_STAT_CORRELATION || kind == CMX_STAT_COVARIANCE) {   // (CorrectedCorrelation arrives as Correlation with its mean vector in mvec)
    for (int b = 0; b < B; ++b) mean += counts[(size_t)b * K * ldc + i] - (mvec ? mvec[b] : 0.0);
    mean /= B;
  }
  double s = 0.0, r = 0.0;
  bool bad = false;
  for (int b = 0; b < B; ++b) {
    double v;
    if (kind == CMX_STAT_CORRELATION || kind == CMX_STAT_COVARIANCE) v = counts[(size_t)b * K * ldc + i] - (mvec ? mvec[b] : 0.0) - mean;
    else if (kind == CMX_STAT_COSINUS || kind == CMX_STAT_SCALAR_PRODUCT) v = counts[(size_t)b * K * ldc + i];
    else {
      double t = 0.0;
      for (int k = 0; k < K; ++k) t += counts[((size_t)b * K + k) * ldc + i];
      if (kind == CMX_STAT_COMPENSATION || kind == CMX_STAT_EUCLIDIAN_DISTANCE) v = t;
      else if (kind == CMX_STAT_COSUBSTITUTION) v = t >= 1.0 ? 1.0 : 0.0;
      else {
        v = t >= param ? 1.0 : 0.0;
        if (!(t >= 0.0 && t < 10000.0)) bad = true;
      }
    }
    X[(size_t)b * ldx + i] = v;
    s += v * v;
    r += v;
  }
  for (int b = B; b < Bp; ++b) X[(size_t)b * ldx + i] = 0.0;
  sv[i] = bad ? __builtin_nan("") : s;
  rv[i] = r;
}

hipError_t launch_pair_prep(const Stat& st, const double* d_counts, size_t n, size_t ldc, const double* d_mvec, size_t blk,
                            const PairOperand& o, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(pair_prep_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, stream, st.gk, st.param,
                     d_counts, n, ldc, st.B, st.K, o.X, o.ldx, pair_Bp(st.B), o.s, o.r, d_mvec, blk, st.d_w);
  return hipGetLastError();
}

// the factor of a statistic that depends on one site only (fi, fj of pair_epilogue)
__device__ __forceinline__ double pair_site_factor(int kind, int B, double s) {
  if (kind == CMX_STAT_CORRELATION) return sqrt(s / (B - 1));
  if (kind == CMX_STAT_COSINUS || kind == CMX_STAT_COMPENSATION) return sqrt(s);
  return 0.0;
}
__device__ __forceinline__ double pair_epilogue(int kind, int B, double g, double si, double sj, double ri, double rj, double fi,
                                                double fj) {
  switch (kind) {
    case CMX_STAT_CORRELATION: {
      const double cov = g / (B - 1);
      return cov / (fi * fj);
    }
    case CMX_STAT_COVARIANCE: return g / (B - 1);
    case CMX_STAT_SCALAR_PRODUCT: return g;
    case CMX_STAT_COSINUS: return g / (fi * fj);
    case CMX_STAT_COMPENSATION: {
      double s3 = si + sj + 2.0 * g;
      if (s3 < 0.0) s3 = 0.0;
      return 1.0 - sqrt(s3) / (fi + fj);
    }
    case CMX_STAT_COSUBSTITUTION: return g;
    case CMX_STAT_DISCRETE_MI: {
      if (si != si || sj != sj) return __builtin_nan("");
      const double np = B;
      const double cell[4] = {g, ri - g, rj - g, np - ri - rj + g};
      const double ma[4] = {ri, ri, np - ri, np - ri}, mb[4] = {rj, np - rj, rj, np - rj};
      double s = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (cell[q] > 0) s += (cell[q] / np) * log(cell[q] * np / (ma[q] * mb[q]));
      return s / log(2.7182818);
    }
  }
  return __builtin_nan("");
}

// Compensation's sum (t1 + t2)^2 of one pair taken over the operand columns themselves, by a whole wave: lane = branch
// mod 64, eight of a lane's branches per trip with their loads in flight together (a branch past B adds (0 + 0)^2),
// then a butterfly sum.  Every lane returns the sum.  The value depends on the two columns only.
__device__ __forceinline__ double comp_direct_wave(int lane, int B, const double* __restrict__ c1, size_t ldx1,
                                                   const double* __restrict__ c2, size_t ldx2) {
  double s3 = 0.0;
  for (int b0 = lane; b0 < B; b0 += 8 * kWave) {
    double x[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = b0 + u * kWave;
      x[u] = c1[(size_t)(b < B ? b : 0) * ldx1];
      y[u] = c2[(size_t)(b < B ? b : 0) * ldx2];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double t = b0 + u * kWave < B ? x[u] + y[u] : 0.0;
      s3 += t * t;
    }
  }
  for (int off = 32; off; off >>= 1) s3 += __shfl_xor(s3, off);
  return s3;
}

// One wave computes a 64x64 tile of G = X1^T-rows . X2-rows on v_mfma_f64_16x16x4_f64 (A[i][k]: lane = i + 16k,
// C[row = (lane>>4) + 4r][col = lane & 15]); operands come straight from L2 (X is a few MB), prefetched one k-step
// ahead; 16 MFMAs per 8 operand loads.
// Four tiles (four waves) per workgroup: single-wave workgroups made the launch dispatch-bound (262 144 of them for a
// batch of 256 matrices of 2 000 sites ran at 0.1-0.5 resident waves per SIMD, profiles/r01_cluster_null_pmc_summary.json).
__global__ __launch_bounds__(4 * kWave) void pair_gram_kernel(int kind, int B, int Bp, const double* __restrict__ X1,
                                                         const double* __restrict__ s1, const double* __restrict__ r1,
                                                         size_t n1, size_t ldx1, const double* __restrict__ X2,
                                                         const double* __restrict__ s2, const double* __restrict__ r2,
                                                         size_t n2, size_t ldx2, int intra, double* __restrict__ out,
                                                         size_t ldo, size_t zsite, size_t zout, size_t zx, size_t irow0) {
  // blockIdx.z: independent blocks of sites (clustering null: one per replicate): per-site vectors side by side
  // (zsite apart), operands zx apart
  X1 += blockIdx.z * zx; s1 += blockIdx.z * zsite; r1 += blockIdx.z * zsite;
  X2 += blockIdx.z * zx; s2 += blockIdx.z * zsite; r2 += blockIdx.z * zsite;
  out += blockIdx.z * zout;
  const int lane = threadIdx.x & 63;
  const size_t ti = blockIdx.y, tj = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const size_t i0 = ti * 64, j0 = tj * 64;
  if (j0 >= n2) return;
  const double nanv = __builtin_nan("");
  // irow0: the rows are rows irow0 .. of the full matrix (row-block / multi-GPU processing); "below the diagonal" is
  // then j <= irow0 + i.  A tile wholly below it is skipped (kPairUpperRows: the caller never reads it) or NaN-filled.
  if (intra == kPairUpperRows && j0 + 63 < irow0 + i0) return;   // (clustering: mirrored distances; row blocks: only j > i is read)
  if (intra != kPairRectangle && irow0 == 0 && tj < ti) {  // strictly below the diagonal: NaN fill (reference loop is j > i, CoETools.cpp:680)
    for (int r = 0; r < 64; ++r) {
      const size_t i = i0 + r, j = j0 + lane;
      if (i < n1 && j < n2) out[i * ldo + j] = nanv;
    }
    return;
  }
  const int li = lane & 15, lk = lane >> 4;
  size_t ia[4], jb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    size_t i = i0 + 16 * t + li, j = j0 + 16 * t + li;
    ia[t] = i < n1 ? i : n1 - 1;
    jb[t] = j < n2 ? j : n2 - 1;
  }
  d4 acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = (d4){0.0, 0.0, 0.0, 0.0};
  double a[4], b[4], an[4], bn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    a[t] = X1[(size_t)lk * ldx1 + ia[t]];
    b[t] = X2[(size_t)lk * ldx2 + jb[t]];
  }
  for (int k0 = 0; k0 < Bp; k0 += 4) {
    const int kn = (k0 + 4 < Bp) ? k0 + 4 : k0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      an[t] = X1[(size_t)(kn + lk) * ldx1 + ia[t]];
      bn[t] = X2[(size_t)(kn + lk) * ldx2 + jb[t]];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], b[q], acc[p][q], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) { a[t] = an[t]; b[t] = bn[t]; }
  }
  // Epilogue: the per-site factors of the statistic (a square root and a division each) are computed once per row
  // and column of the tile, not once per pair -- the same operations on the same operands, so the values do not
  // change, but 64 pairs per lane no longer repeat them (they were three quarters of the kernel's instructions).
  double sjv[4], rjv[4], fj[4];
  unsigned long long redo = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const size_t j = j0 + 16 * q + li;
    sjv[q] = s2[j < n2 ? j : n2 - 1];
    rjv[q] = r2[j < n2 ? j : n2 - 1];
    fj[q] = pair_site_factor(kind, B, sjv[q]);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t i = i0 + 16 * p + lk + 4 * r;
      if (i >= n1) continue;
      const double si = s1[i], ri = r1[i];
      const double fi = pair_site_factor(kind, B, si);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t j = j0 + 16 * q + li;
        if (j < n2) {
          double v = pair_epilogue(kind, B, acc[p][q][r], si, sjv[q], ri, rjv[q], fi, fj[q]);
          // (Compensation, signed totals: pairs whose s3 = si + sj + 2g cancels are redone below; bit = this pair)
          if (kind == CMX_STAT_COMPENSATION && 2.0 * acc[p][q][r] < -0.5 * (si + sjv[q]) && !(intra != kPairRectangle && j <= irow0 + i))
            redo |= 1ull << (16 * p + 4 * r + q);
          if (intra != kPairRectangle && j <= irow0 + i) v = nanv;
          out[i * ldo + j] = v;
        }
      }
    }
  // Compensation forms sum (t1 + t2)^2 as si + sj + 2g.  With signed totals (g < 0) that cancels: near anti-parallel
  // vectors lost every digit of it (1.0 for 1 - 4.9e-10; up to 7e-12 at 10 000 sites of configuration 4, enough to
  // move the count of null values below the statistic for 0.07 % of its pairs).  Where the Gram form keeps less than half of
  // si + sj the sum is taken over the operand columns themselves (comp_direct_wave).  A pair of non-negative totals has
  // g >= 0 and never comes here.  Not in the epilogue above: a loop over b there keeps it from unrolling, and the
  // accumulators then live in scratch.  The wave takes the marked pairs one at a time -- a lane alone would walk its B
  // branches while 63 wait -- so the value depends on the pair only, not on its place in a tile, a row block or a rank.
  // (Every lane of the wave is here: the returns above are per wave.)
  for (unsigned long long live = __ballot(redo != 0); live; live &= live - 1) {
    const int src = __builtin_ctzll(live);
    for (unsigned long long m = __shfl(redo, src); m; m &= m - 1) {
      const int bit = __builtin_ctzll(m);
      const size_t i = i0 + 16 * (bit >> 4) + (src >> 4) + 4 * ((bit >> 2) & 3), j = j0 + 16 * (bit & 3) + (src & 15);   // i < n1, j < n2: marked there only
      const double s3 = comp_direct_wave(lane, B, X1 + i, ldx1, X2 + j, ldx2);
      if (lane == src) out[i * ldo + j] = 1.0 - sqrt(s3) / (pair_site_factor(kind, B, s1[i]) + pair_site_factor(kind, B, s2[j]));
    }
  }
}

constexpr int kEuclidRows = 8;
// EuclidianDistance (CoMap/Distance.h:157-171): sqrt(sum_b (tot2_b - tot1_b)^2) over the per-branch totals.  Computed from
// the differences themselves, not from the Gram matrix: ||a||^2 + ||b||^2 - 2 a.b loses all digits for near-identical
// vectors.  X = the totals operand of pair_prep_kernel (as Compensation's), [Bp][ldx]; one thread per pair, row i broadcast.
__global__ __launch_bounds__(256) void pair_euclid_kernel(int B, const double* __restrict__ X1, size_t n1, size_t ldx1,
                                                         const double* __restrict__ X2, size_t n2, size_t ldx2, int intra,
                                                         double* __restrict__ out, size_t ldo, size_t zx,
                                                         size_t zout) {
  // one wave = kEuclidRows rows x 64 columns: the column operand is loaded once per branch and used for all rows, the
  // row operands are wave-uniform (scalar loads); per pair the arithmetic is the same chain of FMAs in branch order
  X1 += blockIdx.z * zx; X2 += blockIdx.z * zx; out += blockIdx.z * zout;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t i0 = ((size_t)blockIdx.y * 4 + wave) * kEuclidRows, j = (size_t)blockIdx.x * 64 + (threadIdx.x & 63);
  if (i0 >= n1) return;
  if (intra == kPairUpperRows && (size_t)blockIdx.x * 64 + 63 <= i0) return;   // whole tile in the lower triangle: left to the caller
  const size_t jc = j < n2 ? j : n2 - 1;
  double d[kEuclidRows];
#pragma unroll
  for (int r = 0; r < kEuclidRows; ++r) d[r] = 0.0;
  for (int b = 0; b < B; ++b) {
    const double t2 = X2[(size_t)b * ldx2 + jc];
    const double* row = X1 + (size_t)b * ldx1 + i0;
#pragma unroll
    for (int r = 0; r < kEuclidRows; ++r) {
      const double t = t2 - row[i0 + r < n1 ? r : 0];
      d[r] = __builtin_fma(t, t, d[r]);
    }
  }
  if (j >= n2) return;
#pragma unroll
  for (int r = 0; r < kEuclidRows; ++r) {
    const size_t i = i0 + r;
    if (i >= n1 || (intra == kPairUpperRows && j <= i)) continue;
    out[i * ldo + j] = (intra == kPairRectangle || j > i) ? sqrt(d[r]) : __builtin_nan("");
  }
}

// the epilogue of pair_gram_kernel for st.gk: a weighted operand (pair_prep_kernel with w) carries the weights already, so
// weighted correlation is g / sqrt(s_i s_j) -- the Cosinus epilogue -- and weighted covariance is g -- the scalar
// product's: no (B-1) factors
static int gram_kind(const Stat& st) {
  if (!st.d_w) return st.gk;
  return st.gk == CMX_STAT_CORRELATION ? CMX_STAT_COSINUS : st.gk == CMX_STAT_COVARIANCE ? CMX_STAT_SCALAR_PRODUCT : st.gk;
}

hipError_t launch_pair_gram(const Stat& st, const PairOperand& a, const PairOperand& b, PairMode mode, double* d_out, size_t ldo,
                            const GramBatch& z, size_t irow0, hipStream_t stream) {
  const int kind = gram_kind(st);
  for (size_t z0 = 0; z0 < z.nblk; z0 += 65535) {     // grid.z limit
    const unsigned gz = (unsigned)std::min<size_t>(65535, z.nblk - z0);
    const size_t so = z0 * z.zsite, xo = z0 * z.zx;
    double* out = d_out + z0 * z.zout;
    if (kind == CMX_STAT_EUCLIDIAN_DISTANCE) {
      hipLaunchKernelGGL(pair_euclid_kernel, dim3((unsigned)((b.n + 63) / 64), (unsigned)((a.n + 4 * kEuclidRows - 1) / (4 * kEuclidRows)), gz), dim3(256), 0, stream,
                         st.B, a.X + xo, a.n, a.ldx, b.X + xo, b.n, b.ldx, mode, out, ldo, z.zx, z.zout);
    } else {
      dim3 grid((unsigned)((b.n + 255) / 256), (unsigned)((a.n + 63) / 64), gz);
      hipLaunchKernelGGL(pair_gram_kernel, grid, dim3(4 * kWave), 0, stream, kind, st.B, pair_Bp(st.B), a.X + xo, a.s + so, a.r + so, a.n,
                         a.ldx, b.X + xo, b.s + so, b.r + so, b.n, b.ldx, mode, out, ldo, z.zsite, z.zout, z.zx, irow0);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace cmx
