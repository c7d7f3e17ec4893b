// mica_mfma_kernel: column mutual information as a one-hot Gram on v_mfma_i32_32x32x32_i8 (CoMap/Mica.cpp:349-361).
#include <algorithm>

#include "cmx_device.h"
#include "cmx_lanes.h"

namespace cmx {

// ------------------------------------------------------------------------------------------------ Mica column MI
// SiteTools::mutualInformation / jointEntropy / entropy (resolveUnknowns = true), natural log (Mica.cpp:93-95).
// LDS-table kernel (the general path: any ambiguity code, fractional counts in fp64): one wave per (column i, 16 columns
// j); the 16 joint tables of A x A doubles live in LDS ([cell][pair slot]), four lanes share a pair and spread the
// (fractional) unit counts of their quarter of the taxa into its table with LDS atomics.  The MFMA path below serves the
// columns without partial ambiguity codes; this kernel then only sees the pairs that involve a flagged column (and
// returns after one load when no column is flagged).
template <int A>
__global__ __launch_bounds__(64) void mi_columns_kernel(int T, const uint32_t* __restrict__ masks,
                                                        const uint8_t* __restrict__ aln1, size_t n1, size_t ld1,
                                                        const uint8_t* __restrict__ aln2, size_t n2, size_t ld2,
                                                        int intra, double* __restrict__ mi, double* __restrict__ hj,
                                                        size_t ldo, const uint8_t* __restrict__ flag1,
                                                        const uint8_t* __restrict__ flag2, const int* __restrict__ anyflag) {
  // with flags (MFMA path active) this kernel only serves pairs that involve a column with ambiguous symbols; when no
  // column at all is flagged every workgroup leaves after one load
  if (anyflag && *anyflag == 0) return;
  // LDS: joint table [A*A][16 lanes] fp64 per quarter-wave = A*A*16*8 B (51 KB for A = 20): 16 pairs per block pass
  extern __shared__ double tab[];
  const int lane = threadIdx.x;
  const int sub = lane & 15;       // pair slot
  const int part = lane >> 4;      // 4 lanes cooperate on one pair: taxa are split in 4 strides
  const size_t nbj = (n2 + 15) / 16, ntiles = nbj * n1;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t i = tile / nbj;
    const size_t jb = tile % nbj;
    if (flag1) {
      bool any = flag1[i] != 0;
      for (size_t q = jb * 16; !any && q < jb * 16 + 16 && q < n2; ++q) any = flag2[q] != 0;
      if (!any) continue;
    }
    const size_t j = jb * 16 + sub;
    const bool valid = j < n2 && (!intra || j > i);
    const size_t jj = j < n2 ? j : n2 - 1;
    __syncthreads();   // the previous tile's readers are done with the table
    for (int q = lane; q < A * A * 16; q += 64) tab[q] = 0.0;
    __syncthreads();
    for (int t = part; t < T; t += 4) {
      const unsigned c1 = aln1[(size_t)t * ld1 + i], c2 = aln2[(size_t)t * ld2 + jj];
      if (c1 < (unsigned)A && c2 < (unsigned)A) {
        atomicAdd(&tab[(c1 * A + c2) * 16 + sub], 1.0);
      } else {
        const uint32_t m1 = c1 < (unsigned)A ? (1u << c1) : masks[c1], m2 = c2 < (unsigned)A ? (1u << c2) : masks[c2];
        const double w = 1.0 / (double)(__popc(m1) * __popc(m2));
        for (int a = 0; a < A; ++a)
          if ((m1 >> a) & 1u)
            for (int b = 0; b < A; ++b)
              if ((m2 >> b) & 1u) atomicAdd(&tab[(a * A + b) * 16 + sub], w);
      }
    }
    __syncthreads();
    if (part == 0) {
      double p1[A], p2[A];
#pragma unroll
      for (int a = 0; a < A; ++a) { p1[a] = 0.0; p2[a] = 0.0; }
#pragma unroll
      for (int a = 0; a < A; ++a)
#pragma unroll
        for (int b = 0; b < A; ++b) {
          const double v = tab[(a * A + b) * 16 + sub];
          p1[a] += v;
          p2[b] += v;
        }
      double s = 0.0, h = 0.0;
#pragma unroll
      for (int a = 0; a < A; ++a)
#pragma unroll
        for (int b = 0; b < A; ++b) {
          const double pab = tab[(a * A + b) * 16 + sub] / T;
          if (pab > 0.0) {
            s += pab * log(pab / ((p1[a] / T) * (p2[b] / T)));
            h -= pab * log(pab);
          }
        }
      if (j < n2 && (!flag1 || flag1[i] || flag2[j])) {
        mi[i * ldo + j] = valid ? s : __builtin_nan("");
        hj[i * ldo + j] = valid ? h : __builtin_nan("");
      }
    }
  }
}

// MI / joint entropy of LISTED column pairs (idx1[p], idx2[p]): the building block of Mica's null distributions
// (non-parametric bootstrap = random pairs of the data, Mica.cpp:399-468; parametric bootstrap = column j of one
// simulated alignment against column j of another, Mica.cpp:469-548).  Same table arithmetic as mi_columns_kernel.
template <int A>
__global__ __launch_bounds__(64) void mi_pairs_kernel(int T, const uint32_t* __restrict__ masks,
                                                      const uint8_t* __restrict__ aln1, size_t ld1,
                                                      const uint8_t* __restrict__ aln2, size_t ld2,
                                                      const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2,
                                                      size_t npairs, double* __restrict__ mi, double* __restrict__ hj) {
  extern __shared__ double tab[];
  const int lane = threadIdx.x, sub = lane & 15, part = lane >> 4;
  const size_t p = (size_t)blockIdx.x * 16 + sub;
  const size_t pp = p < npairs ? p : npairs - 1;
  const size_t i = (size_t)idx1[pp], j = (size_t)idx2[pp];
  for (int q = lane; q < A * A * 16; q += 64) tab[q] = 0.0;
  __syncthreads();
  for (int t = part; t < T; t += 4) {
    const unsigned c1 = aln1[(size_t)t * ld1 + i], c2 = aln2[(size_t)t * ld2 + j];
    if (c1 < (unsigned)A && c2 < (unsigned)A) {
      atomicAdd(&tab[(c1 * A + c2) * 16 + sub], 1.0);
    } else {
      const uint32_t m1 = c1 < (unsigned)A ? (1u << c1) : masks[c1], m2 = c2 < (unsigned)A ? (1u << c2) : masks[c2];
      const double w = 1.0 / (double)(__popc(m1) * __popc(m2));
      for (int a = 0; a < A; ++a)
        if ((m1 >> a) & 1u)
          for (int b = 0; b < A; ++b)
            if ((m2 >> b) & 1u) atomicAdd(&tab[(a * A + b) * 16 + sub], w);
    }
  }
  __syncthreads();
  if (part == 0 && p < npairs) {
    double p1[A], p2[A];
#pragma unroll
    for (int a = 0; a < A; ++a) { p1[a] = 0.0; p2[a] = 0.0; }
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
      for (int b = 0; b < A; ++b) {
        const double v = tab[(a * A + b) * 16 + sub];
        p1[a] += v;
        p2[b] += v;
      }
    double s = 0.0, h = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
      for (int b = 0; b < A; ++b) {
        const double pab = tab[(a * A + b) * 16 + sub] / T;
        if (pab > 0.0) {
          s += pab * log(pab / ((p1[a] / T) * (p2[b] / T)));
          h -= pab * log(pab);
        }
      }
    mi[p] = s;
    hj[p] = h;
  }
}

hipError_t launch_mi_pairs(int A, int T, const uint32_t* d_masks, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2,
                           size_t ld2, const int64_t* d_idx1, const int64_t* d_idx2, size_t npairs, double* d_mi,
                           double* d_hj, hipStream_t stream) {
  if (A != 20 && A != 4) return launch_mi_pairs_wide(A, T, d_aln1, ld1, d_aln2, ld2, d_idx1, d_idx2, npairs, d_mi, d_hj, stream);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((npairs + 15) / 16)), dim3(64), sizeof(double) * A * A * 16, stream, T, d_masks, d_aln1, ld1,
                       d_aln2, ld2, d_idx1, d_idx2, npairs, d_mi, d_hj);
  };
  if (A == 20) launch(mi_pairs_kernel<20>); else launch(mi_pairs_kernel<4>);
  return hipGetLastError();
}

// ---- MFMA path (SURVEY 8d "Mica MI"): for columns without ambiguous symbols the joint table of a column pair is one
// 32x32 block of the Gram matrix of one-hot matrices, H_i (32 x T) . H_j^T, exact in int8 x int8 -> int32.  With integer
// counts c the entropies need no logarithm at run time: sum_ab p_ab ln p_ab = (1/T) sum_ab f(c_ab) - ln T with
// f(c) = c ln c read from a (T+1)-entry table, so MI = ln T + (sum_ab f(c_ab) - sum_a f(c_a) - sum_b f(c_b)) / T and
// the epilogue is a layout-free sum over the accumulator registers.
constexpr int kMicaK = 32;   // taxa per MFMA step (v_mfma_i32_32x32x32_i8)

// one block per column: one-hot rows H[col][a][t] (a < 32, t < Tp, zero padded).  A symbol compatible with EVERY state
// (gap, X, N: mask = all ones) becomes pseudo-state A -- row A of the one-hot matrix -- and the column is marked in
// gap[]: its pairs stay on the matrix cores and the epilogue spreads the pseudo-state's counts (weight 1/A per state,
// the fractional counts of SiteTools::getCounts(.., resolveUnknowns = true)).  Any other ambiguity code sets flag[]
// (pairs of that column go to the LDS-table kernel).  S[col] = sum_a f(count_a) with the fractional counts.
__global__ __launch_bounds__(256) void mica_onehot_kernel(int A, int T, int Tp, const uint32_t* __restrict__ masks,
                                                          const uint8_t* __restrict__ aln, size_t ld,
                                                          int8_t* __restrict__ H, uint8_t* __restrict__ codes /*[n][Tp]: the one-hot row of each taxon (state, A = unknown), 63 = none*/,
                                                          uint8_t* __restrict__ flag,
                                                          uint8_t* __restrict__ gap, double* __restrict__ S,
                                                          int* __restrict__ anyflag, size_t n) {
  __shared__ int cnt[33];
  __shared__ int amb;
  const size_t i = blockIdx.x;
  if (i >= n) {   // the columns of padding behind the last one (kMicaCodePad): "no row" everywhere
    for (int t = threadIdx.x; t < Tp; t += blockDim.x) codes[i * (size_t)Tp + t] = 63;
    return;
  }
  const uint32_t full = (1u << A) - 1u;
  if (threadIdx.x < 33) cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) amb = 0;
  __syncthreads();
  for (int t = threadIdx.x; t < Tp; t += blockDim.x) {
    unsigned c = t < T ? aln[(size_t)t * ld + i] : 63u;
    if (t < T) {
      if (c >= (unsigned)A) {
        if ((masks[c] & full) == full) c = (unsigned)A;     // unknown: pseudo-state
        else { amb = 1; c = 63u; }
      }
      if (c <= (unsigned)A) atomicAdd(&cnt[c], 1);
    }
    codes[i * (size_t)Tp + t] = (uint8_t)c;
    if (H) {
#pragma unroll
      for (int a = 0; a < 32; ++a) H[(i * 32 + a) * (size_t)Tp + t] = (int8_t)((c == (unsigned)a) ? 1 : 0);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    const double g = (double)cnt[A] / (double)A;
    for (int a = 0; a < A; ++a) {
      const double c = (double)cnt[a] + g;
      if (c > 0.0) s += c * log(c);
    }
    S[i] = s;
    flag[i] = (uint8_t)amb;
    gap[i] = (uint8_t)(cnt[A] > 0 ? 1 : 0);
    if (amb) atomicOr(anyflag, 1);
  }
}

// The same classification without the one-hot matrices (what the packed kernels need: codes, flags, column sums), 64 columns
// per workgroup: the alignment is [taxon][column], the codes [column][taxon].  mica_onehot_kernel reads a column with
// 256 one-byte loads from 256 cache lines (and counts with 256 LDS atomics on 21 addresses); here a wave reads 64 columns
// of one taxon in one line, counts per (column, state), and a tile of 64 taxa x 64 columns is turned in LDS so that the
// codes leave as 64-byte rows too.  S is summed in the same state order: the same bits.
__global__ __launch_bounds__(256) void mica_codes_kernel(int A, int T, int Tp, const uint32_t* __restrict__ masks,
                                                         const uint8_t* __restrict__ aln, size_t ld, uint8_t* __restrict__ codes,
                                                         uint8_t* __restrict__ flag, uint8_t* __restrict__ gap, double* __restrict__ S,
                                                         int* __restrict__ anyflag, size_t n, size_t npad /* columns behind n that get "no row" codes */) {
  constexpr int kTileRow = 68;           // bytes per taxon of the tile: 17 dwords, so that a column is read conflict-free
  constexpr int kCnt = 35;               // counts per column (states, the unknown; odd stride)
  __shared__ __attribute__((aligned(4))) uint8_t tile[64 * kTileRow];
  __shared__ int cnt[64 * kCnt];
  __shared__ int amb[64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t i0 = (size_t)blockIdx.x * 64, i = i0 + lane;
  const uint32_t full = (1u << A) - 1u;
  for (int k = threadIdx.x; k < 64 * kCnt; k += 256) cnt[k] = 0;
  if (threadIdx.x < 64) amb[threadIdx.x] = 0;
  __syncthreads();
  for (int tc = 0; tc < Tp; tc += 64) {
#pragma unroll 4
    for (int r = 0; r < 16; ++r) {       // wave w: taxa tc + 4 r + w, one column per lane
      const int tl = 4 * r + w, t = tc + tl;
      unsigned c = 63u;
      if (t < T && i < n) {
        c = aln[(size_t)t * ld + i];
        if (c >= (unsigned)A) {
          if ((masks[c] & full) == full) c = (unsigned)A;     // unknown: pseudo-state
          else { amb[lane] = 1; c = 63u; }
        }
        if (c <= (unsigned)A) atomicAdd(&cnt[lane * kCnt + (int)c], 1);
      }
      tile[tl * kTileRow + lane] = (uint8_t)c;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < 16; ++r) {       // wave w: columns 4 r + w, one taxon per lane
      const int col = 4 * r + w;
      if (i0 + col < n + npad && tc + lane < Tp) codes[(i0 + col) * (size_t)Tp + tc + lane] = tile[lane * kTileRow + col];
    }
    __syncthreads();
  }
  if (threadIdx.x < 64 && i < n) {
    const int* cc = cnt + lane * kCnt;
    double s = 0.0;
    const double g = (double)cc[A] / (double)A;
    for (int a = 0; a < A; ++a) {
      const double c = (double)cc[a] + g;
      if (c > 0.0) s += c * log(c);
    }
    S[i] = s;
    flag[i] = (uint8_t)amb[lane];
    gap[i] = (uint8_t)(cc[A] > 0 ? 1 : 0);
    if (amb[lane]) atomicOr(anyflag, 1);
  }
}

// f[c] = c ln c for the integer counts 0..T, followed by f2[m] = (m / A^2) ln(m / A^2) for m = 0..A^2 T: the fractional
// count of a pair with unknowns is c_ab = N_ab + (N_aA + N_Ab) / A + N_AA / A^2 = m / A^2 with the INTEGER
// m = A^2 N_ab + A (N_aA + N_Ab) + N_AA, so those pairs need no logarithm at run time either
__global__ void mica_ftable_kernel(int T, int A, double* __restrict__ f, int* __restrict__ anyflag) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) *anyflag = 0;
  if (c <= T) f[c] = c > 1 ? (double)c * log((double)c) : 0.0;
  const int M = A * A * T;
  if (c <= M) {
    const double v = (double)c / (double)(A * A);
    const double fv = c > 0 ? v * log(v) : 0.0;
    f[T + 1 + c] = fv;
    // third table (cmx_mica4.hip): a zero, then f2[M0 ..], so that "m below M0" can be a load of entry 0
    const int M0 = M + 1 < kMicaLdsF2 ? M + 1 : kMicaLdsF2;
    double* hi = f + (T + 1) + (M + 1);
    if (c == 0) hi[0] = 0.0;
    if (c >= M0) hi[c - M0 + 1] = fv;
  }
}
// the three tables: T + 1 entries of f, A^2 T + 1 of f2, and room for a zero and all of f2 again
size_t mica_ftab_entries(int A, int T) { return (size_t)(T + 1) + 2 * ((size_t)A * A * T + 1) + 2; }

// One workgroup (8 waves) per 8 x 4 tile of column pairs (8 columns of the first alignment, 4 of the second), wave w owns
// the 2 x 2 sub-tile (rows 2*(w/2).., columns 2*(w%2)..): 64 accumulator registers, so that two workgroups share a CU
// (four waves per SIMD) and one workgroup's barriers and table epilogue overlap the other's MFMAs.  The 12 operand tiles
// of a k-step (64 lanes x 16 B each) go through LDS once per workgroup.
constexpr int kMicaTileI = 8, kMicaTileJ = 4;
template <int A>
__global__ __launch_bounds__(512, 2) void mica_mfma_kernel(int T, int Tp, const int8_t* __restrict__ H1, size_t n1,
                                                           const uint8_t* __restrict__ flag1, const uint8_t* __restrict__ gap1,
                                                           const double* __restrict__ S1,
                                                           const int8_t* __restrict__ H2, size_t n2,
                                                           const uint8_t* __restrict__ flag2, const uint8_t* __restrict__ gap2,
                                                           const double* __restrict__ S2,
                                                           const double* __restrict__ ftab_g, int intra,
                                                           double* __restrict__ mi, double* __restrict__ hj, size_t ldo) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mica_smem[];
  double* ftab = reinterpret_cast<double*>(mica_smem);                       // [T + 1]
  cmx_i4* ops = reinterpret_cast<cmx_i4*>(mica_smem + (((size_t)(T + 1) * 8 + 15) & ~(size_t)15));  // [2][12][64]
  constexpr int NOP = kMicaTileI + kMicaTileJ;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
  for (int c = tid; c <= T; c += 512) ftab[c] = ftab_g[c];
  const size_t i0 = (size_t)blockIdx.y * kMicaTileI, j0 = (size_t)blockIdx.x * kMicaTileJ;
  if (intra && j0 + kMicaTileJ <= i0 + 1) {   // no pair with j > i in this tile: only the NaN convention of the intra layout
    if (tid < kMicaTileI * kMicaTileJ) {
      const size_t i = i0 + tid / kMicaTileJ, j = j0 + tid % kMicaTileJ;
      if (i < n1 && j < n2 && !flag1[i] && !flag2[j]) {
        mi[i * ldo + j] = __builtin_nan("");
        hj[i * ldo + j] = __builtin_nan("");
      }
    }
    return;
  }
  // does any column of this tile carry unknowns?  (independent loads, issued here so that the main loop hides them)
  unsigned gapbits = 0;
#pragma unroll
  for (int c = 0; c < kMicaTileI; ++c) gapbits |= gap1[i0 + c < n1 ? i0 + c : n1 - 1];
#pragma unroll
  for (int c = 0; c < kMicaTileJ; ++c) gapbits |= gap2[j0 + c < n2 ? j0 + c : n2 - 1];
  // loader role of this thread: 12 operand tiles x 64 lanes = 768 slots of 16 bytes, threads 0..383 take two each
  // (operand tile q = slot / 64: q < 8 column i0 + q of H1, else column j0 + q - 8 of H2; a lane's 16 bytes are row
  // (lane % 32), taxa group (lane / 32) of the one-hot matrix)
  const bool loader = tid < NOP * 32;
  const int q = loader ? tid >> 5 : 0;
  const size_t col = q < kMicaTileI ? (i0 + q < n1 ? i0 + q : n1 - 1) : (j0 + q - kMicaTileI < n2 ? j0 + q - kMicaTileI : n2 - 1);
  const int8_t* Hq = (q < kMicaTileI ? H1 : H2) + col * 32 * (size_t)Tp;
  const int l0 = 2 * (tid & 31);
  cmx_i16v acc[2][2];
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ii][jj][v] = 0;
  // Operand fetch runs THREE k-steps ahead of the MFMAs (registers -> LDS at the top of each step): with one step of
  // lookahead every k-step exposed most of an L2 / HBM round trip behind its barrier -- eight of them per tile at 256
  // taxa were three quarters of the kernel's time, the matrix cores idle meanwhile.
  constexpr int kAhead = 3;
  cmx_i4 st[kAhead][2] = {};
  auto fetch = [&](cmx_i4 (&dst)[2], int ks) {
    if (loader && ks < Tp) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int l = l0 + u;
        dst[u] = *reinterpret_cast<const cmx_i4*>(Hq + (size_t)(l & 31) * Tp + ks + 16 * (l >> 5));
      }
    }
  };
#pragma unroll
  for (int d = 0; d < kAhead; ++d) fetch(st[d], d * kMicaK);
  int buf = 0;
  auto step = [&](cmx_i4 (&cur)[2], int ks) {
    if (loader) {
#pragma unroll
      for (int u = 0; u < 2; ++u) ops[(buf * NOP + q) * 64 + l0 + u] = cur[u];
    }
    __syncthreads();
    fetch(cur, ks + kAhead * kMicaK);
    cmx_i4 a[2], b[2];
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) a[ii] = ops[(buf * NOP + 2 * wi + ii) * 64 + lane];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) b[jj] = ops[(buf * NOP + kMicaTileI + 2 * wj + jj) * 64 + lane];
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) acc[ii][jj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ii], b[jj], acc[ii][jj], 0, 0, 0);
    buf ^= 1;
  };
  for (int ks = 0; ks < Tp; ks += kAhead * kMicaK) {
    step(st[0], ks);
    if (ks + kMicaK < Tp) step(st[1], ks + kMicaK);
    if (ks + 2 * kMicaK < Tp) step(st[2], ks + 2 * kMicaK);
  }
  const double lnT = log((double)T), invT = 1.0 / (double)T;
  // sum_ab f(c_ab) of the wave's four pairs: 16 table lookups per lane and pair, then ONE reduce-scatter for all four
  // (lane bits 5 and 4 with v_permlane32/16_swap: row r of 16 lanes ends up with pair r; bits 3..0 with DPP row
  // rotations) instead of four butterfly reductions through ds_bpermute
  double ps[4];
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      // register v of a lane holds table row 8 (v / 4) + v % 4 (+ 4 in the upper half of the wave): rows past the
      // pseudo-state (row A) are padding of the 32-row tile, structurally zero -- no lookup for them
      double s = 0.0;
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (8 * (v / 4) + v % 4 <= A) s += ftab[acc[ii][jj][v]];   // compile-time after unrolling
      ps[2 * ii + jj] = s;
    }
  swap32(ps[0], ps[2]);
  swap32(ps[1], ps[3]);
  double k0 = ps[0] + ps[2], k1 = ps[1] + ps[3];
  swap16(k0, k1);
  double s = k0 + k1;
  s += mica_dpp_f64<0x128>(s);   // row_ror:8
  s += mica_dpp_f64<0x124>(s);   // row_ror:4
  s += mica_dpp_f64<0x122>(s);   // row_ror:2
  s += mica_dpp_f64<0x121>(s);   // row_ror:1
  const bool blockgap = gapbits != 0;
  // Pairs with unknowns (pseudo-state A): the integer table N (states + pseudo-state, from the same accumulators) is
  // expanded into the fractional counts c_ab = N_ab + (N_aA + N_Ab) / A + N_AA / A^2 and f is evaluated with a
  // logarithm per cell.  v_mfma_i32_32x32x32_i8 leaves D[row][col] in register v of lane l with
  // row = 8 (v / 4) + 4 (l / 32) + v % 4, col = l % 32.
  {
    if (blockgap) {
      __syncthreads();                                  // the operand buffers are free now: reuse them as count tables
      int* tile = reinterpret_cast<int*>(ops) + w * 448;   // (A + 1)^2 <= 441 ints per wave
      const int A1 = A + 1;
      const double* f2 = ftab_g + T + 1;   // (m / A^2) ln(m / A^2), global (A^2 T + 1 entries, L2-resident)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = r >> 1, jj = r & 1;
        const size_t i = i0 + 2 * wi + ii, j = j0 + 2 * wj + jj;
        if (!(gap1[i < n1 ? i : n1 - 1] || gap2[j < n2 ? j : n2 - 1])) continue;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int row = 8 * (v / 4) + 4 * (lane / 32) + v % 4, col = lane % 32;
          if (row <= A && col <= A) tile[row * A1 + col] = acc[ii][jj][v];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const int gg = tile[A * A1 + A];
        int mm[(A * A + 63) / 64];   // all table indices first, then all gathers (not one dependent L2 round trip each)
#pragma unroll
        for (int k = 0; k < (A * A + 63) / 64; ++k) {
          const int e = lane + 64 * k, x = e / A, y = e % A;
          mm[k] = e < A * A ? A * A * tile[x * A1 + y] + A * (tile[x * A1 + A] + tile[A * A1 + y]) + gg : 0;   // f2[0] = 0
        }
        double sg = 0.0;
#pragma unroll
        for (int k = 0; k < (A * A + 63) / 64; ++k) sg += f2[mm[k]];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sg += __shfl_xor(sg, off, 64);
        if ((lane >> 4) == r) s = sg;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  {
    const int r = lane >> 4;
    const size_t i = i0 + 2 * wi + (r >> 1), j = j0 + 2 * wj + (r & 1);
    if ((lane & 15) == 0 && i < n1 && j < n2 && !flag1[i] && !flag2[j]) {
      const bool valid = !intra || j > i;
      mi[i * ldo + j] = valid ? lnT + (s - S1[i] - S2[j]) * invT : __builtin_nan("");
      hj[i * ldo + j] = valid ? lnT - s * invT : __builtin_nan("");
    }
  }
}
// mica_smem of mica_mfma_kernel: f[0 .. T], two buffers of twelve operand tiles
static size_t mica_mfma_lds_bytes(int T) {
  return (((size_t)(T + 1) * 8 + 15) & ~(size_t)15) + 2 * (kMicaTileI + kMicaTileJ) * 64 * sizeof(cmx_i4);
}

// ---- protein alphabet, packed tiles.  A column needs 21 one-hot rows (20 states + the pseudo-state of unknowns), a
// 32-row MFMA tile per column wastes a third of the rows and (32/21)^2 of the matrix work AND of the table epilogue.
// Here THREE columns share a 64-row block (rows 21 c + state, row 63 = zero): a wave's 2 x 2 MFMA tiles are the 64 x 64
// Gram block of 3 x 3 column pairs (9 pairs where the one-column-per-tile kernel has 4), same operand traffic, same
// accumulators.  Workgroup tile: 12 columns of the first alignment x 6 of the second (4 x 2 blocks, one per wave).
// The epilogue sums f(count) per (column of the block row, column of the block column): an accumulator register's row
// block is known at compile time up to the lane's half (rows + 4 in lanes >= 32), its column block from the lane.
constexpr int kMica3I = 12, kMica3J = 6, kMicaP = 21;
__device__ __forceinline__ void mica3_tile(int T, int Tp, const uint8_t* __restrict__ C1, size_t n1,
                                                            const uint8_t* __restrict__ flag1, const uint8_t* __restrict__ gap1,
                                                            const double* __restrict__ S1,
                                                            const uint8_t* __restrict__ C2, size_t n2,
                                                            const uint8_t* __restrict__ flag2, const uint8_t* __restrict__ gap2,
                                                            const double* __restrict__ S2,
                                                            const double* __restrict__ ftab_g, int intra,
                                                            double* __restrict__ mi, double* __restrict__ hj, size_t ldo,
                                                            unsigned ntx, unsigned tlin) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mica_smem[];
  constexpr int A = 20, P = kMicaP;
  double* ftab = reinterpret_cast<double*>(mica_smem);                       // [T + 1]
  cmx_i4* ops = reinterpret_cast<cmx_i4*>(mica_smem + (((size_t)(T + 1) * 8 + 15) & ~(size_t)15));  // [4][12][64]
  constexpr int NOP = 12, NI = 8;   // operand tiles per k-step: 8 of the first alignment (4 blocks), 4 of the second
  // [18][Tp]: the tile's columns, one byte per taxon (16 KiB behind the operand buffers: the unknowns' path lays 8 x 8 KiB over both)
  uint8_t* codes = reinterpret_cast<uint8_t*>(ops + 4 * NOP * 64) + 16384;
  double* Scol = reinterpret_cast<double*>(codes + (size_t)(kMica3I + kMica3J) * Tp);   // [18] S of the tile's columns (12 + 6)
  int* fcol = reinterpret_cast<int*>(Scol + 18);   // [18] bit 0 partial ambiguity codes, bit 1 unknowns, bit 2 past the end
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
  const size_t i0 = (size_t)(tlin / ntx) * kMica3I, j0 = (size_t)(tlin % ntx) * kMica3J;
  if (intra && j0 + kMica3J <= i0 + 1) {   // no pair with j > i in this tile: only the NaN convention of the intra layout
    if (tid < kMica3I * kMica3J) {
      const size_t i = i0 + tid / kMica3J, j = j0 + tid % kMica3J;
      if (i < n1 && j < n2 && !flag1[i] && !flag2[j]) {
        mi[i * ldo + j] = __builtin_nan("");
        hj[i * ldo + j] = __builtin_nan("");
      }
    }
    return;
  }
  // The operands are NOT read as one-hot matrices (21 rows x T bytes per column, 34 GB through the L2 for 5000 x 5000
  // columns -- the workgroups spent their lives waiting for them): a column travels as its T symbol bytes (the one-hot
  // row of each taxon), all 18 columns of the tile in one round trip, and the loader threads expand them to one-hot
  // operand tiles in LDS k-step by k-step (a dword of four symbols XOR the row's state, zero-byte test -> 0x01 bytes).
  const int chunks = Tp / 16;                  // 16-byte pieces per column
  for (int e = tid; e < (kMica3I + kMica3J) * chunks; e += 512) {
    const int c = e / chunks, o = e % chunks;
    const bool fi = c < kMica3I;
    const size_t want = fi ? i0 + c : j0 + (c - kMica3I);
    const size_t col = want < (fi ? n1 : n2) ? want : (fi ? n1 : n2) - 1;
    reinterpret_cast<cmx_i4*>(codes)[e] = *reinterpret_cast<const cmx_i4*>((fi ? C1 : C2) + col * (size_t)Tp + 16 * o);
  }
  for (int c = tid; c <= T; c += 512) ftab[c] = ftab_g[c];
  // per-column scalars, once per workgroup (not per thread, and not at the very end where their latency would show)
  if (tid < 18) {
    const bool fi = tid < kMica3I;
    const size_t c = fi ? i0 + tid : j0 + (tid - kMica3I), nc = fi ? n1 : n2;
    const size_t cc = c < nc ? c : nc - 1;
    Scol[tid] = (fi ? S1 : S2)[cc];
    fcol[tid] = (int)(fi ? flag1 : flag2)[cc] | ((int)(fi ? gap1 : gap2)[cc] << 1) | (c < nc ? 0 : 4);
  }
  // loader role: 12 operand tiles x 64 lanes = 768 slots of 16 bytes, threads 0..383 take two each.  Operand tile q:
  // q < 8: rows 32 (q % 2) .. + 31 of block q / 2 of the first alignment, else of block (q - 8) / 2 of the second; packed
  // row R = column R / 21 of the block, one-hot row R % 21; R = 63 is padding (state 31 matches no symbol).
  const bool loader = tid < NOP * 32;
  const int q = loader ? tid >> 5 : 0;
  const int l0 = 2 * (tid & 31);
  unsigned srow[2];      // the row's state, replicated in the four bytes of a dword
  const uint8_t* crow[2];  // the row's column in `codes`, at this lane's taxa group
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int R = 32 * (q & 1) + ((l0 + u) & 31);
    const int cb = R / P, st_ = R == 63 ? 31 : R % P;
    const int slot = (q < NI ? 3 * (q >> 1) : kMica3I + 3 * ((q - NI) >> 1)) + (cb < 3 ? cb : 2);
    srow[u] = (unsigned)st_ * 0x01010101u;
    crow[u] = codes + (size_t)slot * Tp + 16 * (l0 >> 5);
  }
  cmx_i16v acc[2][2];
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ii][jj][v] = 0;
  __syncthreads();   // symbols, table and column scalars are in LDS
  // two k-steps per barrier: four operand buffers, the pair being multiplied and the pair being expanded
  int buf = 0;
  for (int ks = 0; ks < Tp; ks += 2 * kMicaK) {
    const bool two = ks + kMicaK < Tp;
    if (loader) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 0 || two) {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const cmx_i4 sy = *reinterpret_cast<const cmx_i4*>(crow[u] + ks + h * kMicaK);
            cmx_i4 oh;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const unsigned x = (unsigned)sy[d] ^ srow[u];
              const unsigned t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 where the byte of x is zero
              oh[d] = (int)(t >> 7);
            }
            ops[((buf + h) * NOP + q) * 64 + l0 + u] = oh;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 0 || two) {
        cmx_i4 a[2], b[2];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) a[ii] = ops[((buf + h) * NOP + 2 * wi + ii) * 64 + lane];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) b[jj] = ops[((buf + h) * NOP + NI + 2 * wj + jj) * 64 + lane];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) acc[ii][jj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ii], b[jj], acc[ii][jj], 0, 0, 0);
      }
    }
    buf ^= 2;
  }
  const double lnT = log((double)T), invT = 1.0 / (double)T;
  const bool hi = lane >= 32;
  const int cl = lane & 31;
  // per lane: sums by (column a of the block row, MFMA tile column jj).  Register v of tile (ii, jj) is packed row
  // R = 32 ii + 8 (v / 4) + v % 4 (+ 4 if hi), packed column 32 jj + cl.
  double pa[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int R0 = 32 * ii + 8 * (v / 4) + v % 4, a0 = R0 / P, a1 = (R0 + 4) / P;
        const double val = ftab[acc[ii][jj][v]];
        if (a0 == a1) {
          pa[a0][jj] += val;
        } else {
          pa[a0][jj] += hi ? 0.0 : val;
          if (a1 < 3) pa[a1][jj] += hi ? val : 0.0;   // a1 == 3: packed row 63, padding (its counts are zero)
        }
      }
  // by column b of the block column: tile 0 holds packed columns 0..31 (b = 0 for cl < 21, else 1), tile 1 holds 32..63
  // (b = 1 for cl < 10, else 2; packed column 63 is padding)
  double sres[3];   // after the reductions: lanes with lane >> 4 == r hold pair 4 g + r in sres[g] (pair = 3 a + b)
  {
    double t[9];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[3 * a + 0] = cl < 21 ? pa[a][0] : 0.0;
      t[3 * a + 1] = (cl >= 21 ? pa[a][0] : 0.0) + (cl < 10 ? pa[a][1] : 0.0);
      t[3 * a + 2] = cl >= 10 ? pa[a][1] : 0.0;
    }
    sres[0] = mica_reduce4(t[0], t[1], t[2], t[3]);
    sres[1] = mica_reduce4(t[4], t[5], t[6], t[7]);
    sres[2] = mica_reduce4(t[8], 0.0, 0.0, 0.0);
  }
  int gapbits = 0;
#pragma unroll
  for (int c = 0; c < kMica3I + kMica3J; ++c) gapbits |= fcol[c] & 2;
  if (gapbits != 0) {
    // Pairs with unknowns: the fractional counts of resolveUnknowns = true are m / A^2 with the integer
    // m = A^2 N_ab + A (N_aG + N_Gb) + N_GG (G = the pseudo-state, row / column 20 of the pair's 21 x 21 block), and
    // sum_ab f2[m] comes from the second table (global, L2-resident).  The wave drops its 64 x 64 accumulator block into
    // LDS once (16-bit counts: T <= 2047), every pair with an unknown reads its cells from there; the nine sums are
    // reduced together like the fast path's.
    __syncthreads();                                     // the operand buffers are free now
    uint16_t* t16 = reinterpret_cast<uint16_t*>(ops) + (size_t)w * 4096;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int R = 32 * ii + 8 * (v / 4) + v % 4 + (hi ? 4 : 0), C = 32 * jj + cl;
          t16[R * 64 + C] = (uint16_t)acc[ii][jj][v];
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const double* f2 = ftab_g + T + 1;   // (m / A^2) ln(m / A^2), A^2 T + 1 entries
    double sg[9];
#pragma unroll
    for (int pr = 0; pr < 9; ++pr) {
      sg[pr] = 0.0;
      const int a = pr / 3, b = pr % 3;
      if (!((fcol[3 * wi + a] | fcol[kMica3I + 3 * wj + b]) & 2)) continue;   // wave-uniform
      const uint16_t* tb = t16 + (P * a) * 64 + P * b;
      const int gg = tb[A * 64 + A];
      int mm[(A * A + 63) / 64];   // all table indices first, then all gathers
#pragma unroll
      for (int q_ = 0; q_ < (A * A + 63) / 64; ++q_) {
        const int e = lane + 64 * q_, x = e / A, y = e % A;
        mm[q_] = e < A * A ? A * A * (int)tb[x * 64 + y] + A * ((int)tb[x * 64 + A] + (int)tb[A * 64 + y]) + gg : 0;   // f2[0] = 0
      }
#pragma unroll
      for (int q_ = 0; q_ < (A * A + 63) / 64; ++q_) sg[pr] += f2[mm[q_]];
    }
    const double g0 = mica_reduce4(sg[0], sg[1], sg[2], sg[3]);
    const double g1 = mica_reduce4(sg[4], sg[5], sg[6], sg[7]);
    const double g2 = mica_reduce4(sg[8], 0.0, 0.0, 0.0);
    // lanes with lane >> 4 == r hold pair 4 g + r: take the general sum where that pair has an unknown
    const int r_ = lane >> 4;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int pr = 4 * g + r_;
      if (pr < 9 && ((fcol[3 * wi + pr / 3] | fcol[kMica3I + 3 * wj + pr % 3]) & 2)) sres[g] = g == 0 ? g0 : (g == 1 ? g1 : g2);
    }
  }
  if ((lane & 15) == 0) {
    const int r = lane >> 4;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int pr = 4 * g + r;
      if (pr < 9) {
        const int ci = 3 * wi + pr / 3, cj = kMica3I + 3 * wj + pr % 3;
        if (!((fcol[ci] | fcol[cj]) & 5)) {              // inside both alignments, no partial ambiguity code
          const size_t i = i0 + ci, j = j0 + (cj - kMica3I);
          const bool valid = !intra || j > i;
          const double s = sres[g];
          mi[i * ldo + j] = valid ? lnT + (s - Scol[ci] - Scol[cj]) * invT : __builtin_nan("");
          hj[i * ldo + j] = valid ? lnT - s * invT : __builtin_nan("");
        }
      }
    }
  }
}

#define CMX_MICA3_PARAMS                                                                                                      \
  int T, int Tp, const uint8_t *__restrict__ C1, size_t n1, const uint8_t *__restrict__ flag1, const uint8_t *__restrict__ gap1, \
      const double *__restrict__ S1, const uint8_t *__restrict__ C2, size_t n2, const uint8_t *__restrict__ flag2,              \
      const uint8_t *__restrict__ gap2, const double *__restrict__ S2, const double *__restrict__ ftab_g, int intra,             \
      double *__restrict__ mi, double *__restrict__ hj, size_t ldo, unsigned ntx
#define CMX_MICA3_ARGS T, Tp, C1, n1, flag1, gap1, S1, C2, n2, flag2, gap2, S2, ftab_g, intra, mi, hj, ldo, ntx
// the proteins the four-wave kernel does not serve: more than 512 taxa, or operands past its 31-bit offsets (mica_path)
__global__ __launch_bounds__(512, 4) void mica_mfma3_kernel(CMX_MICA3_PARAMS, unsigned ntiles, unsigned per_xcd) {
  // XCD-aware tile order.  Workgroups are dealt to the 8 XCDs round-robin (blockIdx.x % 8) and each XCD has its own L2:
  // XCD x takes a contiguous run of the row-major tile order, so that the tiles which complete an output cache line (a
  // tile writes 48-byte pieces of 12 rows) and re-read the same symbol columns meet in one L2.  Measured while this kernel
  // still served 256 taxa: at 5000 x 5000 columns the launch time did not change (6.31 ms either way).  Kept for the
  // traffic, not for the time.
  const unsigned tlin = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  if ((blockIdx.x >> 3) >= per_xcd || tlin >= ntiles) return;
  mica3_tile(CMX_MICA3_ARGS, tlin);
}
// mica_smem of mica_mfma3_kernel: f[0 .. T], four buffers of twelve operand tiles, 16 KiB (the unknowns' path lays 8 x 8 KiB
// over them), the tile's 18 symbol columns, their 18 sums and (20 slots for) their 18 flag words
static size_t mica_mfma3_lds_bytes(int T, int Tp) {
  return (((size_t)(T + 1) * 8 + 15) & ~(size_t)15) + 4 * 12 * 64 * sizeof(cmx_i4) + 16384 + (size_t)(kMica3I + kMica3J) * Tp +
         18 * sizeof(double) + 20 * sizeof(int);
}
// Column entropies (SiteTools::entropy per site; Mica.cpp:349-361 h1 / h2).  Two columns per wave, lane 32 c + a = state a of
// column c: every state's frequency is summed over the taxa in taxon order by its own lane and the A terms are added in
// state order by one lane -- the sums of the one-thread-per-column loop this replaces, bit for bit, in a quarter of its
// time (that loop was 256 x 20 predicated adds per thread on 79 waves: 0.09 ms per alignment of 5 000 columns, twice per
// Mica call, next to a 2.5 ms kernel).
template <int A>
__global__ __launch_bounds__(64) void column_entropy_kernel(int T, const uint32_t* __restrict__ masks, const uint8_t* __restrict__ aln,
                                                            size_t n, size_t ld, double* __restrict__ h) {
  static_assert(A <= 32, "a state per lane, two columns per wave");
  const int lane = threadIdx.x, a = lane & 31, c = lane >> 5;
  const size_t i = 2 * (size_t)blockIdx.x + c, ic = i < n ? i : n - 1;
  double p = 0.0;
  for (int t0 = 0; t0 < T; t0 += 16) {   // sixteen symbols in flight (the lanes of a column read the same byte)
    unsigned cs[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) cs[u] = t0 + u < T ? aln[(size_t)(t0 + u) * ld + ic] : 0xffffffffu;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const unsigned sy = cs[u];
      if (sy == 0xffffffffu) continue;
      const uint32_t m = sy < (unsigned)A ? (1u << sy) : masks[sy];
      const double w = sy < (unsigned)A ? 1.0 : 1.0 / (double)__popc(m);
      if ((m >> a) & 1u) p += w;
    }
  }
  const double term = a < A && p > 0.0 ? (p / T) * log(p / T) : 0.0;   // (s - 0.0 == s: the states that never occur)
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < A; ++k) s -= __shfl(term, 32 * c + k, 64);
  if (a == 0 && i < n) h[i] = s;
}

// Which kernels serve a call.  Above 2 047 taxa the c ln c table and the operand buffers pass 64 KiB of LDS (and the eight-wave
// kernel's 16-bit counts their range): LDS tables alone.  Proteins: the four-wave kernel holds up to sixteen k-steps = 512
// taxa of operands in registers and addresses the symbol arrays and one operand image with 31-bit byte offsets; the
// eight-wave kernel takes the rest.  Nucleotides: the four-wave kernel up to eight k-steps = 256 taxa (its whole weighted
// table in LDS), the same 31-bit offsets -- past them nothing serves the call; the one-column-per-tile kernel above 256 taxa.
// Other alphabets (cmx_mica_wide.hip): the matrix-core kernel up to 2 047 taxa unless the debug switch asks for the plain one; its
// grid is one 32-bit dimension.
MicaPath mica_path(int A, int T, size_t n1, size_t n2) {
  if (A != 4 && A != 20) {
    if (T > 2047 || mica_wide_plain(-1)) return kMicaWidePlain;
    return micaw_tiles(A, n1, n2) <= 0x7fffffffull ? kMicaWide : kMicaRefused;
  }
  if (T > 2047) return kMicaTables;
  const int Tp = mica_padded_taxa(T);
  const bool off31 = (std::max(n1, n2) + kMicaCodePad) * (size_t)Tp < 0x7fffffffull;
  if (A == 20) return Tp <= 512 && off31 && mica4_image_bytes(Tp, n2) / 2 < 0x7fffffffull ? kMicaProtein4 : kMicaProtein8;
  if (Tp > 256) return kMicaDna1;
  return off31 ? kMicaDna4 : kMicaRefused;
}

hipError_t launch_mi_columns(int A, int T, const uint32_t* d_masks, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2,
                             size_t ld2, int intra, double* d_mi, double* d_hj, size_t ldo, double* d_h1, double* d_h2,
                             const MicaWork& work, hipStream_t stream) {
  if (A != 20 && A != 4)
    return launch_mi_columns_wide(A, T, d_aln1, ld1, d_aln2, ld2, intra, d_mi, d_hj, ldo, d_h1, d_h2, work, stream);
  const MicaSide &s1 = work.s[0], &s2 = work.s[1];
  const size_t n1 = s1.n, n2 = s2.n;
  const int Tp = work.Tp;
  const MicaPath path = mica_path(A, T, n1, n2);
  // codes, flags, column sums (and, for the one-column-per-tile kernel, the one-hot matrices) of one alignment
  auto classify = [&](const uint8_t* aln, size_t ld, const MicaSide& s) {
    if (path == kMicaDna1)
      hipLaunchKernelGGL(mica_onehot_kernel, dim3((unsigned)(s.n + kMicaCodePad)), dim3(256), 0, stream, A, T, Tp, d_masks, aln, ld, s.H, s.C,
                         s.flag, s.gap, s.S, work.anyflag, s.n);
    else   // the packed kernels expand the symbol bytes themselves: 64 columns per workgroup
      hipLaunchKernelGGL(mica_codes_kernel, dim3((unsigned)((s.n + kMicaCodePad + 63) / 64)), dim3(256), 0, stream, A, T, Tp, d_masks, aln, ld,
                         s.C, s.flag, s.gap, s.S, work.anyflag, s.n, (size_t)kMicaCodePad);
  };
  // the MFMA paths serve the columns without partial ambiguity codes, the LDS-table kernel behind them the pairs that
  // involve a flagged column; kMicaTables has no flags (null) and that kernel serves every pair
  if (path != kMicaTables && path != kMicaRefused) {
    hipLaunchKernelGGL(mica_ftable_kernel, dim3((unsigned)((A * A * T) / 256 + 1)), dim3(256), 0, stream, T, A, work.ftab, work.anyflag);
    classify(d_aln1, ld1, s1);
    if (!intra) classify(d_aln2, ld2, s2);
  }
  hipError_t e = hipSuccess;
  switch (path) {
    case kMicaTables: break;
    case kMicaWide: case kMicaWidePlain: case kMicaRefused: return hipErrorInvalidValue;
    case kMicaProtein4: e = launch_mica4(T, work, intra, d_mi, d_hj, ldo, stream); break;
    case kMicaDna4: e = launch_mica_dna4(T, work, intra, d_mi, d_hj, ldo, stream); break;
    case kMicaProtein8: {
      const unsigned ntx = (unsigned)((n2 + kMica3J - 1) / kMica3J), nty = (unsigned)((n1 + kMica3I - 1) / kMica3I);
      const unsigned ntiles = ntx * nty, per_xcd = (ntiles + 7) / 8;
      const size_t lds = mica_mfma3_lds_bytes(T, Tp);
      if ((e = mica_allow_lds(&mica_mfma3_kernel, lds)) != hipSuccess) break;
      hipLaunchKernelGGL(mica_mfma3_kernel, dim3(8 * per_xcd), dim3(512), lds, stream, T, Tp, s1.C, n1, s1.flag, s1.gap, s1.S, s2.C, n2,
                         s2.flag, s2.gap, s2.S, work.ftab, intra, d_mi, d_hj, ldo, ntx, ntiles, per_xcd);
      break;
    }
    case kMicaDna1: {
      dim3 grid((unsigned)((n2 + kMicaTileJ - 1) / kMicaTileJ), (unsigned)((n1 + kMicaTileI - 1) / kMicaTileI));
      hipLaunchKernelGGL(mica_mfma_kernel<4>, grid, dim3(512), mica_mfma_lds_bytes(T), stream, T, Tp, s1.H, n1, s1.flag, s1.gap, s1.S,
                         s2.H, n2, s2.flag, s2.gap, s2.S, work.ftab, intra, d_mi, d_hj, ldo);
      break;
    }
  }
  if (e != hipSuccess) return e;
  // the LDS-table kernel, then the column entropies
  const size_t ntiles = ((n2 + 15) / 16) * n1;
  auto tables = [&](auto columns, auto entropy) {
    hipLaunchKernelGGL(columns, dim3((unsigned)std::min<size_t>(ntiles, 8192)), dim3(64), sizeof(double) * A * A * 16, stream, T, d_masks,
                       d_aln1, n1, ld1, d_aln2, n2, ld2, intra, d_mi, d_hj, ldo, s1.flag, s2.flag, work.anyflag);
    if (d_h1) hipLaunchKernelGGL(entropy, dim3((unsigned)((n1 + 1) / 2)), dim3(64), 0, stream, T, d_masks, d_aln1, n1, ld1, d_h1);
    if (d_h2) hipLaunchKernelGGL(entropy, dim3((unsigned)((n2 + 1) / 2)), dim3(64), 0, stream, T, d_masks, d_aln2, n2, ld2, d_h2);
  };
  if (A == 20) tables(mi_columns_kernel<20>, column_entropy_kernel<20>); else tables(mi_columns_kernel<4>, column_entropy_kernel<4>);
  return hipGetLastError();
}

}  // namespace cmx
