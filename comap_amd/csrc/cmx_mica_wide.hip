// Mica column MI for alphabets other than 4 / 20 states (2 .. 64 states: codon models), CoMap/Mica.cpp:164-166, 349-361.
// There is no ambiguity table here: a code < A is that state -- 63 included, no code is reserved -- and every code >= A is an
// unknown, spread evenly over all states (SiteTools::*(.., resolveUnknowns = true): 1/A per state, 1/A^2 per cell of the joint
// table).  An unknown never gets a one-hot row: a taxon with an unknown in either column of a pair adds nothing to the matrix
// product, so 64 states are two row tiles, and the cross counts follow from the margins, exactly, in integers:
//   N_aU = cnt1[a] - sum_b N_ab,  N_Ub = cnt2[b] - sum_a N_ab,  N_UU = unk1 - sum_b N_Ub,
//   cell c_ab = m_ab / A^2 with the integer m_ab = A^2 N_ab + A (N_aU + N_Ub) + N_UU.
// Three stages: classification (symbol bytes, counts, column sums), the matrix-core kernel (up to 2 047 taxa), and a plain
// kernel -- one wave per pair, an integer table in LDS -- for listed pairs, longer columns and as the cross-check.
#include <algorithm>
#include <atomic>

#include "cmx_device.h"
#include "cmx_lanes.h"

namespace cmx {

static std::atomic<int> g_wide_plain{0};   // cmx_debug_mica_wide_plain
int mica_wide_plain(int on) {
  const int was = g_wide_plain.load();
  if (on >= 0) g_wide_plain.store(on ? 1 : 0);
  return was;
}

constexpr int kWideK = 32;        // taxa per MFMA step (v_mfma_i32_32x32x32_i8)
constexpr int kWideNone = 255;    // in the staged column: an unknown or the padding behind the last taxon (no one-hot row)
constexpr int kWideMaxTp = 2048;  // the matrix-core path serves T <= 2047 (16-bit counts in its epilogue, the c ln c table in LDS)

__device__ __forceinline__ double micaw_f(double c) { return c > 0.0 ? c * log(c) : 0.0; }
// totals over the wave, the same tree wherever the pair sits; every lane ends with the total
__device__ __forceinline__ double micaw_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int micaw_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- (a) classification, one workgroup per column: the column's one-hot row of each taxon C[col][Tp] (the state; an unknown
// and the padding behind taxon T - 1 have no row), the integer state counts cnt[col][A], the unknowns unk[col], gap[col] =
// has unknowns, S[col] = sum_a f(cnt_a + unk / A) in state order.  The one-hot rows themselves (32 or 64 per column) are
// never stored: the matrix-core kernel expands these bytes in LDS.
__global__ __launch_bounds__(256) void micaw_classify_kernel(int A, int T, int Tp, const uint8_t* __restrict__ aln, size_t ld,
                                                             uint8_t* __restrict__ C, int* __restrict__ cntg, int* __restrict__ unkg,
                                                             uint8_t* __restrict__ gap, double* __restrict__ S) {
  __shared__ int cnt[65];   // states, then the unknowns
  const size_t i = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < 65) cnt[tid] = 0;
  __syncthreads();
  for (int t = tid; t < Tp; t += 256) {
    unsigned c = kWideNone;
    if (t < T) {
      c = aln[(size_t)t * ld + i];
      if (c >= (unsigned)A) c = kWideNone;
      atomicAdd(&cnt[c < (unsigned)A ? (int)c : 64], 1);
    }
    C[i * (size_t)Tp + t] = (uint8_t)c;
  }
  __syncthreads();
  if (tid < A) cntg[i * (size_t)A + tid] = cnt[tid];
  if (tid == 0) {
    const double g = (double)cnt[64] / (double)A;
    double s = 0.0;
    for (int a = 0; a < A; ++a) s += micaw_f((double)cnt[a] + g);
    S[i] = s;
    unkg[i] = cnt[64];
    gap[i] = (uint8_t)(cnt[64] > 0 ? 1 : 0);
  }
}

// f[c] = c ln c for the integer counts 0 .. T, followed by f2[m] = f(m / A^2) for m = 0 .. A^2 T: the cells of a pair with
// unknowns (m_ab above), so that those pairs need no logarithm at run time either
__global__ void micaw_ftable_kernel(int T, int A, double* __restrict__ f) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= T) f[c] = c > 1 ? (double)c * log((double)c) : 0.0;
  if (c <= A * A * T) f[T + 1 + c] = micaw_f((double)c / (double)(A * A));
}
size_t micaw_ftab_entries(int A, int T) { return (size_t)(T + 1) + (size_t)A * A * T + 1; }

// ---- (b) the matrix-core kernel, modelled on mica_mfma_kernel and, for its operands, on mica3_tile: eight waves per
// workgroup, operand tiles (64 lanes x 16 B) through LDS once per workgroup.  A pair is RT x RT accumulator tiles; the
// workgroup takes 4 columns of the first alignment and 2 (RT = 2) or 4 (RT = 1) of the second, wave w column w / 2 of the
// first and the half w % 2 of the second: one pair of 64 registers, or two of 16.  Rows and columns >= A are structurally
// zero.  The operands are not read as one-hot matrices (64 rows x T bytes per column: 48 GB through the L2 for 2 000 x 2 000
// columns of 256 taxa, 8.4 ms where this form takes less): a column travels as its T symbol bytes, all columns of
// the tile in one round trip, and the loader threads expand them to one-hot operand tiles in LDS, two k-steps per barrier.
constexpr int kWideTI = 4;
constexpr int micaw_tile_j(int A) { return A > 32 ? 2 : 4; }
// bytes of one wave's slot in the epilogue of pairs with unknowns: the pair's table in 16-bit counts (row stride R + 2, so
// that a lane per row reads conflict-free), then N_aU and N_Ub
constexpr size_t micaw_slot_bytes(int R) { return (size_t)R * (R + 2) * 2 + 2 * 64 * sizeof(int); }
// what follows f[0 .. T] in LDS: the larger of four buffers of operand tiles and the eight waves' epilogue slots
constexpr size_t micaw_work_bytes(int RT) {
  return 4 * (size_t)(kWideTI * RT + 4) * 64 * sizeof(cmx_i4) > 8 * micaw_slot_bytes(32 * RT) ? 4 * (size_t)(kWideTI * RT + 4) * 64 * sizeof(cmx_i4)
                                                                                               : 8 * micaw_slot_bytes(32 * RT);
}
template <int RT>
__global__ __launch_bounds__(512, 4) void micaw_mfma_kernel(int A, int T, int Tp, const uint8_t* __restrict__ C1, size_t n1,
                                                            const int* __restrict__ cnt1, const int* __restrict__ unk1,
                                                            const uint8_t* __restrict__ gap1, const double* __restrict__ S1,
                                                            const uint8_t* __restrict__ C2, size_t n2,
                                                            const int* __restrict__ cnt2, const uint8_t* __restrict__ gap2,
                                                            const double* __restrict__ S2, const double* __restrict__ ftab_g,
                                                            int intra, double* __restrict__ mi, double* __restrict__ hj, size_t ldo,
                                                            unsigned ntx) {
  constexpr int R = 32 * RT, NJ = 2 / RT, TJ = 2 * NJ, NOP = kWideTI * RT + 4, LS = R + 2, NC = kWideTI + TJ;
  extern __shared__ __attribute__((aligned(16))) uint8_t micaw_smem[];
  double* ftab = reinterpret_cast<double*>(micaw_smem);                                                  // [T + 1]
  uint8_t* opsb = micaw_smem + (((size_t)(T + 1) * 8 + 15) & ~(size_t)15);
  cmx_i4* ops = reinterpret_cast<cmx_i4*>(opsb);                                                         // [4][NOP][64]
  uint8_t* codes = opsb + micaw_work_bytes(RT);                                                          // [NC][Tp]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
  const size_t i0 = (size_t)(blockIdx.x / ntx) * kWideTI, j0 = (size_t)(blockIdx.x % ntx) * TJ;
  if (intra && j0 + TJ <= i0 + 1) {   // no pair with j > i in this tile: only the NaN convention of the intra layout
    if (tid < kWideTI * TJ) {
      const size_t i = i0 + tid / TJ, j = j0 + tid % TJ;
      if (i < n1 && j < n2) {
        mi[i * ldo + j] = __builtin_nan("");
        hj[i * ldo + j] = __builtin_nan("");
      }
    }
    return;
  }
  // the tile's columns, one byte per taxon (clamped: a column past the end is the last one again, and nothing is written for it)
  const int chunks = Tp / 16;
  for (int e = tid; e < NC * chunks; e += 512) {
    const int c = e / chunks, o = e % chunks;
    const bool fi = c < kWideTI;
    const size_t want = fi ? i0 + c : j0 + (c - kWideTI), nc = fi ? n1 : n2;
    const size_t col = want < nc ? want : nc - 1;
    reinterpret_cast<cmx_i4*>(codes)[e] = *reinterpret_cast<const cmx_i4*>((fi ? C1 : C2) + col * (size_t)Tp + 16 * (size_t)o);
  }
  for (int c = tid; c <= T; c += 512) ftab[c] = ftab_g[c];
  const size_t i = i0 + wi, ic = i < n1 ? i : n1 - 1;
  size_t jc[NJ];
  unsigned gp[NJ];
  const unsigned g1 = gap1[ic];
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    const size_t j = j0 + NJ * wj + jj;
    jc[jj] = j < n2 ? j : n2 - 1;
    gp[jj] = g1 | gap2[jc[jj]];
  }
  // does any column of this tile carry unknowns?  (block-uniform: it decides a barrier)
  unsigned gapbits = 0;
#pragma unroll
  for (int c = 0; c < kWideTI; ++c) gapbits |= gap1[i0 + c < n1 ? i0 + c : n1 - 1];
#pragma unroll
  for (int c = 0; c < TJ; ++c) gapbits |= gap2[j0 + c < n2 ? j0 + c : n2 - 1];
  // loader role: NOP operand tiles x 64 lanes of 16 bytes, threads 0 .. 32 NOP - 1 take two each.  Operand tile q < 4 RT:
  // column q / RT of the first alignment's four, row tile q % RT; else qq = q - 4 RT: column qq / RT of the second's, row
  // tile qq % RT.  A lane's 16 bytes are row (lane % 32) of the row tile, taxa group (lane / 32): the thread's two lanes
  // share the 16 symbols and differ in the row.
  const bool loader = tid < NOP * 32;
  const int q = loader ? tid >> 5 : 0;
  const bool first = q < kWideTI * RT;
  const int qq = first ? q : q - kWideTI * RT;
  const int l0 = 2 * (tid & 31);
  const uint8_t* crow = codes + (size_t)((first ? 0 : kWideTI) + qq / RT) * Tp + 16 * (l0 >> 5);
  const unsigned srow = (unsigned)(32 * (qq % RT) + (l0 & 31)) * 0x01010101u;   // the first lane's state in the four bytes of a dword
  cmx_i16v acc[RT][2];
#pragma unroll
  for (int ii = 0; ii < RT; ++ii)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ii][c][v] = 0;
  __syncthreads();   // symbols and table are in LDS
  // two k-steps per barrier: four operand buffers, the pair being multiplied and the pair being expanded
  int buf = 0;
  for (int ks = 0; ks < Tp; ks += 2 * kWideK) {
    const bool two = ks + kWideK < Tp;
    if (loader) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 0 || two) {
          const cmx_i4 sy = *reinterpret_cast<const cmx_i4*>(crow + ks + h * kWideK);
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            cmx_i4 oh;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const unsigned x = (unsigned)sy[d] ^ (srow + (unsigned)u * 0x01010101u);
              const unsigned z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 where the byte of x is zero
              oh[d] = (int)(z >> 7);
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
        cmx_i4 a[RT], b[2];
#pragma unroll
        for (int ii = 0; ii < RT; ++ii) a[ii] = ops[((buf + h) * NOP + RT * wi + ii) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 2; ++c) b[c] = ops[((buf + h) * NOP + kWideTI * RT + 2 * wj + c) * 64 + lane];
#pragma unroll
        for (int ii = 0; ii < RT; ++ii)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[ii][c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ii], b[c], acc[ii][c], 0, 0, 0);
      }
    }
    buf ^= 2;
  }
  const double lnT = log((double)T), invT = 1.0 / (double)T;
  // pairs without unknowns: sum_ab f(N_ab) from the table, every lane its registers in register order, then the wave's tree --
  // the same order for every pair, whichever wave, tile or workgroup holds it.  Pair jj of the wave is the accumulator
  // tiles acc[.][jj RT .. jj RT + RT - 1].
  double s[NJ];
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    double x = 0.0;
#pragma unroll
    for (int ii = 0; ii < RT; ++ii)
#pragma unroll
      for (int c = 0; c < RT; ++c)
#pragma unroll
        for (int v = 0; v < 16; ++v) x += ftab[acc[ii][jj * RT + c][v]];
    s[jj] = micaw_wave_sum(x);
  }
  // pairs with an unknown in either column: the table goes to LDS (16-bit counts, T <= 2047), a lane per row / column takes
  // the sums, and f of every cell's m_ab / A^2 comes from the second table.  v_mfma_i32_32x32x32_i8 leaves D[row][col] in register v of lane l
  // with row = 8 (v / 4) + 4 (l / 32) + v % 4, col = l % 32.
  if (gapbits != 0) {
    __syncthreads();   // the operand buffers are free now: the waves' slots lie over them
    uint16_t* tab = reinterpret_cast<uint16_t*>(opsb + (size_t)w * micaw_slot_bytes(R));
    int* rU = reinterpret_cast<int*>(tab + R * LS);
    int* cU = rU + 64;
    const double* f2 = ftab_g + T + 1;   // f(m / A^2), global (A^2 T + 1 entries; the small m of the empty cells stay in the caches)
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      if (!gp[jj]) continue;   // wave-uniform
#pragma unroll
      for (int ii = 0; ii < RT; ++ii)
#pragma unroll
        for (int c = 0; c < RT; ++c)
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int row = 32 * ii + 8 * (v / 4) + 4 * (lane / 32) + v % 4, cl = 32 * c + lane % 32;
            tab[row * LS + cl] = (uint16_t)acc[ii][jj * RT + c][v];
          }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      int nau = 0, nub = 0;
      if (lane < A) {   // (A <= R: lane indexes a row and a column of the table)
        int rs = 0, cs = 0;
        for (int k = 0; k < A; ++k) {
          rs += (int)tab[lane * LS + k];
          cs += (int)tab[k * LS + lane];
        }
        nau = cnt1[ic * (size_t)A + lane] - rs;
        nub = cnt2[jc[jj] * (size_t)A + lane] - cs;
      }
      rU[lane] = nau;
      cU[lane] = nub;
      const int nuu = unk1[ic] - micaw_wave_sum(nub);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      // cells in row order, column = lane % R (64 / R rows per step); a lane adds its cells top down
      double sg = 0.0;
      const int b = lane % R;
#pragma unroll 4
      for (int a = lane / R; a < A; a += 64 / R) {
        if (b < A) {
          const int m = A * A * (int)tab[a * LS + b] + A * (rU[a] + cU[b]) + nuu;
          sg += f2[m];
        }
      }
      s[jj] = micaw_wave_sum(sg);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();   // the slot is free for the wave's next pair
    }
  }
  if (lane == 0 && i < n1) {
    const double s1 = S1[ic];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const size_t j = j0 + NJ * wj + jj;
      if (j < n2) {
        const bool valid = !intra || j > i;
        mi[i * ldo + j] = valid ? lnT + (s[jj] - s1 - S2[j]) * invT : __builtin_nan("");
        hj[i * ldo + j] = valid ? lnT - s[jj] * invT : __builtin_nan("");
      }
    }
  }
}
// micaw_smem: f[0 .. T], the operand buffers / epilogue slots, the tile's 6 or 8 symbol columns
static size_t micaw_mfma_lds_bytes(int T, int Tp, int RT) {
  return (((size_t)(T + 1) * 8 + 15) & ~(size_t)15) + micaw_work_bytes(RT) + (size_t)(kWideTI + 4 / RT) * Tp;
}
size_t micaw_tiles(int A, size_t n1, size_t n2) {
  const size_t tj = (size_t)micaw_tile_j(A);
  return ((n1 + kWideTI - 1) / kWideTI) * ((n2 + tj - 1) / tj);
}

// ---- (c) the plain kernel: one wave per pair, the A x A joint table as int32 in LDS, filled with integer LDS atomics;
// margins and unknowns are counted in the same pass.  Integer counts and a fixed cell order: the same bits every time.
// idx1 != null: the listed pairs (idx1[p], idx2[p]) -> mi[p]; else pair p = (p / n2, p % n2) of the rectangle (intra: j > i,
// NaN elsewhere) -> mi[i ldo + j].
__global__ __launch_bounds__(64) void micaw_plain_kernel(int A, int T, const uint8_t* __restrict__ aln1, size_t ld1,
                                                         const uint8_t* __restrict__ aln2, size_t ld2,
                                                         const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2,
                                                         size_t n2, int intra, size_t npairs, double* __restrict__ mi,
                                                         double* __restrict__ hj, size_t ldo) {
  extern __shared__ int micaw_tab[];   // [A * A] N_ab, then [64] each N_aU, N_Ub, cnt1, cnt2, then N_UU, unk1, unk2
  int* rU = micaw_tab + A * A;
  int *cU = rU + 64, *c1 = rU + 128, *c2 = rU + 192, *misc = rU + 256;
  const int lane = threadIdx.x;
  const int W = A <= 32 ? 32 : 64;   // cells of a row per step
  const double lnT = log((double)T), invT = 1.0 / (double)T, A2 = (double)(A * A);
  for (size_t p = blockIdx.x; p < npairs; p += gridDim.x) {
    size_t i, j, o;
    if (idx1) {
      i = (size_t)idx1[p];
      j = (size_t)idx2[p];
      o = p;
    } else {
      i = p / n2;
      j = p % n2;
      o = i * ldo + j;
      if (intra && j <= i) {
        if (lane == 0) {
          mi[o] = __builtin_nan("");
          hj[o] = __builtin_nan("");
        }
        continue;
      }
    }
    __syncthreads();   // the previous pair's readers are done with the table
    for (int k = lane; k < A * A + 260; k += 64) micaw_tab[k] = 0;
    __syncthreads();
    for (int t = lane; t < T; t += 64) {
      const unsigned x = aln1[(size_t)t * ld1 + i], y = aln2[(size_t)t * ld2 + j];
      const bool kx = x < (unsigned)A, ky = y < (unsigned)A;
      atomicAdd(kx ? &c1[x] : &misc[1], 1);
      atomicAdd(ky ? &c2[y] : &misc[2], 1);
      atomicAdd(kx ? (ky ? &micaw_tab[x * A + y] : &rU[x]) : (ky ? &cU[y] : &misc[0]), 1);
    }
    __syncthreads();
    // column sums S = sum_a f(cnt_a + unk / A): a state per lane, added in state order
    const double t1 = lane < A ? micaw_f((double)c1[lane] + (double)misc[1] / (double)A) : 0.0;
    const double t2 = lane < A ? micaw_f((double)c2[lane] + (double)misc[2] / (double)A) : 0.0;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < A; ++k) {
      s1 += __shfl(t1, k, 64);
      s2 += __shfl(t2, k, 64);
    }
    // cells in row order, column = lane % W; a lane adds its cells top down, then the wave's tree
    double sg = 0.0;
    const int b = lane % W;
    const long long nuu = misc[0];
    for (int a = lane / W; a < A; a += 64 / W) {
      if (b < A) {
        const long long m = (long long)A * A * micaw_tab[a * A + b] + (long long)A * (rU[a] + cU[b]) + nuu;
        sg += micaw_f((double)m / A2);
      }
    }
    const double s = micaw_wave_sum(sg);
    if (lane == 0) {
      mi[o] = lnT + (s - s1 - s2) * invT;
      hj[o] = lnT - s * invT;
    }
  }
}
static size_t micaw_plain_lds_bytes(int A) { return ((size_t)A * A + 260) * sizeof(int); }

// ---- (d) column entropies, h = -sum_a p_a ln p_a with p_a = (cnt_a + unk / A) / T in state order, from the counts of the
// classification; where that does not run (the plain path) a wave counts a column first
__global__ __launch_bounds__(64) void micaw_count_kernel(int A, int T, const uint8_t* __restrict__ aln, size_t ld, size_t n,
                                                         int* __restrict__ cntg, int* __restrict__ unkg) {
  __shared__ int cnt[65];
  const int lane = threadIdx.x;
  for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
    __syncthreads();
    cnt[lane] = 0;
    if (lane == 0) cnt[64] = 0;
    __syncthreads();
    for (int t = lane; t < T; t += 64) {
      const unsigned c = aln[(size_t)t * ld + i];
      atomicAdd(&cnt[c < (unsigned)A ? (int)c : 64], 1);
    }
    __syncthreads();
    if (lane < A) cntg[i * (size_t)A + lane] = cnt[lane];
    if (lane == 0) unkg[i] = cnt[64];
  }
}
__global__ __launch_bounds__(256) void micaw_entropy_kernel(int A, int T, const int* __restrict__ cntg, const int* __restrict__ unkg,
                                                            size_t n, double* __restrict__ h) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double g = (double)unkg[i] / (double)A;
  double s = 0.0;
  for (int a = 0; a < A; ++a) {
    const double c = (double)cntg[i * (size_t)A + a] + g;
    if (c > 0.0) {
      const double pr = c / (double)T;
      s -= pr * log(pr);
    }
  }
  h[i] = s;
}

static unsigned micaw_grid(size_t want, size_t cap) { return (unsigned)std::min(want, cap); }

hipError_t launch_mi_pairs_wide(int A, int T, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2, size_t ld2,
                                const int64_t* d_idx1, const int64_t* d_idx2, size_t npairs, double* d_mi, double* d_hj,
                                hipStream_t stream) {
  if (A < 2 || A > 64 || !d_idx1 || !d_idx2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(micaw_plain_kernel, dim3(micaw_grid(npairs, (size_t)1 << 20)), dim3(64), micaw_plain_lds_bytes(A), stream, A, T,
                     d_aln1, ld1, d_aln2, ld2, d_idx1, d_idx2, (size_t)0, 0, npairs, d_mi, d_hj, (size_t)0);
  return hipGetLastError();
}

hipError_t launch_mi_columns_wide(int A, int T, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2, size_t ld2, int intra,
                                  double* d_mi, double* d_hj, size_t ldo, double* d_h1, double* d_h2, const MicaWork& work,
                                  hipStream_t stream) {
  if (A < 2 || A > 64) return hipErrorInvalidValue;
  const MicaSide &s1 = work.s[0], &s2 = work.s[1];
  const size_t n1 = s1.n, n2 = s2.n;
  const MicaPath path = mica_path(A, T, n1, n2);
  if (path == kMicaWide) {
    const int Tp = work.Tp, RT = A > 32 ? 2 : 1;
    if (Tp > kWideMaxTp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(micaw_ftable_kernel, dim3((unsigned)((A * A * T) / 256 + 1)), dim3(256), 0, stream, T, A, work.ftab);
    auto classify = [&](const uint8_t* aln, size_t ld, const MicaSide& s) {
      hipLaunchKernelGGL(micaw_classify_kernel, dim3((unsigned)s.n), dim3(256), 0, stream, A, T, Tp, aln, ld, s.C, s.cnt, s.unk,
                         s.gap, s.S);
    };
    classify(d_aln1, ld1, s1);
    if (!intra) classify(d_aln2, ld2, s2);
    const unsigned ntx = (unsigned)((n2 + micaw_tile_j(A) - 1) / micaw_tile_j(A));
    const size_t lds = micaw_mfma_lds_bytes(T, Tp, RT);
    auto launch = [&](auto kernel) {
      const hipError_t e = mica_allow_lds(kernel, lds);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kernel, dim3((unsigned)micaw_tiles(A, n1, n2)), dim3(512), lds, stream, A, T, Tp, s1.C, n1, s1.cnt, s1.unk, s1.gap,
                         s1.S, s2.C, n2, s2.cnt, s2.gap, s2.S, work.ftab, intra, d_mi, d_hj, ldo, ntx);
      return hipSuccess;
    };
    const hipError_t e = RT == 2 ? launch(&micaw_mfma_kernel<2>) : launch(&micaw_mfma_kernel<1>);
    if (e != hipSuccess) return e;
  } else if (path == kMicaWidePlain) {
    auto count = [&](const uint8_t* aln, size_t ld, const MicaSide& s) {
      hipLaunchKernelGGL(micaw_count_kernel, dim3(micaw_grid(s.n, (size_t)1 << 20)), dim3(64), 0, stream, A, T, aln, ld, s.n, s.cnt, s.unk);
    };
    if (d_h1 || (intra && d_h2)) count(d_aln1, ld1, s1);
    if (!intra && d_h2) count(d_aln2, ld2, s2);
    hipLaunchKernelGGL(micaw_plain_kernel, dim3(micaw_grid(n1 * n2, (size_t)1 << 20)), dim3(64), micaw_plain_lds_bytes(A), stream, A, T,
                       d_aln1, ld1, d_aln2, ld2, (const int64_t*)nullptr, (const int64_t*)nullptr, n2, intra, n1 * n2, d_mi, d_hj, ldo);
  } else {
    return hipErrorInvalidValue;
  }
  if (d_h1) hipLaunchKernelGGL(micaw_entropy_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, stream, A, T, s1.cnt, s1.unk, n1, d_h1);
  if (d_h2) hipLaunchKernelGGL(micaw_entropy_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, stream, A, T, s2.cnt, s2.unk, n2, d_h2);
  return hipGetLastError();
}

}  // namespace cmx
