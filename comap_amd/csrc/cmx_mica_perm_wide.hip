// Mica's permutation test (miTest, CoMap/Mica.cpp:93-118) for alphabets other than 4 / 20 states (2 .. 64: codon models).
// The scheme and its shared pieces are in cmx_mica_perm.h, here specialised to the alphabet rule of cmx_mica_wide.hip: a code
// < A is that state (63 included), every code >= A is THE unknown, there is no mask table.  What differs from the 4 / 20
// kernels (cmx_mica_perm.hip):
//  * classification is a wave per column (64 counters do not fit a thread's registers) and leaves, per column, the end of
//    every state's run in the visiting order (unknowns first, then the states ascending, stable), the unknowns, two flags and
//    the visiting order itself;
//  * the resolved kernel keeps no A x A table: the observed sum comes from the same incremental evaluation as a shuffle's,
//    the states of column i dealt over the pair's lanes, with column j read through column i's visiting order;
//  * the unknowns' kernel stores one row per lane, N_Uy (there is one non-state code), and sums
//    F_g[A (A N_ay + N_aU) + A N_Uy + N_UU] over y as soon as state a is done; rows of states that column i does not hold
//    are sum_y F_g[A N_Uy + N_UU] each, computed once per shuffle.  (m_ab = A^2 N_ab + A (N_aU + N_Ub) + N_UU, the table of
//    micaw_mfma_kernel; m <= A^2 T <= 8.4 M.)  F_g is read from global memory.
// No grid here is computed from a pair or tile count: every kernel walks its columns / pairs with a 64-bit stride loop.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cmx_device.h"
#include "cmx_mica_perm.h"

namespace cmx {

namespace {

constexpr int kPermwSeg = 128;        // bytes of a pair's run ends in LDS (64 states x 16 bits)

constexpr unsigned kPermwUnknown = 1, kPermwConstant = 2;   // flag bits of a column

// ---- classification, one wave per column.  end[i][x]: where state x's run ends in column i's visiting order (its start is
// end[i][x - 1], or unk[i] for x = 0); flag: has unknowns | at most one distinct state (SiteTools::isConstant(site,
// ignoreUnknown = true); an all-unknown column is one); order[i][pos] = taxon at position pos.  The stable placement keeps
// the next free position of state x in lane x and of the unknowns in a wave-uniform register.
__global__ __launch_bounds__(64) void permw_classify_kernel(int A, int T, const uint8_t* __restrict__ aln, size_t ld, size_t n,
                                                            uint16_t* __restrict__ endg, uint16_t* __restrict__ unkg,
                                                            uint8_t* __restrict__ flag, uint16_t* __restrict__ order,
                                                            int* __restrict__ any) {
  __shared__ int cnt[65];   // states, then the unknowns
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
    const int unk = cnt[64];
    const int mine = lane < A ? cnt[lane] : 0;
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    int st = unk + incl - mine;   // next free position of state `lane`
    int su = 0;                   // ... of the unknowns
    if (lane < A) endg[i * (size_t)A + lane] = (uint16_t)(unk + incl);
    const int nz = __popcll(__ballot(mine > 0));
    if (lane == 0) {
      unkg[i] = (uint16_t)unk;
      flag[i] = (uint8_t)((unk > 0 ? kPermwUnknown : 0u) | (nz <= 1 ? kPermwConstant : 0u));
      if (unk > 0) *any = 1;
    }
    for (int t0 = 0; t0 < T; t0 += 64) {
      const int t = t0 + lane;
      const bool live = t < T;
      int b = -1;
      if (live) {
        const unsigned c = aln[(size_t)t * ld + i];
        b = c < (unsigned)A ? (int)c : 64;
      }
      unsigned long long todo = __ballot(live);
      int pos = 0;
      while (todo) {   // one distinct symbol of these 64 taxa per turn, lanes in taxon order
        const int bl = __shfl(b, __ffsll((long long)todo) - 1, 64);
        const unsigned long long m = __ballot(b == bl);
        const int base = bl == 64 ? su : __shfl(st, bl & 63, 64);
        if (b == bl) pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (bl == 64) su += __popcll(m);
        else if (lane == bl) st += __popcll(m);
        todo &= ~m;
      }
      if (live) order[i * (size_t)T + pos] = (uint16_t)t;
    }
  }
}

// bytes per lane of 16-bit counters cleared with 64-bit stores (an odd number of 8-byte chunks: the 16 lanes of a
// ds_write_b64 group fall on 16 different bank pairs)
inline int permw_cstride(int counters) { int c8 = (counters * 2 + 7) / 8; if (c8 % 2 == 0) ++c8; return 8 * c8; }

__device__ __forceinline__ void permw_clear(uint16_t* cnt, int chunks) {
  for (int c = 0; c < chunks; ++c) reinterpret_cast<unsigned long long*>(cnt)[c] = 0ull;
}

struct PermwArgs {
  const uint8_t* aln; int T; size_t n, ld; int A;
  const uint16_t* end;       // [n][A]
  const uint16_t* unk;       // [n]
  const uint16_t* order;     // [n][T]
  const uint8_t* flag;       // [n]
  const long long* dF;       // [T]: F[c+1] - F[c], F[c] = round(c ln c 2^40)   (resolved pairs)
  const long long* F;        // [A^2 T + 1]: round(m ln m 2^sh)                (pairs with unknowns)
  uint32_t max_perm; uint64_t seed;
  size_t pair_begin, pair_end;
  double* pvalue; int32_t* nperm;   // indexed by pair - pair_begin
  int qstride, cstride, wave_bytes;
  uint32_t first;            // shuffles already done by the opening pass (0 if it was skipped)
};

// ---- resolved pairs.  G = 4: the opening pass (four pairs per wave, 16 shuffles each; an undecided pair leaves nperm =
// -1 - hits); G = 1: one pair per wave, 64 shuffles per round, from shuffle a.first on.  Per pair in LDS: the run ends of
// column i and column j in taxon order; per lane: its copy of column j and A 16-bit counters, cleared for every state of
// column i that occurs.
template <int G>
__global__ void permw_kernel(PermwArgs a) {
  constexpr int LPG = 64 / G;
  extern __shared__ __attribute__((aligned(16))) uint8_t permw_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int grp = lane / LPG, gl = lane % LPG;
  const int T = a.T, A = a.A, Tr8 = (T + 7) & ~7, clr = (A * 2 + 7) / 8;
  long long* dF = reinterpret_cast<long long*>(permw_smem);                       // [T] block-shared
  uint8_t* wbase = permw_smem + (((size_t)T * 8 + 15) & ~(size_t)15) + (size_t)wave * a.wave_bytes;
  const int gbytes = kPermwSeg + Tr8;
  uint16_t* seg = reinterpret_cast<uint16_t*>(wbase + (size_t)grp * gbytes);      // [A] end of state x in column i's order
  uint8_t* qbase = wbase + (size_t)grp * gbytes + kPermwSeg;                      // [T] column j
  uint8_t* priv = wbase + (size_t)G * gbytes;
  uint8_t* q = priv + (size_t)lane * a.qstride;
  uint16_t* cnt = reinterpret_cast<uint16_t*>(priv + (size_t)64 * a.qstride + (size_t)lane * a.cstride);
  for (int c = threadIdx.x; c < T; c += blockDim.x) dF[c] = a.dF[c];
  __syncthreads();
  const size_t n = a.n;
  for (size_t pb = a.pair_begin + ((size_t)blockIdx.x * nwaves + wave) * G; pb < a.pair_end; pb += (size_t)gridDim.x * nwaves * G) {
    const bool exists = pb + grp < a.pair_end;
    const size_t p = exists ? pb + grp : a.pair_end - 1;
    uint32_t done = 0, count = 0;
    bool open = exists;
    if (G == 1) {                      // second pass: only what the opening pass left undecided
      const int st = a.nperm[p - a.pair_begin];
      if (st >= 0) continue;
      count = (uint32_t)(-1 - st);
      done = a.first;
    }
    size_t i, j;
    perm_pair_of(p, n, &i, &j);
    const unsigned fl = (unsigned)a.flag[i] | (unsigned)a.flag[j];
    if (fl & kPermwUnknown) {          // decided by permw_general_kernel: nothing is written for it here
      open = false;
      if (G == 1) continue;
    } else if (fl & kPermwConstant) {  // Mica.cpp:100-104
      if (open && gl == 0) { a.pvalue[p - a.pair_begin] = 1.0; a.nperm[p - a.pair_begin] = 0; }
      open = false;
      if (G == 1) continue;
    }
    __builtin_amdgcn_wave_barrier();   // the previous pair's readers are done with seg and qbase
    if (open) {
      for (int x = gl; x < A; x += LPG) seg[x] = a.end[i * (size_t)A + x];
      for (int t = gl; t < T; t += LPG) qbase[t] = a.aln[(size_t)t * a.ld + j];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // the observed sum: the pair's lanes share the states of column i; a lane walks the run of its state in column i's
    // visiting order and counts column j's symbols there
    long long sobs = 0;
    if (open) {
      for (int x = gl; x < A; x += LPG) {
        const int beg = x ? (int)seg[x - 1] : 0, end = seg[x];
        if (beg == end) continue;
        permw_clear(cnt, clr);
        for (int t = beg; t < end; ++t) {
          const int y = a.aln[(size_t)a.order[i * (size_t)T + t] * a.ld + j];
          const int c = cnt[y];
          sobs += dF[c];
          cnt[y] = (uint16_t)(c + 1);
        }
      }
    }
    for (int off = LPG / 2; off; off >>= 1) sobs += __shfl_xor(sobs, off, 64);
    bool stop = false;
    do {
      const uint32_t k = done + (uint32_t)gl;
      bool hit = false;
      if (open) {
        for (int t = 0; t < T; t += 4) *reinterpret_cast<uint32_t*>(q + t) = *reinterpret_cast<const uint32_t*>(qbase + t);
        long long s = 0;
        uint32_t r[4] = {0, 0, 0, 0};
        int t = 0;
        for (int x = 0; x < A; ++x) {    // the states of column i that occur (uniform within the pair's lanes)
          const int end = seg[x];
          if (t >= end) continue;
          permw_clear(cnt, clr);
          for (; t < end; ++t) {
            if ((t & 3) == 0) perm_philox4(a.seed, (uint32_t)p, (uint32_t)((uint64_t)p >> 32), k, 0x50000000u | (uint32_t)(t >> 2), r);
            const int jj = t + (int)__umulhi(r[t & 3], (uint32_t)(T - t));
            const uint8_t vj = q[jj], vt = q[t];
            q[jj] = vt;                  // q[t] itself is not read again
            const int c = cnt[vj];
            s += dF[c];
            cnt[vj] = (uint16_t)(c + 1);
          }
        }
        hit = k < a.max_perm && s >= sobs;
      }
      const unsigned long long mw = __ballot(hit);
      const unsigned long long m = G == 1 ? mw : (mw >> (grp * LPG)) & ((1ull << LPG) - 1ull);
      stop = perm_stop(m, min((uint32_t)LPG, a.max_perm - done), done, count);
    } while (G == 1 && !stop && done < a.max_perm);
    if (open && gl == 0) perm_write(a, p, stop, done, count);
  }
}

// ---- pairs with an unknown in either column: one wave per pair, one lane per shuffle.  qbase is column j carried along
// column i's visiting order, its unknowns as code A; a lane keeps A + 1 counters (column j's symbols against the current
// symbol of column i) and the row N_Uy.  The observed value is the same evaluation without a shuffle.
template <bool SHUF>
__device__ __forceinline__ long long permw_general_eval(const PermwArgs& a, const uint8_t* qbase, uint8_t* q, uint16_t* cnt,
                                                        uint16_t* nu, const uint16_t* seg, int unk_i, size_t p, uint32_t k) {
  const int T = a.T, A = a.A, clr = ((A + 1) * 2 + 7) / 8;
  const long long* __restrict__ F = a.F;
  for (int t = 0; t < T; t += 4) *reinterpret_cast<uint32_t*>(q + t) = *reinterpret_cast<const uint32_t*>(qbase + t);
  permw_clear(cnt, clr);
  uint32_t r[4] = {0, 0, 0, 0};
  int t = 0;
  auto walk = [&](int end) {
    for (; t < end; ++t) {
      uint8_t vj;
      if (SHUF) {
        if ((t & 3) == 0) perm_philox4(a.seed, (uint32_t)p, (uint32_t)((uint64_t)p >> 32), k, 0x50000000u | (uint32_t)(t >> 2), r);
        const int jj = t + (int)__umulhi(r[t & 3], (uint32_t)(T - t));
        vj = q[jj];
        q[jj] = q[t];
      } else {
        vj = q[t];
      }
      cnt[vj] = (uint16_t)(cnt[vj] + 1);
    }
  };
  long long s = 0, su = 0;
  uint32_t nuu = 0;
  if (unk_i > 0) {                       // the unknowns of column i: the stored row, and what a row without a state is worth
    walk(unk_i);
    nuu = cnt[A];
#pragma unroll 4
    for (int y = 0; y < A; ++y) {
      const uint32_t c = cnt[y];
      nu[y] = (uint16_t)c;
      su += F[(uint32_t)A * c + nuu];
    }
    permw_clear(cnt, clr);
  }
  int nocc = 0;
  for (int x = 0; x < A; ++x) {          // the states of column i that occur (wave-uniform)
    const int end = seg[x];
    if (t >= end) continue;
    ++nocc;
    walk(end);
    const uint32_t nau = cnt[A];
    if (unk_i > 0) {
#pragma unroll 4
      for (int y = 0; y < A; ++y) s += F[(uint32_t)A * ((uint32_t)A * cnt[y] + nau + nu[y]) + nuu];
    } else {
#pragma unroll 4
      for (int y = 0; y < A; ++y) s += F[(uint32_t)A * ((uint32_t)A * cnt[y] + nau)];
    }
    permw_clear(cnt, clr);
  }
  return s + (long long)(A - nocc) * su;
}

__global__ void permw_general_kernel(PermwArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t permw_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int T = a.T, A = a.A, Tr8 = (T + 7) & ~7;
  uint8_t* wbase = permw_smem + (size_t)wave * a.wave_bytes;
  uint16_t* seg = reinterpret_cast<uint16_t*>(wbase);                // [A] run ends of column i
  uint8_t* qbase = wbase + kPermwSeg;                                // [T] column j in column i's visiting order
  uint8_t* priv = wbase + kPermwSeg + Tr8;
  uint8_t* q = priv + (size_t)lane * a.qstride;
  uint16_t* cnt = reinterpret_cast<uint16_t*>(priv + (size_t)64 * a.qstride + (size_t)lane * a.cstride);
  uint16_t* nu = reinterpret_cast<uint16_t*>(priv + (size_t)64 * a.qstride + (size_t)64 * a.cstride + (size_t)lane * a.cstride);
  const size_t n = a.n;
  for (size_t p = a.pair_begin + (size_t)blockIdx.x * nwaves + wave; p < a.pair_end; p += (size_t)gridDim.x * nwaves) {
    size_t i, j;
    perm_pair_of(p, n, &i, &j);
    const unsigned fl = (unsigned)a.flag[i] | (unsigned)a.flag[j];
    if (!(fl & kPermwUnknown)) continue;             // fully resolved pair: permw_kernel
    if (fl & kPermwConstant) {                       // Mica.cpp:100-104
      if (lane == 0) { a.pvalue[p - a.pair_begin] = 1.0; a.nperm[p - a.pair_begin] = 0; }
      continue;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < A) seg[lane] = a.end[i * (size_t)A + lane];
    for (int t = lane; t < T; t += 64) qbase[t] = (uint8_t)min((int)a.aln[(size_t)a.order[i * (size_t)T + t] * a.ld + j], A);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const int unk_i = a.unk[i];
    const long long sobs = permw_general_eval<false>(a, qbase, q, cnt, nu, seg, unk_i, p, 0);
    uint32_t done = 0, count = 0;
    bool stop = false;
    do {
      const uint32_t k = done + (uint32_t)lane;
      const long long s = permw_general_eval<true>(a, qbase, q, cnt, nu, seg, unk_i, p, k);
      const bool hit = k < a.max_perm && s >= sobs;
      stop = perm_stop(__ballot(hit), min(64u, a.max_perm - done), done, count);
    } while (!stop && done < a.max_perm);
    if (lane == 0) perm_write(a, p, stop, done, count);
  }
}

// LDS of one wave: the resolved kernel with G pairs per wave, the unknowns' kernel.  2 047 taxa x 64 states, the largest
// shape, in bytes -- resolved, one pair per wave: 16 384 (dF) + 128 + 2 048 + 64 x 2 052 + 64 x 136 = 158 592; with unknowns:
// 128 + 2 048 + 64 x 2 052 + 2 x 64 x 136 = 150 912; both below 163 840, so there is no smaller limit for either path.  The
// opening pass (G = 4) adds three more columns and run ends: it fits up to 2 028 taxa.
size_t permw_wave_bytes(int T, int A, int G) {
  return ((size_t)G * (kPermwSeg + ((T + 7) & ~7)) + 64 * (size_t)perm_qstride(T) + 64 * (size_t)permw_cstride(A) + 15) & ~(size_t)15;
}
size_t permw_general_wave_bytes(int T, int A) {
  return ((size_t)kPermwSeg + ((T + 7) & ~7) + 64 * (size_t)perm_qstride(T) + 2 * 64 * (size_t)permw_cstride(A + 1) + 15) & ~(size_t)15;
}
size_t permw_dF_bytes(int T) { return ((size_t)T * 8 + 15) & ~(size_t)15; }

}  // namespace

hipError_t launch_mica_permw_classify(int A, int T, const uint8_t* d_aln, size_t ld, size_t n, uint16_t* d_end, uint16_t* d_unk,
                                      uint8_t* d_flag, uint16_t* d_order, int* d_any, hipStream_t stream) {
  if (A < 2 || A > 64 || T < 2 || T > kPermMaxTaxa) return hipErrorInvalidValue;
  hipLaunchKernelGGL(permw_classify_kernel, dim3((unsigned)std::min<size_t>(n, (size_t)1 << 20)), dim3(64), 0, stream, A, T, d_aln, ld, n,
                     d_end, d_unk, d_flag, d_order, d_any);
  return hipGetLastError();
}

// d_F != null: some column has unknowns.  Order: (nperm = -1 where no opening pass runs) -> pairs with unknowns -> the
// opening pass -> one pair per wave for what is still undecided.
hipError_t launch_mica_permw(int A, int T, const uint8_t* d_aln, size_t ld, size_t n, const uint16_t* d_end, const uint16_t* d_unk,
                             const uint8_t* d_flag, const uint16_t* d_order, const long long* d_dF, const long long* d_F,
                             uint32_t max_perm, uint64_t seed, size_t pair_begin, size_t pair_end, double* d_pvalue, int32_t* d_nperm,
                             int cu_count, hipStream_t stream) {
  if (A < 2 || A > 64 || T < 2 || T > kPermMaxTaxa || pair_end <= pair_begin) return hipErrorInvalidValue;
  PermwArgs a{};
  a.aln = d_aln; a.T = T; a.n = n; a.ld = ld; a.A = A; a.end = d_end; a.unk = d_unk; a.order = d_order; a.flag = d_flag;
  a.dF = d_dF; a.F = d_F; a.max_perm = max_perm; a.seed = seed; a.pair_begin = pair_begin; a.pair_end = pair_end;
  a.pvalue = d_pvalue; a.nperm = d_nperm;
  a.qstride = perm_qstride(T);
  const size_t npairs = pair_end - pair_begin;
  const bool opening = permw_dF_bytes(T) + permw_wave_bytes(T, A, 4) <= kPermLdsLimit;
  hipError_t e;
  if (!opening && (e = hipMemsetAsync(d_nperm, 0xFF, sizeof(int32_t) * npairs, stream)) != hipSuccess) return e;   // -1: undecided, no hits
  if (d_F) {
    a.cstride = permw_cstride(A + 1);
    if ((e = perm_launch(&permw_general_kernel, a, 0, permw_general_wave_bytes(T, A), 1, npairs, cu_count, stream)) != hipSuccess) return e;
  }
  a.cstride = permw_cstride(A);
  a.first = opening ? kPermFirst : 0;
  if (opening && (e = perm_launch(&permw_kernel<4>, a, permw_dF_bytes(T), permw_wave_bytes(T, A, 4), 4, npairs, cu_count, stream)) != hipSuccess) return e;
  return perm_launch(&permw_kernel<1>, a, permw_dF_bytes(T), permw_wave_bytes(T, A, 1), 1, npairs, cu_count, stream);
}

}  // namespace cmx
