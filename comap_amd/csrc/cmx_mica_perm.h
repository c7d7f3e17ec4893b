// What the two families of Mica's permutation test (miTest, CoMap/Mica.cpp:93-118) share: cmx_mica_perm.hip (4 / 20 states,
// a mask table) and cmx_mica_perm_wide.hip (2 .. 64 states, one unknown).  The scheme, once:
//  * shuffling both columns or one is the same distribution of joint tables; H1 and H2 do not change under a shuffle,
//    so "rep >= mi" is "sum_xy f(c_xy) of the shuffle >= the observed one", f(c) = c ln c.  That sum is kept in fixed
//    point (F[c] = round(c ln c * 2^40), int64), so it is exact and order-free: tables with the same counts tie
//    exactly, on any device and in the CPU restatement (the reference's own floating-point sums decide such ties by
//    rounding noise);
//  * one wave per pair, one LANE per permutation: 64 shuffles of the same pair run side by side, each lane with its
//    own copy of column j in LDS (forward Fisher-Yates from the counter RNG: Philox4x32-10, key = seed, counter =
//    (pair, pair >> 32, permutation, 'P' << 24 | position / 4)) and 16-bit counters for the current state of column i
//    -- positions are taken in the order of column i's states, so only the counts of the current state are live, and
//    the sum is accumulated from the increments (F[c+1] - F[c]), no pass over the A x A table;
//  * the sequential stopping rule is applied to the 64 results in order (ballot + popcount);
//  * an opening pass of kPermFirst shuffles for four pairs per wave where its four column copies fit the LDS: half of
//    all pairs between unrelated columns collect their 5 hits there, and a whole wave per pair would run 64.  A pair
//    that is not decided yet leaves nperm = -1 - hits; the one-pair-per-wave pass picks those up at shuffle kPermFirst.
//    Shuffle k of a pair is the same in either pass: the result does not depend on the split.
// The LDS layouts and counter strides are each family's own, stated beside the kernel that carves the LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cmx_device.h"

namespace cmx {

constexpr int kPermMaxTaxa = 2047;   // 16-bit positions and counts; the private column copies of 64 lanes in LDS
inline int mica_perm_max_taxa() { return kPermMaxTaxa; }
constexpr int kPermFirst = 16;       // shuffles of the opening pass
// waves per workgroup are planned within kPermLdsPlan, workgroups per CU and every refusal by kPermLdsLimit
constexpr size_t kPermLdsPlan = 150 * 1024, kPermLdsLimit = 160 * 1024;

// bytes per lane of the private column copy: an odd number of words (LDS banks)
inline int perm_qstride(int T) { int sd = (T + 3) / 4; if (sd % 2 == 0) ++sd; return 4 * sd; }

__device__ __forceinline__ void perm_philox4(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t (&out)[4]) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// (i, j) of pair p in row-major (i < j) order: p = i n - i (i + 1) / 2 + (j - i - 1)
__device__ __forceinline__ void perm_pair_of(size_t p, size_t n, size_t* pi, size_t* pj) {
  size_t i = (size_t)((2.0 * n - 1.0 - sqrt((2.0 * n - 1.0) * (2.0 * n - 1.0) - 8.0 * (double)p)) / 2.0);
  while (i > 0 && i * n - i * (i + 1) / 2 > p) --i;
  while ((i + 1) * n - (i + 1) * (i + 2) / 2 <= p) ++i;
  *pi = i;
  *pj = p - (i * n - i * (i + 1) / 2) + i + 1;
}

// the sequential stopping rule on the results of `avail` shuffles done side by side (bit l of m: shuffle done + l reached the
// observed value): the (5 - count)-th hit ends the test
__device__ __forceinline__ bool perm_stop(unsigned long long m, uint32_t avail, uint32_t& done, uint32_t& count) {
  const int need = 5 - (int)count;
  if (__popcll(m) >= need) {
    unsigned long long mm = m;
    for (int z = 1; z < need; ++z) mm &= mm - 1;
    done += (uint32_t)(__ffsll((long long)mm) - 1) + 1;
    count = 5;
    return true;
  }
  count += (uint32_t)__popcll(m);
  done += avail;
  return false;
}

// what pair p leaves behind (a: a kernel's arguments; the outputs are indexed by pair - pair_begin): its p-value and shuffle
// count, or (only after the opening pass) -1 - hits for the pass that goes on
template <class Args>
__device__ __forceinline__ void perm_write(const Args& a, size_t p, bool stop, uint32_t done, uint32_t count) {
  if (stop || done >= a.max_perm) {
    a.pvalue[p - a.pair_begin] = (double)(count + 1) / (double)(done + 1);
    a.nperm[p - a.pair_begin] = (int32_t)done;
  } else {
    a.nperm[p - a.pair_begin] = -1 - (int32_t)count;
  }
}

// One launch of a permutation-test kernel over npairs pairs, G per wave: `shared` bytes of LDS per workgroup and wave_bytes
// per wave.  Up to four waves per workgroup within kPermLdsPlan, workgroups per CU by what fits kPermLdsLimit, the grid
// bounded by the CUs (the kernels walk their pairs with a stride loop).  Refuses what does not fit one workgroup.
template <class Args>
hipError_t perm_launch(void (*kernel)(Args), Args& a, size_t shared, size_t wave_bytes, int G, size_t npairs, int cu_count,
                       hipStream_t stream) {
  if (shared + wave_bytes > kPermLdsLimit) return hipErrorInvalidValue;
  a.wave_bytes = (int)wave_bytes;
  const int waves = (int)std::max<size_t>(1, std::min<size_t>(4, (kPermLdsPlan - shared) / wave_bytes));
  const size_t lds = shared + (size_t)waves * wave_bytes;
  const hipError_t e = mica_allow_lds(kernel, lds);
  if (e != hipSuccess) return e;
  const size_t per_cu = std::max<size_t>(1, kPermLdsLimit / lds);
  const size_t units = (npairs + G - 1) / G;
  const unsigned grid = (unsigned)std::min<size_t>((units + waves - 1) / waves, (size_t)cu_count * per_cu);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, stream, a);
  return hipGetLastError();
}

}  // namespace cmx
