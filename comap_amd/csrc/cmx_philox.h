// The counter RNG of the simulators, one definition for device and host (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmx {

// Philox2x32-10 (Random123): counter = (g_lo, g_hi[14:0] | draw << 15), key = seed_lo ^ seed_hi * 0x9E3779B9 ^ 'CMX2'.
// Same scheme as oracle/oracle.c (DESIGN.md "RNG").  One 32 x 32 -> 64 multiply per round: the 4x32 variant (two per
// round, 128 output bits) cost the fused null kernel 4.7 % of its time in quarter-rate integer multiplies.
// g < 2^47, draw < 2^17.
//   draw 0 (rate class / continuous rate / a bootstrap's site index) and 1 (root state): counter from the site's g, the
//   64 output bits give one 53-bit uniform (philox_uniform);
//   draw 2 + node (state at the lower end of a branch): the sites 2k and 2k + 1 SHARE the call with counter g >> 1 and
//   take its first and second output word as a 32-bit uniform (cmx_simulate.hip: philox_node_uniform): the node draws
//   are 99 % of a simulation's calls, a category's probability is resolved to 2^-32 either way, and a thread that holds
//   both sites of a pair (simulate_chain_kernel) makes one call for two draws.
__host__ __device__ __forceinline__ void philox_words(uint64_t seed, uint64_t g, uint32_t draw, uint32_t& w0, uint32_t& w1) {
  uint32_t c0 = (uint32_t)g, c1 = ((uint32_t)(g >> 32) & 0x7fffu) | (draw << 15);
  uint32_t k = (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x9E3779B9u) ^ 0x434d5832u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p = (uint64_t)0xD256D193u * (uint64_t)c0;   // one v_mad_u64_u32 instead of v_mul_hi + v_mul_lo
#ifdef __HIP_DEVICE_COMPILE__
    c0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p >> 32), k, c1, 0x96);   // three-way xor in one v_bitop3_b32
#else
    c0 = (uint32_t)(p >> 32) ^ k ^ c1;
#endif
    c1 = (uint32_t)p;
    k += 0x9E3779B9u;
  }
  w0 = c0;
  w1 = c1;
}
__host__ __device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t g, uint32_t draw) {
  uint32_t c0, c1;
  philox_words(seed, g, draw, c0, c1);
  const uint64_t bits = (((uint64_t)c0 << 32) | c1) >> 11;
  return (double)bits * (1.0 / 9007199254740992.0);
}

}  // namespace cmx
