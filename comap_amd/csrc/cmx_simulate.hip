// The sequence simulators: simulate_kernel, the null's simulate_blocked_kernel / simulate_chain_kernel (the same draws in
// the layout the null-mode mapping kernel reads) and simulate_continuous_kernel, all on the counter RNG of cmx_philox.h.
#include <algorithm>

#include "cmx_device.h"
#include "cmx_lanes.h"
#include "cmx_philox.h"

namespace cmx {

// a node draw of site g: its word of the call the sites g & ~1 and g | 1 share (cmx_philox.h)
__device__ __forceinline__ double philox_node_uniform(uint64_t seed, uint64_t g, uint32_t node) {
  uint32_t w0, w1;
  philox_words(seed, g >> 1, 2u + node, w0, w1);
  return (double)((g & 1) ? w1 : w0) * (1.0 / 4294967296.0);
}

template <class CumPtr>
__device__ __forceinline__ int draw_index(double u, CumPtr cum, int n) {
  int idx = 0;
  for (int j = 0; j < n - 1; ++j) idx += (u >= cum[j]) ? 1 : 0;
  return idx;
}
// the same index (#{ j < n-1 : u >= cum[j] }, cum non-decreasing) found from a guide table: entry k = the number of
// leading running sums that are <= k/32, so the scan for a u in [k/32, (k+1)/32) starts there -- one or two reads of the
// lane's own row instead of n - 1 (the rows are lane-divergent 160-byte gathers: the simulator's whole cost)
__device__ __forceinline__ int draw_guided(double u, const double* __restrict__ cum, const uint8_t* __restrict__ guide, int n) {
  int idx = guide[(int)(u * 32.0)];
  while (idx < n - 1 && u >= cum[idx]) ++idx;
  return idx;
}
// the two draws a site makes for itself: its rate class (draw 0, on DevModel::cum_probs) and its state at the root
// (draw 1, on cum_pi).  They take the table and its length, not the model: a kernel holds S0 and C0 already, and the
// text hipcc emits for simulate_chain_kernel changes when the helpers read them from the model again.
__device__ __forceinline__ int draw_class(const double* cum_probs, int C0, uint64_t seed, uint64_t g) {
  return draw_index(philox_uniform(seed, g, 0), cum_probs, C0);
}
__device__ __forceinline__ int draw_root(const double* cum_pi, int S0, uint64_t seed, uint64_t g) {
  return draw_index(philox_uniform(seed, g, 1), cum_pi, S0);
}

// ------------------------------------------------------------------------------------------------ stand-alone simulator
// rep_ram != 0: the n sites are blocks of rep_ram (the replicates of one side of a null, side by side in the alignment);
// block r holds the global sites g0 + r * gstep ..  (one launch for all replicates of a side)
__global__ void simulate_kernel(const DevModel m, uint64_t seed, uint64_t g0, size_t n, uint8_t* aln, size_t ld,
                                int32_t* classes, uint8_t* states, size_t rep_ram, uint64_t gstep) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t g = rep_ram ? g0 + (uint64_t)(j / rep_ram) * gstep + (uint64_t)(j % rep_ram) : g0 + j;
  const int S = m.S0;
  const int c = draw_class(m.cum_probs, m.C0, seed, g);
  if (classes) classes[j] = c;
  states[(size_t)m.root * ld + j] = (uint8_t)draw_root(m.cum_pi, S, seed, g);
  for (int node = m.nn - 2; node >= 0; --node) {
    const int x = states[(size_t)m.parent[node] * ld + j];
    const size_t row = ((size_t)c * m.nn + node) * S + x;
    const int y = draw_guided(philox_node_uniform(seed, g, (uint32_t)node), m.CP + row * S, m.CPG + row * 32, S);
    states[(size_t)node * ld + j] = (uint8_t)y;
    const int tx = m.taxon_of[node];
    if (tx >= 0) aln[(size_t)tx * ld + j] = (uint8_t)y;
  }
}

hipError_t launch_simulate(const DevModel& m, uint64_t seed, uint64_t g0, size_t n, uint8_t* d_aln, size_t ld,
                           int32_t* d_classes, uint8_t* d_states, hipStream_t stream, size_t rep_ram, uint64_t gstep) {
  const int block = 256;
  const int grid = (int)((n + block - 1) / block);
  hipLaunchKernelGGL(simulate_kernel, dim3(grid), dim3(block), 0, stream, m, seed, g0, n, d_aln, ld, d_classes, d_states, rep_ram, gstep);
  return hipGetLastError();
}

// The null's simulator (cmx_null_simulate_dev), the gather kernel: the SAME draws as simulate_kernel, one thread per site
// at full occupancy.  A mapping wave holds half a SIMD's registers, and simulating its 64 sites inside it was 7.8 % of
// the wave's time, all of it dependent L2 gathers that two waves per SIMD cannot hide; here thousands of waves hide them
// (cfg3, same box: simulated inside the mapping kernel 12.96 ms, mapping of supplied alignments 11.98 ms + this kernel).
// Nodes are drawn level by level in groups of four (m.simg), four running sums per round trip of the search.
// Sites s = 0 .. of one null launch: g = g0 + s; (replicate, batch) block s / blk, column s % blk of an alignment stored
// as [block][taxon][blk] -- the layout map_kernel<S, kModeNull> reads its alignments in.
__global__ __launch_bounds__(256) void simulate_blocked_kernel(const DevModel m, uint64_t seed, uint64_t g0, size_t s0, size_t n,
                                                               size_t blk, uint8_t* __restrict__ aln,
                                                               uint8_t* __restrict__ states /*[nn][n]*/) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const size_t s = s0 + j;
  const uint64_t g = g0 + s;
  const int S0 = m.S0;
  uint8_t* out = aln + (s / blk) * (size_t)m.T * blk + s % blk;
  const int c = draw_class(m.cum_probs, m.C0, seed, g);
  states[(size_t)m.root * n + j] = (uint8_t)draw_root(m.cum_pi, S0, seed, g);
  for (int gi = 0; gi < m.nsimg; ++gi) {
    const cmx_cint q = (cmx_cint)m.simg + gi * 16;   // [0..3] node, [4..7] its parent, [8..11] its taxon or -1
    int x[4], idx[4];
    double u[4];
    size_t row[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) x[jj] = states[(size_t)q[4 + jj] * n + j];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) u[jj] = philox_node_uniform(seed, g, (uint32_t)q[jj]);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      row[jj] = ((size_t)c * m.nn + q[jj]) * S0 + x[jj];
      idx[jj] = m.CPG[row[jj] * 32 + (int)(u[jj] * 32.0)];
    }
    bool any;
    do {
      double cv[4][4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int d = 0; d < 4; ++d) cv[jj][d] = m.CP[row[jj] * S0 + idx[jj] + d];   // the table is padded by 4 sums
      any = false;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        bool go = true;
        int adv = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          go = go && idx[jj] + d < S0 - 1 && u[jj] >= cv[jj][d];
          adv += go ? 1 : 0;
        }
        idx[jj] += adv;
        any |= adv == 4;
      }
    } while (any);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      states[(size_t)q[jj] * n + j] = (uint8_t)idx[jj];
      if (q[8 + jj] >= 0) out[(size_t)q[8 + jj] * blk] = (uint8_t)idx[jj];
    }
  }
}

// The same simulator with the tables of the node being drawn in LDS.  A draw needs one guide byte and a few entries of
// ONE of C * S rows of its node; gathered from L2 by every thread that is ~100 bytes of traffic per draw (2.5e9 draws per
// target launch: the gather kernel above took 22 ms there, L2-bound).  Here a workgroup draws batches of 2 NT sites (a
// pair per thread), node by node, parents first (m.simord, level by level): the node's
// block is copied into LDS once per workgroup, double-buffered (global -> registers while the current node is drawn,
// registers -> the other buffer), and every search runs on LDS.  The vector unit issues for most of the kernel
// (DESIGN 6), so the kernel is built to save instructions first and a node's latencies second.  Same draws, same states
// as simulate_kernel.
//  * integer search.  A node draw is u = w / 2^32 of a 32-bit Philox word: the guide entry is w >> 27 and "u >= cum" is
//    "w > threshold" against the host's 32-bit thresholds (cmx_layout.h, HostModel::simtab) -- no conversion to double,
//    no 64-bit compares, and a row ends in thresholds nobody exceeds instead of a bounds test per running sum.  A node's
//    block is two thirds of the bytes of its running sums and guides and arrives as one contiguous copy.
//  * STEP thresholds per search and LDS round trip, the pair's two searches side by side (a `while (w > thr[idx]) ++idx`
//    per site is a chain of dependent LDS reads under a divergent branch).
//  * the tables are staged once per NB batches of 2 NT sites, drawn one after the other (a loop over batches, not wider
//    searches): barriers, table bytes and their addressing per site fall by NB at a few registers per batch.
//  * one barrier per node: the next node's tables go into the other buffer BEFORE the barrier (every thread stopped
//    reading that buffer at the previous node's barrier).
//  * the parent's states of node it + 1 are loaded at the top of node it, beside the table prefetch; a node whose parent
//    is the node just drawn (the root's first child, caterpillar chains) takes them from the registers they were drawn into.
//  * a leaf's states go to the alignment only: nobody reads them back from `states`.
template <int NB /* batches of 2 NT sites per workgroup */, int NCH /* 16-byte pieces of a node's block per thread */, int NT, int WAVES, int STEP>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void simulate_chain_kernel(const DevModel m, const uint8_t* __restrict__ tabs, uint64_t seed, uint64_t g0, size_t s0, size_t n,
                                                           size_t blk, uint8_t* __restrict__ aln, uint8_t* __restrict__ states) {
  static_assert(STEP <= kSimThrPad, "a search reads STEP thresholds past its index");
  extern __shared__ __attribute__((aligned(16))) uint8_t sim_smem[];
  const int S0 = m.S0, C0 = m.C0, tid = threadIdx.x;
  const int rs = sim_thr_row(S0), tabb = C0 * S0 * rs * 4, nodeb = (int)sim_node_bytes(S0, C0), nch = nodeb / 16;
  // batch b of this thread: the sites jb0 + b * 2 NT and its neighbour (g0, s0, n even: one Philox call per node, the pair's
  // states one 16-bit word; both inside n or both outside)
  const size_t jb0 = (size_t)blockIdx.x * NB * (2 * NT) + (size_t)(2 * tid);
  const uint64_t gp0 = (g0 + s0 + jb0) >> 1;
  uint8_t* out[NB];
  unsigned crow[NB], xc[NB];   // class rows of the pair (16 bits each); the parent's states of the pair (8 bits each)
  unsigned on = 0, wrap = 0;   // per batch: inside n; the pair's second site opens the next replicate block (odd blk only)
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const size_t jj = jb0 + (size_t)b * (2 * NT);
    const bool in = jj < n;
    const size_t s = s0 + (in ? jj : 0);   // (a batch outside n draws site 0 again and stores nothing)
    const uint64_t g = g0 + s;
    const size_t col = s % blk;
    out[b] = aln + (s / blk) * (size_t)m.T * blk + col;
    on |= (in ? 1u : 0u) << b;
    wrap |= (col == blk - 1 ? 1u : 0u) << b;
    const int c0 = draw_class(m.cum_probs, C0, seed, g), c1 = draw_class(m.cum_probs, C0, seed, g + 1);
    crow[b] = (unsigned)(c0 * S0) | ((unsigned)(c1 * S0) << 16);
    const int r0 = draw_root(m.cum_pi, S0, seed, g), r1 = draw_root(m.cum_pi, S0, seed, g + 1);
    xc[b] = (unsigned)r0 | ((unsigned)r1 << 8);
    if (in) *reinterpret_cast<unsigned short*>(states + (size_t)m.root * n + jj) = (unsigned short)xc[b];
  }
  const cmx_cint ord = (cmx_cint)m.simord;
  int buf = 0;
  for (int q = tid; q < nch; q += NT)
    reinterpret_cast<cmx_i4*>(sim_smem)[q] = reinterpret_cast<const cmx_i4*>(tabs + (size_t)ord[0] * nodeb)[q];
  __syncthreads();
  // (ord[0] is a child of the root: xc holds its parent's states)
  for (int it = 0; it < m.nn - 1; ++it) {
    const int node = ord[it];
    const bool more = it + 1 < m.nn - 1;
    cmx_i4 nxt[NCH];
    unsigned xn[NB];
    bool chain = false;
    if (more) {
      const int nnode = ord[it + 1], npar = ((cmx_cint)m.parent)[nnode];
      const cmx_i4* src = reinterpret_cast<const cmx_i4*>(tabs + (size_t)nnode * nodeb);
#pragma unroll
      for (int i = 0; i < NCH; ++i)
        if (tid + NT * i < nch) nxt[i] = src[tid + NT * i];
      chain = npar == node;
      if (!chain) {
        const uint8_t* sp = states + (size_t)npar * n + (unsigned)jb0;
#pragma unroll
        for (int b = 0; b < NB; ++b) xn[b] = (on >> b & 1) ? *reinterpret_cast<const unsigned short*>(sp + b * (2 * NT)) : 0u;
      }
    }
    const uint32_t* T_ = reinterpret_cast<const uint32_t*>(sim_smem + (size_t)buf * nodeb);
    const uint8_t* G_ = sim_smem + (size_t)buf * nodeb + tabb;
    const int tx = ((cmx_cint)m.taxon_of)[node];
    uint8_t* sn = states + (size_t)node * n + (unsigned)jb0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      uint32_t w[2];
      philox_words(seed, gp0 + (uint64_t)(b * NT), 2u + (uint32_t)node, w[0], w[1]);
      int idx[2];
      const uint32_t* thr[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int row = (int)((crow[b] >> (16 * k)) & 0xffffu) + (int)((xc[b] >> (8 * k)) & 0xffu);
        idx[k] = G_[row * 32 + (int)(w[k] >> 27)];
        thr[k] = T_ + __mul24(row, rs);
      }
      // STEP thresholds per search and LDS round trip; the thresholds rise along a row, so the ones below w come first
      bool any;
      do {
        uint32_t tv[2][STEP];
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int d = 0; d < STEP; ++d) tv[k][d] = thr[k][idx[k] + d];
        any = false;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          int adv = 0;
#pragma unroll
          for (int d = 0; d < STEP; ++d) adv += w[k] > tv[k][d] ? 1 : 0;
          idx[k] += adv;
          any |= adv == STEP;
        }
      } while (any);
      const unsigned pair = (unsigned)idx[0] | ((unsigned)idx[1] << 8);
      if (chain) xn[b] = pair;
      if (on >> b & 1) {
        if (tx < 0) {
          *reinterpret_cast<unsigned short*>(sn + b * (2 * NT)) = (unsigned short)pair;
        } else if (((blk | (size_t)(uintptr_t)aln) & 1) == 0) {   // (an even rep_ram: the pair sits in one replicate block, at an even address)
          *reinterpret_cast<unsigned short*>(out[b] + (size_t)tx * blk) = (unsigned short)pair;
        } else {
          uint8_t* o = out[b] + (size_t)tx * blk;
          o[0] = (uint8_t)idx[0];
          o[(wrap >> b & 1) ? 1 + (size_t)(m.T - 1) * blk : (size_t)1] = (uint8_t)idx[1];
        }
      }
    }
    if (more) {
#pragma unroll
      for (int b = 0; b < NB; ++b) xc[b] = xn[b];
#pragma unroll
      for (int i = 0; i < NCH; ++i)
        if (tid + NT * i < nch) reinterpret_cast<cmx_i4*>(sim_smem + (size_t)(buf ^ 1) * nodeb)[tid + NT * i] = nxt[i];
      __syncthreads();   // the next node's tables are in place, and nobody reads this node's any more
      buf ^= 1;
    }
  }
}

// From how many sites of a launch on the tables go through LDS; below, the gather kernel, one thread per site and no
// barrier, is quicker.  A workgroup's walk over the 126 nodes of the target's tree takes simulate_chain_kernel 0.15 ms
// however few workgroups there are (the gather kernel: 0.14 ms at 50 000 sites, 0.18 at 100 000, 0.50 at 450 000).
constexpr size_t kSimChainMinSites = 75000;
// Four batches per workgroup once they fill every workgroup slot of the chip (256 CUs x 4) at least once: 4.04 ms
// against 5.09 for the target's 2 * 10^7 sites, but 0.51 against 0.30 ms for 10^6, where a quarter of the CUs would work.
constexpr size_t kSimChainFourBatches = (size_t)4 * 1024 * 1024;

// 512 threads, a pair of sites each per batch, eight waves per SIMD; two 16-byte pieces of a node's block per thread up
// to six classes of 20 states (16 384 B), three up to kSimNodeBytesMax.  One batch: 38 / 44 registers, four thresholds per round
// trip of a search; four batches: 64 registers (8 / 12 spilled), two thresholds (four: 4.27 ms, more spills).
// LDS: two node blocks, 20 480 B for the target's model.
template <int NB, int STEP>
static void launch_simulate_chain(const DevModel& m, const uint8_t* d_simtab, uint64_t seed, uint64_t g0, size_t s0, size_t n, size_t blk,
                                  uint8_t* d_aln, uint8_t* d_states, hipStream_t stream) {
  const size_t nodeb = sim_node_bytes(m.S0, m.C0);
  const dim3 grid((unsigned)((n + NB * 1024 - 1) / (NB * 1024)));
  if (nodeb <= (size_t)2 * 512 * 16)
    hipLaunchKernelGGL((simulate_chain_kernel<NB, 2, 512, 8, STEP>), grid, dim3(512), 2 * nodeb, stream, m, d_simtab, seed, g0, s0, n, blk,
                       d_aln, d_states);
  else
    hipLaunchKernelGGL((simulate_chain_kernel<NB, 3, 512, 8, STEP>), grid, dim3(512), 2 * nodeb, stream, m, d_simtab, seed, g0, s0, n, blk,
                       d_aln, d_states);
}

// nsites sites with global indices g0 .. in passes of at most `chunk` (the states scratch holds nn * chunk bytes)
hipError_t launch_simulate_blocked(const DevModel& m, uint64_t seed, uint64_t g0, size_t nsites, size_t blk, uint8_t* d_aln,
                                   uint8_t* d_states, size_t chunk, hipStream_t stream, const SimChoice& choice) {
  const size_t min_sites = choice.min_sites >= 0 ? (size_t)choice.min_sites : kSimChainMinSites;
  const size_t four_sites = choice.four_batch_sites >= 0 ? (size_t)choice.four_batch_sites : kSimChainFourBatches;
  for (size_t s0 = 0; s0 < nsites; s0 += chunk) {
    const size_t n = std::min(chunk, nsites - s0);
    // the chain kernel wherever the model has its tables (cmx_layout.h: sim_has_tables) and the pass is large enough.  It
    // pairs the sites 2 k, 2 k + 1 of the global numbering and stores a pair's symbols as one 16-bit word at column
    // s0 + j of its replicate block: g0, s0 and n all have to be even, not just g0 + s0.
    if (choice.simtab && n >= min_sites && (g0 & 1) == 0 && (s0 & 1) == 0 && (n & 1) == 0) {
      if (n >= four_sites)
        launch_simulate_chain<4, 2>(m, choice.simtab, seed, g0, s0, n, blk, d_aln, d_states, stream);
      else
        launch_simulate_chain<1, 4>(m, choice.simtab, seed, g0, s0, n, blk, d_aln, d_states, stream);
    } else {
      hipLaunchKernelGGL(simulate_blocked_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, seed, g0, s0, n, blk,
                         d_aln, d_states);
    }
  }
  return hipGetLastError();
}

// ---- simulations.continuous = yes (CoMap/CoMap.cpp:146, 213: NonHomogeneousSequenceSimulator::enableContinuousRates).
// Every site draws its own rate from the CONTINUOUS Gamma(alpha, beta = alpha) distribution (Invariant(Gamma): rate 0 with
// probability p_inv, else the Gamma draw divided by 1 - p_inv) and every branch uses exp(Q r t) of that very rate: the
// row of the parent's state is rebuilt from the generator's eigensystem at each node (S exponentials + S^2 multiply-adds)
// -- there is no table to look up.  Same counter RNG and draw numbering as the discrete simulator (draw 0 = rate).

__host__ __device__ inline void cmx_gamma_pq(double a, double x, double* p, double* q) {
  /* regularised incomplete gamma, lower P and upper Q = 1 - P, each from the expansion that gives it without
   * cancellation: series for x < a + 1 (P), Lentz continued fraction otherwise (Q) */
  if (x <= 0.0) { *p = 0.0; *q = 1.0; return; }
  const double pre = exp(-x + a * log(x) - lgamma(a));
  if (x < a + 1.0) {
    double term = 1.0 / a, sum = term;
    for (int n = 1; n < 1000; ++n) {
      term *= x / (a + n);
      sum += term;
      if (fabs(term) < fabs(sum) * 1e-17) break;
    }
    *p = sum * pre;
    *q = 1.0 - *p;
    return;
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i < 1000; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 1e-16) break;
  }
  *q = pre * h;
  *p = 1.0 - *q;
}
/* "x is below the u-quantile": decided on the tail that carries the information (P < u, or Q > 1 - u for u > 1/2) */
__host__ __device__ inline int cmx_gamma_below(double a, double x, double u) {
  double p, q;
  cmx_gamma_pq(a, x, &p, &q);
  return u <= 0.5 ? p < u : q > 1.0 - u;
}
/* quantile of Gamma(shape a, scale 1): bracket [lo, 2 lo] by doubling / halving from 1, then 110 bisection steps
 * (deterministic, no tolerance test) */
__host__ __device__ inline double cmx_gamma_quantile(double a, double u) {
  if (u <= 0.0) return 0.0;
  double lo = 1.0, hi;
  if (cmx_gamma_below(a, lo, u)) {
    for (int i = 0; i < 1100 && cmx_gamma_below(a, 2.0 * lo, u); ++i) lo *= 2.0;
    hi = 2.0 * lo;
  } else {
    hi = lo;
    lo = 0.5 * hi;
    for (int i = 0; i < 1070 && !cmx_gamma_below(a, lo, u); ++i) { hi = lo; lo *= 0.5; }
  }
  for (int i = 0; i < 110; ++i) {
    const double mid = 0.5 * (lo + hi);
    if (cmx_gamma_below(a, mid, u)) lo = mid; else hi = mid;
  }
  return 0.5 * (lo + hi);
}

__global__ void simulate_continuous_kernel(const DevModel m, uint64_t seed, uint64_t g0, size_t n, double alpha, double p_inv,
                                           uint8_t* aln, size_t ld, double* rates, uint8_t* states) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t g = g0 + j;
  const int S = m.S0;
  const double u0 = philox_uniform(seed, g, 0);
  double r = 0.0;
  if (u0 >= p_inv) r = cmx_gamma_quantile(alpha, (u0 - p_inv) / (1.0 - p_inv)) / alpha / (1.0 - p_inv);
  if (rates) rates[j] = r;
  states[(size_t)m.root * ld + j] = (uint8_t)draw_root(m.cum_pi, S, seed, g);
  for (int node = m.nn - 2; node >= 0; --node) {
    const int x = states[(size_t)m.parent[node] * ld + j];
    const double u = philox_node_uniform(seed, g, (uint32_t)node);
    const size_t mo = (size_t)m.model_of[node];
    const double *V = m.eigV + mo * S * S + (size_t)x * S, *Vi = m.eigVi + mo * S * S, *lam = m.eigLam + mo * S;
    const double rt = r * m.blen[node];
    double w[kPlainStates];    // V[x][k] exp(lambda_k r t), S <= kPlainStates entries (dynamically indexed: private memory)
    for (int k = 0; k < S; ++k) w[k] = V[k] * exp(lam[k] * rt);
    // index = #{ y < S-1 : u >= cum_y } with cum the running sum of the row P(x, .) -- the discrete simulator's rule
    int idx = 0;
    double cum = 0.0;
    for (int y = 0; y < S - 1; ++y) {
      double pxy = 0.0;
      for (int k = 0; k < S; ++k) pxy += w[k] * Vi[(size_t)k * S + y];
      cum += pxy;
      idx += (u >= cum) ? 1 : 0;
    }
    states[(size_t)node * ld + j] = (uint8_t)idx;
    const int tx = m.taxon_of[node];
    if (tx >= 0) aln[(size_t)tx * ld + j] = (uint8_t)idx;
  }
}

hipError_t launch_simulate_continuous(const DevModel& m, uint64_t seed, uint64_t g0, size_t n, double alpha, double p_inv,
                                      uint8_t* d_aln, size_t ld, double* d_rates, uint8_t* d_states, hipStream_t stream) {
  const int block = 128;
  hipLaunchKernelGGL(simulate_continuous_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, stream, m, seed, g0, n,
                     alpha, p_inv, d_aln, ld, d_rates, d_states);
  return hipGetLastError();
}

}  // namespace cmx
