// The mapping walk: hand-written gfx950 (CDNA4) kernels.  fp64 throughout (the reference computes in double and its
// DR likelihood has no per-node rescaling, CoMap/CoETools.cpp:244).
//
// map_kernel<S, MODE, FUSE, NG>
//   one wavefront = 64 sites (lane == site, NG = 4 site groups of 16) x all rate classes in turn; four independent waves
//   per workgroup.  (NG = 1: the 16-site wave-tasks of the class-split launch for small alignments.)
//   Replaces, per site: DRHomogeneousTreeLikelihood::initialize (post-order "inside" pass), the pre-order
//   "outside" pass, LegacySubstitutionMappingTools::computeSubstitutionVectors and computeNormForSite
//   (call sites CoMap/CoETools.cpp:397, CoMap/AnalysisTools.cpp:592-612; algorithm SURVEY.md A.2/A.3/A.6).
//   The SxS operator of an edge is the same for all 64 lanes: every operator use of a class pass (products on
//   internal edges, row gathers by observed symbol on leaf edges) is listed by the host in one op stream and staged
//   in LDS by LDS-DMA one op ahead (an op requests the next op's operator and waits for its own; a product of the 64-site
//   protein walk requests from the gaps between its first matrix instructions).  How long an op may leave later requests
//   in flight when it waits -- the vmcnt immediate -- is counted at run time (CountedState::vs) by every instantiation but the
//   64-site protein walk, which reads it from its stream entry: the host has counted it per entry and proved the plan on a
//   model of the wave's memory queue (cmx_layout.h: wait plan; cmx_host_verify.cpp: WaitModel).  That walk's stream entry
//   is one 16-byte scalar load per op from a running pointer: the operator's offset from the pass's class block, the
//   symbol row, the immediate; the wrap into the next pass is in the copy of the stream a pass reads, chosen at the pass
//   boundary.  Products run on the matrix cores
//   (v_mfma_f64_4x4x4_4b, 100 per 20x20 product; the
//   64-site protein walk: 20 v_mfma_f64_16x16x4_f64 for states 0..15 and 20 v_mfma_f64_4x4x4_4b for states 16..19) in
//   a layout where lane = (state inside a 4-state tile, site of a group of 16).
//   Matrices are packed host-side in 4x4 blocks so that one copy serves both P.d (inside) and P^T.u (outside).
//   Inside vectors / outside messages that must survive go to a per-wave HBM workspace as [S/2][lane][2]: every
//   access is one fully coalesced 1 KiB row; they come back by compiler-visible global loads into registers the walk has
//   declared dead long before (DevWalk::load), under the cache policy StatePolicy names (`nt` both ways for proteins).
//   LDS holds, per wave, two operator stage buffers and four symbol slots; the 64-site
//   protein walk adds one workspace vector (DevWalk::kLdsSlot) for the short-lived vectors the host's plan names.
//   DESIGN.md 4.1 has the full description and the measurements.
//   MODE == kModeNull: map (x2 batches) -> per-pair statistic of AnalysisTools::getNullDistributionIntraDR
//   (CoMap/AnalysisTools.cpp:587-653) per wave, on alignments simulated beforehand by simulate_chain_kernel /
//   simulate_blocked_kernel at full occupancy.
//   MODE == kModeNullPatterns: the same walk over the null's distinct columns, one lane per pattern; the pairs are scored
//   by null_pattern_pairs_kernel (cmx_null_patterns.hip).
//   MODE == kModeNullMsg / kModeNullPatternsMsg: the two null modes of a 20-state model with a cherry message table
//   (cmx_layout.h; filled by cherry_msg_kernel below): an inlined cherry's message is gathered from the table.
#include "cmx_device.h"
#include "cmx_lanes.h"
#include "cmx_pairstat.h"
#include "cmx_walk.h"

namespace cmx {

// ------------------------------------------------------------------------------------------------ ring matvec
typedef double d2 __attribute__((ext_vector_type(2)));

// Every edge of the tree applies one SxS operator that is the same for all 64 lanes: a matrix-vector product on
// internal edges, a row gather by observed symbol on leaf edges.  The sequence of operators of a class pass is known
// (host-built op stream, m.msched), so each operator is DMAed into LDS one op ahead: two S*S*8-byte stage buffers per
// wave, op i reads buffer i&1 while the DMA of op i+1 fills the other (global_load_lds_dwordx4, 1 KiB per
// instruction, no VGPRs).  A product reads the A operand of each 4x4 tile with one ds_read_b64 and runs on
// v_mfma_f64_4x4x4_4b (see "Matrix-core layout" below); a leaf op reads the values its lane holds of row `symbol` of
// the transposed matrix.  The symbols of the next leaf op are DMAed the same way (global_load_lds_ubyte into a
// 256-byte slot).
// History: an s_load-fed v_fma_f64 version ran at 39 TFLOP/s; tiles in a VGPR ring applied with
// v_fmac_f64_dpp row_newbcast (53 TFLOP/s in isolation) needed either fixed registers -- amdgpu_num_vgpr turned out not
// to be a hard limit, the compiler reused them under pressure -- or 50 more loop-carried registers than two waves per
// SIMD can afford; the LDS-staged DPP version (lane = site) reached 16.7 ms per launch, the matrix-core layout 15.5 ms;
// gathering leaf rows straight from L2 (lane-divergent 160-byte rows, latency exposed at every leaf) cost 5 of 21 ms.

typedef __attribute__((address_space(1))) const void* cmx_gptr;
typedef __attribute__((address_space(3))) void* cmx_lptr;

template <int S>
struct MatStage {
  static constexpr int NROW = S + max_ambig(S);              // rows of a transposed leaf operator (states + ambiguity ids)
  static constexpr int UNIT = mat_unit(S);                   // doubles per device matrix
  static constexpr int BYTES = UNIT * 8;                     // one operator
  static constexpr int FULL = BYTES / 1024;                  // full 1 KiB DMA rows
  static constexpr int TAIL = (BYTES % 1024) / 16;           // lanes of the last, partial row
  static constexpr int ROWS = FULL + (TAIL ? 1 : 0);         // VMEM instructions per operator
  static_assert(BYTES % 16 == 0, "operator size must be a multiple of 16 bytes");
};
constexpr int kCodeSlotBytes = 4 * kWave;  // one dword per lane

// LDS-DMA is issued through inline asm on purpose.  hipcc models __builtin_amdgcn_global_load_lds as a write to
// LDS that any later ds_read may alias, and puts s_waitcnt vmcnt(0) in front of the next LDS read: with one dynamic LDS
// array every operator and symbol would then be waited for right after the NEXT one was requested,
// i.e. the whole L2/HBM latency exposed once per op.  An asm DMA is invisible to that bookkeeping; the ordering
// between a DMA and the LDS reads of its data is kept by the counted waits below (wait_vm), and compiler-issued
// vmcnt waits for its own loads only become stricter (it undercounts what is in flight).
// One instruction moves 64 lanes x 16 B = 1 KiB; the instruction offset advances the global and the LDS address alike,
// so consecutive 1 KiB rows need one M0 value and one address register.
__device__ __forceinline__ uint32_t lds_addr(const uint8_t* p) {
  // wave-uniform by construction; readfirstlane tells the compiler so (M0 is written from an SGPR)
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uintptr_t)(__attribute__((address_space(3))) const uint8_t*)p);
}
template <int NROWS>
__device__ __forceinline__ void dma_rows16(const void* g /* per lane: row 0 address of this lane */, uint32_t lds) {
  static_assert(NROWS >= 1 && NROWS <= 4, "instruction offset range");
  if constexpr (NROWS == 1)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds), "v"(g) : "memory");
  else if constexpr (NROWS == 2)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %1, off offset:1024" ::"s"(lds), "v"(g) : "memory");
  else if constexpr (NROWS == 3)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %1, off offset:1024\n\tglobal_load_lds_dwordx4 %1, off offset:2048" ::"s"(lds), "v"(g) : "memory");
  else
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %1, off offset:1024\n\tglobal_load_lds_dwordx4 %1, off offset:2048\n\t"
                 "global_load_lds_dwordx4 %1, off offset:3072" ::"s"(lds), "v"(g) : "memory");
}

// DMA the operator at `src` (global, wave-uniform) into the stage buffer `buf` (LDS, wave-uniform)
template <int S>
__device__ __forceinline__ void mat_dma_l(const double* src, uint32_t l, int lane);
template <int S>
__device__ __forceinline__ void mat_dma(const double* src, uint8_t* buf, int lane) { mat_dma_l<S>(src, lds_addr(buf), lane); }
template <int S>
__device__ __forceinline__ void mat_dma_l(const double* src, uint32_t l /* LDS byte address, wave-uniform */, int lane) {
  const double* g = src + 2 * lane;
  if constexpr (MatStage<S>::FULL > 0) dma_rows16<MatStage<S>::FULL>(g, l);
  if constexpr (MatStage<S>::TAIL > 0) {
    if (lane < MatStage<S>::TAIL) dma_rows16<1>(g + MatStage<S>::FULL * 128, l + MatStage<S>::FULL * 1024);
  }
}
// the first BYTES bytes of an operator only (compile-time): products of a class-fused model need their NB diagonal tiles,
// leaf ops on fully resolved alignments (the null's simulated ones) the S0 state rows of the transposed operator
template <int BYTES>
struct MatPart {
  static constexpr int FULL = BYTES / 1024, TAIL = (BYTES % 1024 + 15) / 16, ROWS = FULL + (TAIL ? 1 : 0);
};
template <int BYTES>
__device__ __forceinline__ void mat_dma_part(const double* src, uint32_t l, int lane) {
  const double* g = src + 2 * lane;
  if constexpr (MatPart<BYTES>::FULL > 0) dma_rows16<MatPart<BYTES>::FULL>(g, l);
  if constexpr (MatPart<BYTES>::TAIL > 0) {
    if (lane < MatPart<BYTES>::TAIL) dma_rows16<1>(g + MatPart<BYTES>::FULL * 128, l + MatPart<BYTES>::FULL * 1024);
  }
}
// DMA one symbol per lane (address p is per lane) into dword `lane` of the code slot.  The symbols of the null are
// written by this very wave (simulation) through the same address, hence the L1-bypassing cache policy (sc0 sc1).
__device__ __forceinline__ void code_dma_l(const uint8_t* p, uint32_t l) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_ubyte %1, off sc0 sc1" ::"s"(l), "v"(p) : "memory");
}
__device__ __forceinline__ void code_dma(const uint8_t* p, uint8_t* slot) { code_dma_l(p, lds_addr(slot)); }

// s_waitcnt vmcnt(n) needs an immediate: pick the largest supported threshold <= allowed (waiting for more is safe)
template <int N>
__device__ __forceinline__ void waitcnt_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory"); }
template <int BASE>
__device__ __forceinline__ void wait_vm_from(int v /* 0 .. 6 */) {   // vmcnt(BASE + v), as a tree of wave-uniform branches
  if (v <= 3) { if (v <= 1) { if (v == 0) waitcnt_vm<BASE>(); else waitcnt_vm<BASE + 1>(); } else { if (v == 2) waitcnt_vm<BASE + 2>(); else waitcnt_vm<BASE + 3>(); } }
  else { if (v == 4) waitcnt_vm<BASE + 4>(); else if (v == 5) waitcnt_vm<BASE + 5>(); else waitcnt_vm<BASE + 6>(); }
}
template <int S, int VL>
__device__ __forceinline__ void wait_vm(int allowed) {
  // what can have been issued after X: the next operator (1 .. R DMA rows, +1 with symbols) and up to three workspace
  // vectors (stores or loads, H instructions each).  The operator part varies per op since round 4 (products of a fused
  // model and leaf ops of resolved alignments stage a part of the unit), so every count up to R + 1 + H is exact and the
  // steps above are the multiples of H the vectors add; a smaller immediate than `allowed` only waits for more.
  constexpr int R = MatStage<S>::ROWS, H = (VL + 1) / 2;
  static_assert(R + 1 + 2 * H < 64, "vmcnt is a 6-bit counter");
  static_assert(R + 1 <= 6, "operator rows + symbols");
  const int v = allowed % H < 7 ? allowed % H : 6, q = allowed / H;   // (H >= 7 for every instantiation but S = 4: there v < H anyway)
  if (q == 0) wait_vm_from<0>(v);
  else if (q == 1) wait_vm_from<H>(v);
  else if (q == 2 && 2 * H + 6 < 64) wait_vm_from<2 * H>(v);
  else {
    // three vectors or more in flight: whatever the counter can still tell apart (it saturates at 63)
    constexpr int TOP = (3 * H + 4 < 64) ? 3 * H : (2 * H + 6 < 64 ? 2 * H + 6 : 2 * H);
    waitcnt_vm<TOP>();
  }
}

// ---- Matrix-core layout of an S-vector of the wave's 64 sites.  v_mfma_f64_4x4x4_4b computes four independent
// D[4x4] += A[4x4] . B[4x4]; measured on gfx950 (scripts/probe_mfma_f64_4x4x4.hip): A lane = 16 k + 4 blk + i,
// B lane = 16 k + 4 blk + n, D lane = 16 i + 4 blk + n.  With i / k = state inside a 4-state tile and (blk, n) = site inside
// a group of 16, B and D share one layout:
//     register v[sb * 4 + g] of lane l holds state 4 sb + (l >> 4) of site 16 g + (l & 15)
// (sb = state tile, g = site group).  A product is one MFMA per (output tile, input tile, site group): 100 matrix
// instructions instead of 400 DPP-broadcast FMAs, the accumulators of the four site groups are independent chains, and
// the other wave's vector work issues while they run.  The operator tile is read from the same packed 4x4 blocks as
// before, each lane taking the one element its A slot needs.  Elementwise work is layout-blind; sums over states
// become a reduce-scatter over the lane bits 4 and 5 that leaves lane l with the total of site l.

// reduce-scatter of per-site-group partial sums over the four state-in-tile lanes: lane l returns the total of site l.
// v_permlane32_swap exchanges the upper half of its first operand with the lower half of its second one,
// v_permlane16_swap does the same for the odd / even rows of 16 lanes: after swap(a, b) the sum a + b holds, in the
// lanes that keep a's site group, own + partner's a, and in the others own + partner's b -- no LDS round trip.
template <int NG>
__device__ __forceinline__ double reduce_sites(const double (&p)[NG]) {
  if constexpr (NG == 4) {
    double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
    swap32(p0, p2);            // lanes < 32: own p0, partner's p0   | lanes >= 32: partner's p2, own p2
    swap32(p1, p3);
    double k0 = p0 + p2, k1 = p1 + p3;   // site groups 0 / 1 in the lower half of the wave, 2 / 3 in the upper
    swap16(k0, k1);            // even rows: own k0, partner's k0    | odd rows: partner's k1, own k1
    return k0 + k1;            // site group lane >> 4: lane l holds site l
  } else {
    // one site group (16 sites per wave, small alignments): all four lanes l, l ^ 16, l ^ 32, l ^ 48 end with the total of site l & 15
    static_assert(NG == 1, "site groups per wave");
    double p0 = p[0], p1 = p0;
    swap32(p0, p1);            // p0 = the lower half's value everywhere, p1 = the upper half's
    double k = p0 + p1, q = k;
    swap16(k, q);
    return k + q;
  }
}

// step q of a product: output tile o = q / NB, input tile i = q % NB; the stored tile is (o, i), or (i, o) for the
// transposed product.  Tiles are read three steps ahead of their use (an LDS read takes ~100+ cycles and longer under
// load, the four MFMAs of a step 64); the empty asm pins the read in front of the MFMAs it overlaps.
// DIAG (class-fused nucleotide model: one 4-state tile per class, the operator is block diagonal): only the NB diagonal
// tiles are applied, step q = tile (q, q) -- the same bits as the dense product, whose other tiles are exact zeros.
template <int S, bool TR, bool DIAG>
__device__ __forceinline__ constexpr int mfma_tile(int q) {
  return DIAG ? q : (TR ? (q % (S / 4)) * (S / 4) + q / (S / 4) : q);   // (DIAG: the host stores tile (q, q) at position q)
}
// ---- The 64-site protein walk (kMfma16) runs output states 0 .. 15 of a product on v_mfma_f64_16x16x4_f64.  Measured on
// gfx950 (scripts/probe_mfma_f64_16x16x4.hip): A lane = (row l & 15, k l >> 4), B lane = (k l >> 4, column l & 15), D (lane,
// register q) = (column l & 15, row (l >> 4) + 4 q).  With column = site of a group and k / row = state, B is the register
// x of input tile i as it stands and the four D registers are states 4 q + (l >> 4), q = 0 .. 3, of the group: the walk's
// layout with q = sb.  Per site group a product is a chain of five 16x16x4 over the input tiles (A = the 16x4 panel of the
// operator, cmx_layout.h: mfma16_a_offset) and, for states 16 .. 19, the five 4x4x4_4b of output tile 4 as before: 20 + 20
// matrix instructions and 10 operator reads instead of 100 and 25.  Both instructions have K = 4 and the chain over the input
// tiles keeps its order: the same bits as 25 tile steps (the probe compares them).
// The instruction wants a group's four results in consecutive registers and the 16-byte workspace accesses want pairs, so
// an S-vector of this walk is named [g][sb 0 .. 3] followed by [sb 4][g]; every other instantiation keeps [sb][g].
template <int S, int NG, bool DIAG>
constexpr bool kMfma16 = S == 20 && NG == 4 && !DIAG;
template <int S, int NG, bool DIAG>
__device__ __forceinline__ constexpr int vreg(int sb, int g) {
  return kMfma16<S, NG, DIAG> ? (sb < 4 ? g * 4 + sb : 16 + g) : sb * NG + g;
}
typedef double d4 __attribute__((ext_vector_type(4)));

// step i of such a product: input tile i into all five output tiles of the four site groups.  The operator elements of
// step i + 1 are read before the eight matrix instructions of step i (4 x 64 + 4 x 16 cycles) that cover the read; a
// group's next 16x16x4 comes eight matrix instructions after its previous one, so no accumulator is waited for.
// REQ: the request of the NEXT op's operator, issued in the product's gaps (PlannedWalk::ProductRequest).  Slot 4 I + g lies
// between the 16x16x4 of site group g in step I -- 64 cycles during which the matrix pipe takes nothing else from this
// wave -- and the group's 4x4x4_4b; req.slot gets the accumulator the former wrote and the operand the latter reads.
struct NoRequest {
  template <int SLOT> __device__ __forceinline__ void slot(d4&, double&) {}
};
template <int S, int I, int G, class REQ>   // site groups G .. 3 of step I (a recursion: the slot is a template argument)
__device__ __forceinline__ void mfma16_groups(double& p0, double& t0, const double (&x)[S], d4 (&acc)[4], double (&y)[S], REQ& req) {
  if constexpr (G < 4) {
    const double xi = x[vreg<S, 4, false>(I, G)];
    double& y4 = y[vreg<S, 4, false>(S / 4 - 1, G)];
    acc[G] = __builtin_amdgcn_mfma_f64_16x16x4f64(p0, xi, I == 0 ? (d4){0.0, 0.0, 0.0, 0.0} : acc[G], 0, 0, 0);
    req.template slot<4 * I + G>(acc[G], t0);
    y4 = __builtin_amdgcn_mfma_f64_4x4x4f64(t0, xi, I == 0 ? 0.0 : y4, 0, 0, 0);
    mfma16_groups<S, I, G + 1>(p0, t0, x, acc, y, req);
  }
}
template <int S, bool TR, int I, class REQ>
__device__ __forceinline__ void mfma16_steps(const uint8_t* pan0, const uint8_t* tile0, double p0, double t0, const double (&x)[S],
                                             d4 (&acc)[4], double (&y)[S], REQ& req) {
  constexpr int NB = S / 4;
  if constexpr (I < NB) {
    double p1 = 0.0, t1 = 0.0;
    if constexpr (I + 1 < NB) {
      p1 = *reinterpret_cast<const double*>(pan0 + mfma16_a_offset(0, I + 1, TR, S));
      t1 = *reinterpret_cast<const double*>(tile0 + mfma_tile<S, TR, false>((NB - 1) * NB + I + 1) * 128);
      // (the reads stay in front of the statement, and this step's operands are its outputs: hipcc otherwise moves the
      // step's matrix instructions in front of the reads and waits for them right behind)
      asm volatile("" : "+v"(p0), "+v"(t0) :: "memory");
    }
    mfma16_groups<S, I, 0>(p0, t0, x, acc, y, req);
    mfma16_steps<S, TR, I + 1>(pan0, tile0, p1, t1, x, acc, y, req);
  }
}

template <int S, bool TR, int NG, bool DIAG, int Q>
__device__ __forceinline__ void mfma_steps(const uint8_t* tile0, double m0, double m1, double m2, const double (&x)[S / 4 * NG],
                                           double (&y)[S / 4 * NG]) {
  constexpr int NB = S / 4, NT = DIAG ? NB : NB * NB;
  if constexpr (Q < NT) {
    constexpr int o = DIAG ? Q : Q / NB, i = DIAG ? Q : Q % NB;
    double m3 = 0.0;
    if constexpr (Q + 3 < NT) {
      m3 = *reinterpret_cast<const double*>(tile0 + mfma_tile<S, TR, DIAG>(Q + 3) * 128);
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
      y[o * NG + g] = __builtin_amdgcn_mfma_f64_4x4x4f64(m0, x[i * NG + g], (DIAG || i == 0) ? 0.0 : y[o * NG + g], 0, 0, 0);
    mfma_steps<S, TR, NG, DIAG, Q + 1>(tile0, m1, m2, m3, x, y);
  }
}

// y = M x (TR = false) or y = M^T x (TR = true) with M = the packed matrix staged in buf (already landed)
template <int S, bool TR, int NG, bool DIAG, class REQ>
__device__ __forceinline__ void matvec_stage(const uint8_t* buf, int lane, const double (&x)[S / 4 * NG],
                                             double (&y)[S / 4 * NG], REQ& req) {
  static_assert(S % 4 == 0, "state count must be a multiple of 4");
  constexpr int NT = DIAG ? S / 4 : (S / 4) * (S / 4);
  // element (row r, column c) of a packed tile sits at (4 r + c) * 8; the A slot of lane l is row l & 3, column l >> 4
  // (transposed product: the transposed tile, i.e. row l >> 4, column l & 3)
  const uint8_t* tile0 = buf + (TR ? (4 * (lane >> 4) + (lane & 3)) : (4 * (lane & 3) + (lane >> 4))) * 8;
  if constexpr (kMfma16<S, NG, DIAG>) {
    const uint8_t* pan0 = buf + mfma16_a_offset(lane, 0, TR, S);
    d4 acc[4];
    mfma16_steps<S, TR, 0>(pan0, tile0, *reinterpret_cast<const double*>(pan0),
                           *reinterpret_cast<const double*>(tile0 + mfma_tile<S, TR, false>((S / 4 - 1) * (S / 4)) * 128), x, acc, y, req);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int sb = 0; sb < 4; ++sb) y[vreg<S, NG, DIAG>(sb, g)] = acc[g][sb];
  } else {
    mfma_steps<S, TR, NG, DIAG, 0>(tile0, *reinterpret_cast<const double*>(tile0 + mfma_tile<S, TR, DIAG>(0) * 128),
                         NT > 1 ? *reinterpret_cast<const double*>(tile0 + mfma_tile<S, TR, DIAG>(1) * 128) : 0.0,
                         NT > 2 ? *reinterpret_cast<const double*>(tile0 + mfma_tile<S, TR, DIAG>(2) * 128) : 0.0, x, y);
  }
}

// Message of a leaf edge from the transposed operator staged in buf ([z][x] = M[x][z], rows >= S: ambiguity ids):
// lane l needs, for each site group g, element 4 sb + (l >> 4) of the row named by the symbol of site 16 g + (l & 15).
// SET out = row, MUL out = row o in (in may be out), DOT returns sum_x in[x] * row[x] of site l (reduce_sites).
enum { LEAF_SET = 0, LEAF_MUL = 1, LEAF_DOT = 2 };
// r[g]: the lane's values of site group g's row (rows are stored state-in-tile major: state 4 sb + s4 at position
// s4 * NB + sb, cmx_layout.h: leaf_col).  Per site group the row values and their use: the reads of the next group do not
// depend on anything computed for the previous one.
template <int S, int MODE, int NG, bool DIAG>
__device__ __forceinline__ double rows_apply(const double* const (&r)[NG], const double (&in)[S / 4 * NG], double (&out)[S / 4 * NG]) {
  constexpr int NB = S / 4;
  double part[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    part[g] = 0.0;
    double v[NB];
#pragma unroll
    for (int sb = 0; sb < NB; ++sb) v[sb] = r[g][sb];
#pragma unroll
    for (int sb = 0; sb < NB; ++sb) {
      const int X = vreg<S, NG, DIAG>(sb, g);
      if (MODE == LEAF_SET) out[X] = v[sb];
      else if (MODE == LEAF_MUL) out[X] = v[sb] * in[X];
      else part[g] = __builtin_fma(in[X], v[sb], part[g]);
    }
  }
  if (MODE != LEAF_DOT) return 0.0;
  return reduce_sites<NG>(part);
}
// where the lane's values of row `row` of a staged leaf operator or cherry table start
template <int S>
__device__ __forceinline__ const double* stage_row(const uint8_t* buf, unsigned row, int lane) {
  return reinterpret_cast<const double*>(buf + row * (leaf_row_stride(S) * 8)) + (lane >> 4) * (S / 4);
}
template <int S, int MODE, int NG, bool DIAG>
__device__ __forceinline__ double leaf_apply(const uint8_t* buf, const uint8_t* codes /* slot + 4 * (lane & 15) */, int lane,
                                             const double (&in)[S / 4 * NG], double (&out)[S / 4 * NG]) {
  // all symbols first (one LDS round trip): one dword per LANE in the slot, group g at 64 / NG * g
  unsigned code[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) code[g] = codes[g * (256 / NG)];
  const double* r[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g)
    r[g] = stage_row<S>(buf, code[g] < (unsigned)MatStage<S>::NROW ? code[g] : (unsigned)(MatStage<S>::NROW - 1), lane);
  return rows_apply<S, MODE, NG, DIAG>(r, in, out);
}

// Row of a cherry table (cmx_walk.h): the row is named by the symbols of the cherry's two leaves, 4 * symbol(l1) + symbol(l2)
// (fully resolved alignments only: both symbols are states of the 4-letter alphabet), the columns are a leaf row's.
template <int S, int MODE, int NG, bool DIAG>
__device__ __forceinline__ double cherry_apply(const uint8_t* buf, const uint8_t* codes1, const uint8_t* codes2, int lane,
                                               const double (&in)[S / 4 * NG], double (&out)[S / 4 * NG]) {
  unsigned c1[NG], c2[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) { c1[g] = codes1[g * (256 / NG)]; c2[g] = codes2[g * (256 / NG)]; }
  const double* r[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) r[g] = stage_row<S>(buf, ((c1[g] & 3u) << 2) | (c2[g] & 3u), lane);
  return rows_apply<S, MODE, NG, DIAG>(r, in, out);
}

// ------------------------------------------------------------------------------------------------ small helpers
// Workspace vectors are stored as [S/2][64 lanes][2 doubles]: one 16-byte access per lane and row, 1 KiB per
// wave-instruction.  An odd length (16-site tasks: S = 5) ends with a row of single doubles.
// (Round 4 tried [S][64] with 64-bit accesses: hipcc puts v_mov copies and the s_waitcnt for them right behind the 128-bit
// loads at 3 of the 5 load sites of map_kernel<20, null> -- the loaded quads do not match the registers the vector's phi
// with the other arms of the child switch got -- and 64-bit loads remove copies and early waits alike.  Twice the VMEM
// instructions cost what that saved: target launch 445 -> 450 ms, same box, profiles/r04_ab_workspace_64bit.log.)
//
// ---- Cache policy of the per-wave state.  Every global access of state a wave keeps for itself goes through
// state_load / state_store (store_vec / load_vec for whole vectors) with a compile-time policy; StatePolicy names the
// policy of each class of state per instantiation (DESIGN.md 4.1 has the table with every reader):
//   V  workspace vectors (DevWalk::store / load)          P  per-class counts `part` (dot3 / ldot / cdot, the epilogue's loads)
//   T  final counts and per-site scalars (the epilogue's tile / cnt0 / cnt1 stores, observed mode's copy loop)
//   S  class-split mode's split_part / split_lc
// Operators (LDS-DMA, plain) and symbols (sc0 sc1) are not state and keep their own forms.
// RULE: a location stored with a form that may bypass the CU's L1 (anything but kPolPlain) is loaded ONLY with a form
// that bypasses the L1 too (kPolNt), by every reader in every kernel.  A slot is rewritten in every class pass and
// read back by the same wave: a store that does not update the L1 followed by a plain load could be served the
// previous pass's line.  The walk's other traffic evicts that line almost always, so no test can show a violation:
// the rule holds by construction (StatePolicy's static_asserts) or not at all.
// Loads stay compiler-visible (plain or __builtin_nontemporal_load: hipcc counts them, os.vs / wait_vm keep their exact
// counts); a vector is kVecInstrs VMEM instructions under every policy.
enum { kPolPlain = 0, kPolNt = 1 };   // kPolNt: `nt` -- streaming in the L2, past the L1 (DESIGN.md 8.8 has the forms that lost)
template <int POL, class T>
__device__ __forceinline__ T state_load(const T* p) {
  static_assert(POL == kPolPlain || POL == kPolNt, "load forms");
  if constexpr (POL == kPolNt) return __builtin_nontemporal_load(p);
  else return *p;
}
template <int POL, class T>
__device__ __forceinline__ void state_store(const T v, T* p) {   // (value first: evaluated in an assignment's order)
  static_assert(POL == kPolPlain || POL == kPolNt, "store forms");
  if constexpr (POL == kPolNt) __builtin_nontemporal_store(v, p);
  else *p = v;
}
template <int S, int MODE, int FUSE, int NG>
struct StatePolicy {
  // V streams through the L2 in the 64-site and 16-site protein walks (each byte written once and read once, 10 KiB per
  // vector and wave); the class-fused and 4-state instantiations keep plain accesses (not measured: their device code is
  // the parent's).  P, T and S stay plain everywhere: `nt` stores of P or of the pattern tiles gained nothing (DESIGN.md
  // 8.8), cnt0 / cnt1 are read back by pair_stat_strided and split_part / split_lc by map_finalize_kernel with plain loads.
  static constexpr bool kOn = S == 20 && FUSE == 1;
  static constexpr int v_store = kOn ? kPolNt : kPolPlain, v_load = v_store;
  static constexpr int p_store = kPolPlain, p_load = kPolPlain;
  static constexpr int t_store = kPolPlain, t_load = kPolPlain;
  static constexpr int split_store = kPolPlain;
  static_assert(v_store == kPolPlain || v_load != kPolPlain, "RULE: V");
  static_assert(p_store == kPolPlain || p_load != kPolPlain, "RULE: P");
  static_assert(t_store == kPolPlain && split_store == kPolPlain, "RULE: T and S have readers outside this file with plain loads");
};

template <int S, int POL>
__device__ __forceinline__ void load_vec(const double* p /* slice base */, double (&v)[S], int lane) {
  p += 2 * lane;
#pragma unroll
  for (int i = 0; i < S / 2; ++i) {
    const d2 t = state_load<POL>(reinterpret_cast<const d2*>(p + (size_t)i * 2 * kWave));
    v[2 * i] = t[0];
    v[2 * i + 1] = t[1];
  }
  if constexpr (S % 2) v[S - 1] = state_load<POL>(p + (size_t)(S / 2) * 2 * kWave - lane);
}
template <int S, int POL>
__device__ __forceinline__ void store_vec(double* p, const double (&v)[S], int lane) {
  p += 2 * lane;
#pragma unroll
  for (int i = 0; i < S / 2; ++i) {
    d2 t;
    t[0] = v[2 * i];
    t[1] = v[2 * i + 1];
    state_store<POL>(t, reinterpret_cast<d2*>(p + (size_t)i * 2 * kWave));
  }
  if constexpr (S % 2) state_store<POL>(v[S - 1], p + (size_t)(S / 2) * 2 * kWave - lane);
}

// ------------------------------------------------------------------------------------------------ mapping core
extern __shared__ __attribute__((aligned(16))) uint8_t cmx_smem[];

// per-visited-node record of the tree walk (cmx_walk.h): 16 ints, one scalar load
typedef int cmx_i16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void sload_rec(cmx_cint p, cmx_i16& r) {
  asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(p) : "memory");
}

struct ConstModel {
  cmx_cint nrec, msched;
  cmx_cdbl rates, probs;
  // tables: the cherry-table walk's operator stream (class-fused nucleotide models on resolved alignments)
  __device__ __forceinline__ explicit ConstModel(const DevModel& m, bool tables = false)
      : nrec((cmx_cint)m.nrec), msched((cmx_cint)(tables ? m.msched_r : m.msched)), rates((cmx_cdbl)m.rates),
        probs((cmx_cdbl)m.probs) {}
};
// Operator-stream bookkeeping of a wave (wave-uniform, lives across site blocks): one struct per way an op learns how long
// to wait (CountedWalk, PlannedWalk below).
// The counted walk: vs counts the VMEM instructions this code issued and knows about (DMA rows, vector stores and
// loads); an asynchronous transfer remembers vs right after its issue,
// and "wait for X" is s_waitcnt vmcnt(vs - X_seq): VMEM completes in order, so the instructions issued after X may stay
// in flight.  Instructions that are not counted only make the wait stricter.
struct CountedState {   // (the members keep their order: the class-fused kernels' text depends on it)
  int pre_mat;       // the NEXT op's operator, element offset in a class block
  int pre_tx;        // op-stream entry of the NEXT op, loaded one op early (its latency hides behind the current op)
  unsigned par;      // stage buffer / code slot of the current operator op
  unsigned vs;       // counted VMEM instructions issued so far
  unsigned cur_seq;  // vs right after the current operator op's operator (and symbols) were requested
};
// The planned walk (the 64-site protein walk, kMfma16) counts nothing at run time: the distance vs - cur_seq of an op is a function of the tree,
// the LDS-slot plan and the op's place in the stream, the host records it per stream entry (cmx_layout.h: wait plan; proved
// against a model of this queue by verify_walk before a context exists) and the entry carries the immediate.  Its stream
// entry is a PlanEntry: pre_off / pre_tx / pre_w.
struct PlannedState {
  int pre_tx;        // op-stream entry of the NEXT op, loaded one op early (its latency hides behind the current op)
  unsigned par;      // stage buffer / code slot of the current operator op
  long long pre_off; // byte offset of the NEXT op's operator from the pass's class block
  int pre_w;         // the vmcnt immediate of the CURRENT op's wait (it travels with the next op's entry)
};
// an entry as the scalar load sees it: four dwords (off low, off high, tx, w), read through the constant address space
typedef int cmx_i4 __attribute__((ext_vector_type(4)));
typedef const cmx_i4 __attribute__((address_space(4)))* cmx_cplan;
static_assert(offsetof(PlanEntry, off) == 0 && offsetof(PlanEntry, tx) == 8 && offsetof(PlanEntry, w) == 12, "dwords of an entry");
__device__ __forceinline__ void plan_entry(cmx_cplan p, PlannedState& os) {
  const cmx_i4 q = *p;
  os.pre_off = (long long)(((unsigned long long)(unsigned)q[1] << 32) | (unsigned)q[0]);
  os.pre_tx = q[2];
  os.pre_w = q[3];
}

// Device backend of the tree walk (cmx_walk.h): registers R0..R3 are S-vectors of the wave's sites in the matrix-core
// layout.  The walk names what it wants, workspace slots included; the operator stream (m.msched) -- recorded from the
// same walk on the host and checked numerically there -- says where the operators are.
// RESOLVED: every symbol of the alignment is a state (the null's simulated or supplied alignments): leaf ops then stage the
// S0 state rows of the transposed operator only, not its ambiguity rows
// WalkRegs is what both backends share: the register file and everything that does not care how an op learns how long to
// wait.  CountedWalk and PlannedWalk add the operator ops; DevWalk names the one an instantiation runs.
template <int S, int FUSE, int NG, bool RESOLVED, class POL>
struct WalkRegs {
  static constexpr int VL = S / 4 * NG, kSites = 16 * NG;
  static constexpr bool DIAG = FUSE > 1 && S / FUSE == 4;
  static constexpr int kProductBytes = DIAG ? (S / 4) * 128 : MatStage<S>::BYTES;                      // diagonal tiles come first
  static constexpr int kLeafBytes = RESOLVED ? (S / FUSE) * leaf_row_stride(S) * 8 : MatStage<S>::BYTES;
  static constexpr int kVecInstrs = (VL + 1) / 2;   // VMEM instructions of one workspace vector
  static constexpr bool kCherryTables = RESOLVED && DIAG;   // cmx_walk.h: cset / cdot instead of a cherry's operator ops
  static constexpr bool kCherryRows = FUSE == 1;            // cmx_walk.h: a cherry's outside visit keeps its leaf rows in registers
  // cmx_walk.h: one workspace vector per wave stays in LDS where the records say so (the 64-site protein walk in all its
  // modes; the 16-site shape shares the records and ignores the bits, like every backend without a slot)
  static constexpr bool kLdsSlot = map_lds_slot(S, FUSE, NG);
  double R0[VL], R1[VL], R2[VL], R3[VL];
  const ConstModel& cm;
  const double* pi;            // root frequencies (vector loads: lane-dependent index)
  double *wsM, *wsU, *pcnt;
  const uint8_t* gcodes;
  size_t gstride;
  uint8_t *stage, *cslot, *cslot2, *vslot;
  uint32_t lds_stage, lds_codes, lds_codes2;
  int lane;
  double pc;
  double Lg[FUSE];

  __device__ __forceinline__ explicit WalkRegs(const ConstModel& cm_) : cm(cm_) {}

  // The lane index as an opaque value: address arithmetic built on it is redone at every use (a few VALU instructions)
  // instead of being hoisted out of the walk as a dozen loop-invariant 64-bit per-lane addresses, which the register
  // allocator then spills -- and every reload of a spilled address is a scratch load whose vmcnt(0) wait drains the
  // DMAs in flight.
  __device__ __forceinline__ int vlane() const {
    int l = lane;
    asm volatile("" : "+v"(l));
    return l;
  }
  // site of the lane inside the wave's block (see map_sites_wave)
  __device__ __forceinline__ int vsidx() const {
    const int l = vlane();
    return NG == 4 ? l : (l & 15);
  }
  // where an S-vector keeps state tile sb of site group g (vreg)
  static constexpr int vr(int sb, int g) { return vreg<S, NG, DIAG>(sb, g); }
  template <int I>
  __device__ __forceinline__ double (&reg())[VL] {
    if constexpr (I == 0) return R0;
    else if constexpr (I == 1) return R1;
    else if constexpr (I == 2) return R2;
    else return R3;
  }
  __device__ __forceinline__ void begin_pass() {
#pragma unroll
    for (int g = 0; g < FUSE; ++g) Lg[g] = 0.0;
  }
  __device__ __forceinline__ void rec(int v, int (&r)[16]) const {
    cmx_i16 q;
    sload_rec(cm.nrec + v * 16, q);
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = q[i];
  }
  // tells the compiler a register's old value is dead here (defines it without an instruction)
  // (ONE asm statement: hipcc puts an `s_nop 0` behind every inline asm, and a wave issues one instruction per four
  // cycles -- sixty one-element kills per visited node were sixty issue slots of the walk's chain: target launch -0.6 %, same box)
  template <int R>
  __device__ __forceinline__ void kill() {
    double(&r)[VL] = reg<R>();
    static_assert(VL == 4 || VL == 5 || VL == 16 || VL == 20, "kill() names every element in one statement");
    if constexpr (VL == 5)
      asm volatile("" : "=v"(r[0]), "=v"(r[1]), "=v"(r[2]), "=v"(r[3]), "=v"(r[4]));
    else if constexpr (VL == 4)
      asm volatile("" : "=v"(r[0]), "=v"(r[1]), "=v"(r[2]), "=v"(r[3]));
    else if constexpr (VL == 16)
      asm volatile("" : "=v"(r[0]), "=v"(r[1]), "=v"(r[2]), "=v"(r[3]), "=v"(r[4]), "=v"(r[5]), "=v"(r[6]), "=v"(r[7]), "=v"(r[8]),
                        "=v"(r[9]), "=v"(r[10]), "=v"(r[11]), "=v"(r[12]), "=v"(r[13]), "=v"(r[14]), "=v"(r[15]));
    else
      asm volatile("" : "=v"(r[0]), "=v"(r[1]), "=v"(r[2]), "=v"(r[3]), "=v"(r[4]), "=v"(r[5]), "=v"(r[6]), "=v"(r[7]), "=v"(r[8]),
                        "=v"(r[9]), "=v"(r[10]), "=v"(r[11]), "=v"(r[12]), "=v"(r[13]), "=v"(r[14]), "=v"(r[15]), "=v"(r[16]),
                        "=v"(r[17]), "=v"(r[18]), "=v"(r[19]));
  }
  // what an operator op does once its operator has landed in buf: a product (req: what it issues in its gaps) ...
  template <int SRC, int DST, bool TR, class REQ>
  __device__ __forceinline__ void product(const uint8_t* buf, REQ& req) {
    matvec_stage<S, TR, NG, DIAG>(buf, vlane(), reg<SRC>(), reg<DST>(), req); asm volatile("" :: "v"(reg<DST>()[0]), "v"(reg<DST>()[VL - 1]));
  }
  // ... a leaf op, or a cherry-table op (cmx_walk.h): the table is staged like a leaf operator, its row named by two
  // symbols.  par: the op's code slot
  template <bool CHERRY, int MODE, int SRC, int DST>
  __device__ __forceinline__ double rows(const uint8_t* buf, unsigned par) {
    const int vl = vlane();
    const uint8_t* codes = cslot + par * kCodeSlotBytes + 4 * (vl & 15);
    double tot;
    if constexpr (CHERRY) tot = cherry_apply<S, MODE, NG, DIAG>(buf, codes, cslot2 + par * kCodeSlotBytes + 4 * (vl & 15), vl, reg<SRC>(), reg<DST>());
    else tot = leaf_apply<S, MODE, NG, DIAG>(buf, codes, vl, reg<SRC>(), reg<DST>());
    asm volatile("" :: "v"(tot), "v"(reg<DST>()[0]), "v"(reg<DST>()[VL - 1]));
    return tot;
  }
  // per-class count of row `row` of this lane's site (P; class-split mode: S)
  __device__ __forceinline__ void part_store(int row, double v) { state_store<POL::p_store>(v, pcnt + ((size_t)row * kSites + vsidx())); }
  // workspace vector -> register: global loads (POL::v_load) straight into the destination register, which the walk has
  // declared dead (kill) long before -- in the outside pass the two sibling messages of a node are requested before the
  // first product and first read after it, so their latency hides behind ~100 MFMAs without a landing buffer.  The
  // loads are compiler-visible (hipcc waits for them before the first use).
  template <int D>
  __device__ __forceinline__ void load(int arr, int slot) {
    const int vl = vlane();
    load_vec<VL, POL::v_load>((arr ? wsU : wsM) + (size_t)slot * VL * kWave, reg<D>(), vl);
  }
  template <int SRC>
  __device__ __forceinline__ void store(int arr, int slot) {
    const int vl = vlane();
    store_vec<VL, POL::v_store>((arr ? wsU : wsM) + (size_t)slot * VL * kWave, reg<SRC>(), vl);
  }
  // LDS slot (kLdsSlot): the vector in the workspace layout [VL/2][64 lanes][2], one 16-byte access per lane and row (no
  // bank conflict).  Plain accesses: the compiler's own lgkmcnt waits cover them, and they are not VMEM, so os.vs does
  // not count them.  Through a pointer that SAYS local memory: where the walk chooses between lstore and store (lload and
  // load) on a record's flag, hipcc otherwise sinks the two arms' accesses into one run of flat_store / flat_load on a
  // selected generic address -- the vector's LDS transfers become VMEM instructions the wait plan has not counted, and
  // the HBM arm loses its cache policy.
  template <int D>
  __device__ __forceinline__ void lload(int, int) {
    static_assert(kLdsSlot && VL % 2 == 0, "LDS slot");
    const __attribute__((address_space(3))) d2* p = (const __attribute__((address_space(3))) d2*)vslot + vlane();
#pragma unroll
    for (int i = 0; i < VL / 2; ++i) {
      const d2 t = p[i * kWave];
      reg<D>()[2 * i] = t[0];
      reg<D>()[2 * i + 1] = t[1];
    }
  }
  template <int SRC>
  __device__ __forceinline__ void lstore(int, int) {
    static_assert(kLdsSlot && VL % 2 == 0, "LDS slot");
    __attribute__((address_space(3))) d2* p = (__attribute__((address_space(3))) d2*)vslot + vlane();
#pragma unroll
    for (int i = 0; i < VL / 2; ++i) {
      d2 t;
      t[0] = reg<SRC>()[2 * i];
      t[1] = reg<SRC>()[2 * i + 1];
      p[i * kWave] = t;
    }
  }
  template <int SRC> __device__ __forceinline__ void lcopy(int arr, int slot) { lstore<SRC>(arr, slot); }
  template <int D, int SRC> __device__ __forceinline__ void mov() {
#pragma unroll
    for (int x = 0; x < VL; ++x) reg<D>()[x] = reg<SRC>()[x];
  }
  template <int D, int SRC> __device__ __forceinline__ void mul() {
#pragma unroll
    for (int x = 0; x < VL; ++x) reg<D>()[x] *= reg<SRC>()[x];
  }
  template <int D, int A, int B> __device__ __forceinline__ void prod() {
#pragma unroll
    for (int x = 0; x < VL; ++x) reg<D>()[x] = reg<A>()[x] * reg<B>()[x];
  }
  __device__ __forceinline__ void mulup() {
#pragma unroll
    for (int x = 0; x < VL; ++x) { R1[x] *= R3[x]; R2[x] *= R3[x]; }
  }
  template <int D> __device__ __forceinline__ void setpi() {
#pragma unroll
    for (int sb = 0; sb < S / 4; ++sb) {
      const double pv = pi[(4 * sb + (vlane() >> 4)) % (S / FUSE)];
#pragma unroll
      for (int g = 0; g < NG; ++g) reg<D>()[vr(sb, g)] = pv;
    }
  }
  template <int SRC> __device__ __forceinline__ void rootl() {
    // lane l holds state 4 sb + (l >> 4) of its four sites: weight it with that state's frequency
    if constexpr (FUSE == 1) {
      double p_[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) p_[g] = 0.0;
#pragma unroll
      for (int sb = 0; sb < S / 4; ++sb) {
        const double pv = pi[4 * sb + (vlane() >> 4)];
#pragma unroll
        for (int g = 0; g < NG; ++g) p_[g] = __builtin_fma(pv, reg<SRC>()[vr(sb, g)], p_[g]);
      }
      Lg[0] = reduce_sites<NG>(p_);
    } else {   // one 4-state tile per fused class
      const double pv = pi[vlane() >> 4];
#pragma unroll
      for (int sb = 0; sb < FUSE; ++sb) {
        double p_[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) p_[g] = pv * reg<SRC>()[vr(sb, g)];
        Lg[sb] = reduce_sites<NG>(p_);
      }
    }
  }
  __device__ __forceinline__ void dot3(int row) {
    double p_[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) p_[g] = 0.0;
#pragma unroll
    for (int sb = 0; sb < S / 4; ++sb)
#pragma unroll
      for (int g = 0; g < NG; ++g) p_[g] = __builtin_fma(R3[vr(sb, g)] * R1[vr(sb, g)], R2[vr(sb, g)], p_[g]);
    part_store(row, pc * reduce_sites<NG>(p_));
  }
};

// The counted walk: every instantiation but the 64-site protein walk.
template <int S, int FUSE, int NG, bool RESOLVED, class POL>
struct CountedWalk : WalkRegs<S, FUSE, NG, RESOLVED, POL> {
  using Regs = WalkRegs<S, FUSE, NG, RESOLVED, POL>;
  using State = CountedState;
  using Regs::VL, Regs::DIAG, Regs::kProductBytes, Regs::kLeafBytes, Regs::kVecInstrs, Regs::kCherryTables;
  using Regs::cm, Regs::gcodes, Regs::gstride, Regs::stage, Regs::lds_stage, Regs::lds_codes, Regs::lds_codes2, Regs::pc, Regs::vlane, Regs::part_store;
  static_assert(!kMfma16<S, NG, DIAG>, "the 64-site protein walk: PlannedWalk");
  static constexpr bool kCherryMsg = false;
  static constexpr int kCherryBytes = 16 * leaf_row_stride(S) * 8;   // a table's 16 rows (one per symbol pair)
  static_assert(kCherryBytes <= MatStage<S>::BYTES, "a cherry table fits a stage buffer");
  State& os;
  int nmv, mi;                       // ops of a pass, op of the pass
  const double *mat_c, *mat_after;   // class blocks of the pass and of the pass that follows
  int c, c_end;

  // (the launcher guarantees m.msched_r with cherry tables)
  __device__ __forceinline__ CountedWalk(State& os_, const ConstModel& cm_, const MapArgs& a)
      : Regs(cm_), os(os_), nmv(kCherryTables ? a.m.nmv_r : a.m.nmv) {}
  // operators of class c and of the class of the pass that follows (its first operator is requested by our last op)
  __device__ __forceinline__ void begin_class(const MapArgs& a, int c_, int c_end_, int c_after) {
    const DevModel& m = a.m;
    c = c_;
    c_end = c_end_;
    mat_c = m.MAT + (size_t)c * m.MC * MatStage<S>::UNIT;
    mat_after = m.MAT + (size_t)((c + 1 < c_end) ? c + 1 : c_after) * m.MC * MatStage<S>::UNIT;
    mi = 0;
  }
  // One operator op has two halves.  The request: the operator (and symbols) of the NEXT op of the stream -- entry mi + 1,
  // or entry 0 of the next class / next site block -- into the other buffer, and the stream entry two ops ahead.  The
  // wait: for this op's operator; it returns its buffer.  op_begin requests, then waits: a leaf op has no matrix
  // instructions to hide the request behind, and every product but those of the 64-site protein walk keeps this order.
  // (One function on purpose: as two, op_request and op_wait, hipcc orders a few instructions of the request otherwise in
  // thirteen kernels that are to keep their text.)  The 64-site protein walk does not come here: its leaf ops run
  // leaf_begin, its products wait (wait_planned_product) and then request from inside the product (ProductRequest).
  // The request overwrites the other stage buffer and code slot, whose last readers are the LDS reads of the op before:
  // op_begin waits for them (lgkmcnt(0)) first.
  __device__ __forceinline__ const uint8_t* op_begin(unsigned& nseq) {
    const bool more = (mi + 1 < nmv);
    const int emat = os.pre_mat, etx = os.pre_tx;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the LDS reads of the other buffer are done
    unsigned issued;
    {
      const double* src = (more ? mat_c : mat_after) + emat;   // element offset, premultiplied on the host
      const uint32_t dst = lds_stage + (os.par ^ 1u) * MatStage<S>::BYTES;
      if constexpr (kProductBytes == MatStage<S>::BYTES && kLeafBytes == MatStage<S>::BYTES) {
        mat_dma_l<S>(src, dst, vlane());
        issued = MatStage<S>::ROWS;
      } else if (etx >= 0) {   // (wave-uniform: the next op is a leaf op -- or a cherry-table op)
        if (kCherryTables && (etx & kCherryFlag)) {
          mat_dma_part<kCherryBytes>(src, dst, vlane());
          issued = MatPart<kCherryBytes>::ROWS;
        } else {
          mat_dma_part<kLeafBytes>(src, dst, vlane());
          issued = MatPart<kLeafBytes>::ROWS;
        }
      } else {
        mat_dma_part<kProductBytes>(src, dst, vlane());
        issued = MatPart<kProductBytes>::ROWS;
      }
    }
    if (etx >= 0 && (more || c + 1 < c_end)) {
      if (kCherryTables && (etx & kCherryFlag)) {
        code_dma_l(gcodes + (size_t)cherry_taxon1(etx) * gstride, lds_codes + (os.par ^ 1u) * kCodeSlotBytes);
        code_dma_l(gcodes + (size_t)cherry_taxon2(etx) * gstride, lds_codes2 + (os.par ^ 1u) * kCodeSlotBytes);
        issued += 2;
      } else {
        code_dma_l(gcodes + (size_t)etx * gstride, lds_codes + (os.par ^ 1u) * kCodeSlotBytes);
        issued += 1;
      }
    }
    {  // entry two ops ahead; the stream carries its first two entries again after the last (no wrap test)
      const int i2 = more ? mi + 2 : 1;
      os.pre_mat = cm.msched[2 * i2];
      os.pre_tx = cm.msched[2 * i2 + 1];
    }
    wait_vm<S, VL>((int)(os.vs - os.cur_seq + issued));
    os.vs += issued;
    nseq = os.vs;
    return stage + os.par * MatStage<S>::BYTES;
  }
  __device__ __forceinline__ void op_end(unsigned nseq) {
    os.par ^= 1u;
    os.cur_seq = nseq;
    ++mi;
  }
  template <int SRC, int DST, bool TR>
  __device__ __forceinline__ void mv(int, int) {
    unsigned nseq;
    const uint8_t* buf = op_begin(nseq);
    NoRequest req;
    this->template product<SRC, DST, TR>(buf, req);
    op_end(nseq);
  }
  template <bool CHERRY, int MODE, int SRC, int DST>
  __device__ __forceinline__ double row_op() {
    unsigned nseq;
    const uint8_t* buf = op_begin(nseq);
    const double tot = this->template rows<CHERRY, MODE, SRC, DST>(buf, os.par);
    op_end(nseq);
    return tot;
  }
  template <int D> __device__ __forceinline__ void lset(int, int) { (void)row_op<false, LEAF_SET, D, D>(); }
  template <int SRC, int D> __device__ __forceinline__ void lmul(int, int) { (void)row_op<false, LEAF_MUL, SRC, D>(); }
  template <int SRC> __device__ __forceinline__ void ldot(int, int, int row) {
    const double tot = row_op<false, LEAF_DOT, SRC, SRC>();
    part_store(row, pc * tot);
  }
  template <int D> __device__ __forceinline__ void cset(int, int, int) { (void)row_op<true, LEAF_SET, D, D>(); }
  template <int SRC> __device__ __forceinline__ void cdot(int, int, int, int, int row) {
    const double tot = row_op<true, LEAF_DOT, SRC, SRC>();
    part_store(row, pc * tot);
  }
  // workspace vectors are counted in vs like every VMEM instruction this code issues, so that the counted waits of the
  // operator stream let them stay in flight
  template <int D>
  __device__ __forceinline__ void load(int arr, int slot) {
    Regs::template load<D>(arr, slot);
    os.vs += kVecInstrs;
  }
  template <int SRC>
  __device__ __forceinline__ void store(int arr, int slot) {
    Regs::template store<SRC>(arr, slot);
    os.vs += kVecInstrs;
  }
};

// The planned walk: the 64-site protein walk (kMfma16).  The host has counted every VMEM instruction, workspace vectors
// included (cmx_layout.h: kPlanVec), so load / store are WalkRegs's.
// MSG: the walk gathers an inlined cherry's message from the cherry message table (cmx_walk.h: kCherryMsg)
template <int S, int FUSE, int NG, bool RESOLVED, class POL, bool MSG>
struct PlannedWalk : WalkRegs<S, FUSE, NG, RESOLVED, POL> {
  using Regs = WalkRegs<S, FUSE, NG, RESOLVED, POL>;
  using State = PlannedState;
  using Regs::VL, Regs::DIAG, Regs::kProductBytes, Regs::kLeafBytes, Regs::kCherryTables, Regs::vr;
  using Regs::gcodes, Regs::gstride, Regs::stage, Regs::lds_stage, Regs::lds_codes, Regs::pc, Regs::vlane, Regs::part_store;
  static_assert(kMfma16<S, NG, DIAG>, "every other instantiation: CountedWalk");
  static constexpr bool kCherryMsg = MSG;   // cmx_walk.h: a cherry's message is a gathered table row
  static_assert(!MSG || (RESOLVED && !kCherryTables && S == 20), "the message table serves the 64-site protein walk on resolved alignments");
  State& os;
  const uint8_t* op_base;      // the pass's class block (wave-uniform); an operator is op_base + its entry's offset
  cmx_cplan sp;                // the stream entry the next op loads; set at the pass boundary, bumped per op
  const uint8_t* cmsg;         // kCherryMsg: the message tables of the pass's class, table of cherry i at i * C * kCherryMsgTableBytes (wave-uniform)
  cmx_cint cmsg_ref;           // kCherryMsg: the table's node index (cmx_layout.h)
  size_t cmsg_stride;          // kCherryMsg: bytes from a cherry's table to the next cherry's

  __device__ __forceinline__ PlannedWalk(State& os_, const ConstModel& cm_, const MapArgs& a) : Regs(cm_), os(os_) {
    if constexpr (MSG) {
      cmsg_ref = (cmx_cint)reinterpret_cast<const int*>(a.cherry_msg);
      cmsg_stride = (size_t)a.m.C * kCherryMsgTableBytes;
    }
  }
  // the pass's class block, and the copy of the stream whose entries behind the last one lead to the pass that follows
  // (cmx_layout.h: planned_stream_copy) -- the wrap is settled here, no op knows about it.  MSG: the planned walk over the
  // resolved stream, and the class's message tables
  __device__ __forceinline__ void begin_class(const MapArgs& a, int c, int c_end, int c_after) {
    const DevModel& m = a.m;
    const bool last = c + 1 >= c_end;
    op_base = reinterpret_cast<const uint8_t*>(m.MAT + (size_t)c * m.MC * MatStage<S>::UNIT);
    sp = (cmx_cplan)(MSG ? a.plan_r : m.plan) + ((size_t)planned_stream_copy(m.C, last, last ? c_after - c : 1) * (size_t)((MSG ? m.nmv_r : m.nmv) + 2) + 2);
    if constexpr (MSG) cmsg = a.cherry_msg + cherry_msg_header_bytes(m.nn) + (size_t)c * kCherryMsgTableBytes;
  }
  // ---- The halves of an op.  The wait is a dispatch on the entry's immediate over the values that
  // occur at this kind of op (cmx_layout.h: planned_wait_dispatchable; the host uploads no other).  ONE asm statement with
  // its own branches: written as nested ifs around seven asm waits, hipcc structurises the tree with an s_mov_b64 -1 /
  // s_andn2 vcc / s_cbranch_vccnz triple per arm -- 16 instructions to reach vmcnt(4) or vmcnt(5).  Here the most frequent
  // immediate is reached last and falls out of the statement: vmcnt(0) of a product (96 % of the benchmark tree's) in 3
  // instructions, vmcnt(5) / vmcnt(4) of a leaf op (71 %) in 5 / 6, vmcnt(14) / vmcnt(15) (26 %) in 7 / 8, the rest one
  // level deeper.  An arm that takes a range gives its smallest value to everything but the value it names: never a laxer wait.
  __device__ __forceinline__ static void wait_planned_product(int w) {
    asm volatile("s_cmp_lt_i32 %0, 10\n\ts_cbranch_scc1 8f\n\t"
                 "s_cmp_lt_i32 %0, 20\n\ts_cbranch_scc1 7f\n\t"
                 "s_cmp_lt_i32 %0, 30\n\ts_cbranch_scc1 6f\n\t"
                 "s_waitcnt vmcnt(30)\n\ts_branch 9f\n"
                 "6:\ts_waitcnt vmcnt(20)\n\ts_branch 9f\n"
                 "7:\ts_waitcnt vmcnt(10)\n\ts_branch 9f\n"
                 "8:\ts_waitcnt vmcnt(0)\n"
                 "9:" ::"s"(w) : "scc", "memory");
  }
  __device__ __forceinline__ static void wait_planned_leaf(int w) {
    asm volatile("s_cmp_lt_i32 %0, 14\n\ts_cbranch_scc1 7f\n\t"
                 "s_cmp_lt_i32 %0, 24\n\ts_cbranch_scc1 5f\n\t"
                 "s_cmp_lt_i32 %0, 30\n\ts_cbranch_scc1 3f\n\t"
                 "s_waitcnt vmcnt(30)\n\ts_branch 9f\n"
                 "3:\ts_cmp_eq_u32 %0, 25\n\ts_cbranch_scc1 4f\n\t"
                 "s_waitcnt vmcnt(24)\n\ts_branch 9f\n"
                 "4:\ts_waitcnt vmcnt(25)\n\ts_branch 9f\n"
                 "5:\ts_cmp_eq_u32 %0, 15\n\ts_cbranch_scc1 6f\n\t"
                 "s_waitcnt vmcnt(14)\n\ts_branch 9f\n"
                 "6:\ts_waitcnt vmcnt(15)\n\ts_branch 9f\n"
                 "7:\ts_cmp_eq_u32 %0, 5\n\ts_cbranch_scc1 8f\n\t"
                 "s_waitcnt vmcnt(4)\n\ts_branch 9f\n"
                 "8:\ts_waitcnt vmcnt(5)\n"
                 "9:" ::"s"(w) : "scc", "memory");
  }
  // the entry two ops ahead: one 16-byte scalar load from the running pointer
  __device__ __forceinline__ void next_entry() {
    plan_entry(sp, os);
    ++sp;
  }
  // a leaf op: request the next op's operator (and symbols), then wait for this op's.  The rows are addressed as
  // (wave-uniform operator address in SGPRs) + (16 x lane), here and in ProductRequest: no 64-bit address per lane.  Three
  // full rows and a partial one, whatever the next op is.
  __device__ __forceinline__ const uint8_t* leaf_begin() {
    static_assert(MatStage<S>::FULL == 3 && MatPart<kLeafBytes>::FULL == 3 && kProductBytes == MatStage<S>::BYTES, "rows of a request");
    const uint8_t* src = op_base + os.pre_off;
    const int etx = os.pre_tx, w = os.pre_w;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the LDS reads of the other buffer are done
    {
      const uint32_t dst = lds_stage + (os.par ^ 1u) * MatStage<S>::BYTES;
      const int l = vlane();
      const int tl = etx != kPlanProduct ? MatPart<kLeafBytes>::TAIL : MatStage<S>::TAIL;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\tglobal_load_lds_dwordx4 %1, %2 offset:2048" ::"s"(dst), "v"(16 * l), "s"(src) : "memory");
      if (l < tl) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:3072" ::"s"(dst), "v"(16 * l), "s"(src) : "memory");
    }
    if (etx >= 0) code_dma_l(gcodes + (size_t)etx * gstride, lds_codes + (os.par ^ 1u) * kCodeSlotBytes);
    next_entry();
    wait_planned_leaf(w);
    return stage + os.par * MatStage<S>::BYTES;
  }
  __device__ __forceinline__ void planned_end() { os.par ^= 1u; }
  // ---- The request of a product, cut into six pieces that mfma16_steps places in
  // its slots: behind a 16x16x4 the matrix pipe is busy for 64 cycles and the wave has nothing else to issue.  The pieces:
  // the operator's three full DMA rows (0 .. 2), its last row under the exec mask (3), the symbols (4), the stream entry
  // two ops ahead (5); req_slot says where each goes.  All of them sit in step 0: there the accumulators of the site
  // groups behind the slot are not live yet, so the pieces' temporaries -- a lane offset, the symbols' 64-bit address --
  // take registers nobody holds; from step 1 on they would come on top of the kernel's peak (DESIGN.md 4.1 has the counts).
  // The rows are addressed as (wave-uniform base in SGPRs) + (16 x lane): no 64-bit address per lane.
  // What op_begin requests, transfer for transfer, in another place; why each point holds there:
  //  * DMA overwrite.  The pieces write the other stage buffer and code slot; their last readers are LDS reads of earlier
  //    ops, all of them in front of the wait's asm in program order (a "memory" clobber: no access moves across it), hence
  //    issued before the product's first operand read.  Slot 0 lies behind the product's first matrix instruction, which
  //    reads that operand: the wave has executed an lgkmcnt wait that covers it (lgkmcnt(0) if a scalar load is in
  //    flight), and LDS reads return in order, so every earlier LDS read has returned.  No lgkmcnt(0) of our own is needed.
  //  * Workspace loads in front of the product are counted in the plan (kPlanVec each) and stay in flight across the wait.
  //  * Scheduling.  A slot begins with an empty asm that names the accumulator the 16x16x4 in front of it wrote ("+v": it
  //    cannot rise above that instruction) and the operand of the 4x4x4_4b behind it, as every DMA asm does (the 4x4x4_4b
  //    cannot rise above them); volatile asm statements keep their order, and the lane index the address arithmetic
  //    starts from is an output of the slot's first asm.  No asm reads the two registers.  The stream entry is a pair of
  //    compiler-visible scalar loads, which hipcc places where it likes.
  //  * M0.  Every piece that issues a DMA writes M0 itself.  Nothing else in a product reads or writes it: matrix
  //    instructions, ds_read_b64 and VALU arithmetic do not use M0 on gfx950.
  static constexpr int kReqPieces = 6;
  static constexpr int req_slot(int piece) { return piece < 2 ? 0 : (piece < 4 ? 1 : piece - 2); }
  static_assert(req_slot(kReqPieces - 1) < 4, "step 0");
  struct ProductRequest {
    PlannedWalk& w;
    int etx, tail;       // the next op's stream entry; lanes of its operator's last DMA row
    const uint8_t* src;  // wave-uniform
    uint32_t dst;
    __device__ __forceinline__ explicit ProductRequest(PlannedWalk& w_) : w(w_) {
      static_assert(!kCherryTables && kProductBytes == MatStage<S>::BYTES, "the 64-site protein walk");
      static_assert(MatStage<S>::FULL == 3 && MatPart<kLeafBytes>::FULL == 3 && MatStage<S>::TAIL > 0 && MatPart<kLeafBytes>::TAIL > 0,
                    "three full rows and a partial one, whatever the next op is");
      etx = w.os.pre_tx;
      src = w.op_base + w.os.pre_off;
      dst = w.lds_stage + (w.os.par ^ 1u) * MatStage<S>::BYTES;
      tail = etx != kPlanProduct ? MatPart<kLeafBytes>::TAIL : MatStage<S>::TAIL;   // (a leaf op's operator may be shorter: kLeafBytes)
    }
    template <int P, int SLOT>
    __device__ __forceinline__ void piece(int l, d4& acc, double& t) {
      if constexpr (req_slot(P) == SLOT) {
        if constexpr (P < 3) {
          asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %4 offset:%5"
                       : "+v"(acc), "+v"(t) : "s"(dst), "v"(16 * l), "s"(src), "i"(P * 1024) : "memory");
        } else if constexpr (P == 3) {
          if (l < tail)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:3072" ::"s"(dst), "v"(16 * l), "s"(src) : "memory");
        } else if constexpr (P == 4) {
          if (etx >= 0) code_dma_l(w.gcodes + (size_t)etx * w.gstride, w.lds_codes + (w.os.par ^ 1u) * kCodeSlotBytes);
        } else {
          w.next_entry();   // as leaf_begin
        }
      }
    }
    template <int SLOT>
    __device__ __forceinline__ void slot(d4& acc, double& t) {
      if constexpr (SLOT <= req_slot(kReqPieces - 1)) {
        int l = w.lane;
        if constexpr (SLOT <= req_slot(kReqPieces - 2)) asm volatile("" : "+v"(l), "+v"(acc), "+v"(t));   // (the stream entry alone: nothing to pin)
        piece<0, SLOT>(l, acc, t);
        piece<1, SLOT>(l, acc, t);
        piece<2, SLOT>(l, acc, t);
        piece<3, SLOT>(l, acc, t);
        piece<4, SLOT>(l, acc, t);
        piece<5, SLOT>(l, acc, t);
      }
    }
  };
  template <int SRC, int DST, bool TR>
  __device__ __forceinline__ void mv(int, int) {
    wait_planned_product(os.pre_w);
    const uint8_t* buf = stage + os.par * MatStage<S>::BYTES;
    ProductRequest req(*this);
    this->template product<SRC, DST, TR>(buf, req);
    planned_end();
  }
  template <int MODE, int SRC, int DST>
  __device__ __forceinline__ double row_op() {
    const uint8_t* buf = leaf_begin();
    const double tot = this->template rows<false, MODE, SRC, DST>(buf, os.par);
    planned_end();
    return tot;
  }
  template <int D> __device__ __forceinline__ void lset(int, int) { (void)row_op<LEAF_SET, D, D>(); }
  template <int SRC, int D> __device__ __forceinline__ void lmul(int, int) { (void)row_op<LEAF_MUL, SRC, D>(); }
  template <int SRC> __device__ __forceinline__ void ldot(int, int, int row) {
    const double tot = row_op<LEAF_DOT, SRC, SRC>();
    part_store(row, pc * tot);
  }
  // kCherryMsg: row 20 s1 + s2 of the cherry's table straight into the destination register, which the walk has killed.  No
  // stream entry, no request, no stage buffer: the lane loads the two symbols of its own site (plain loads: the alignments
  // were written by earlier kernels), fetches the row indices of its four site groups from the lanes that hold those sites,
  // and issues per group two 16-byte loads and one 8-byte load (cmx_layout.h: a row's quad slot).  All of it compiler-
  // visible, so hipcc waits for it; none of it counted in the wait plan: the operator of the op behind was requested by the
  // op in front and completes, in order, in front of these loads, and a planned wait that finds them in the queue only
  // waits for more (cmx_host_verify.cpp: WaitModel models them so).
  template <int D> __device__ __forceinline__ void cset(int node, int l1, int l2) {
    static_assert(MSG, "no other walk of this backend asks for a cherry's message");
    const int ci = cmsg_ref[node], t1 = cmsg_ref[l1], t2 = cmsg_ref[l2];   // cherry index, alignment rows (scalar loads)
    const int vl = vlane();
    unsigned s1 = gcodes[(size_t)t1 * gstride], s2 = gcodes[(size_t)t2 * gstride];
    s1 = s1 < 19u ? s1 : 19u;
    s2 = s2 < 19u ? s2 : 19u;
    const int row = (int)(20u * s1 + s2);
    const uint8_t* quad = cmsg + (size_t)ci * cmsg_stride + (vl >> 4) * kCherryMsgQuadBytes;
    double(&d)[VL] = this->template reg<D>();
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const uint8_t* p = quad + (size_t)__shfl(row, 16 * g + (vl & 15)) * kCherryMsgRowBytes;
      const d2 a = *reinterpret_cast<const d2*>(p), b = *reinterpret_cast<const d2*>(p + 16);
      const double e = *reinterpret_cast<const double*>(p + 32);
      d[vr(0, g)] = a[0];
      d[vr(1, g)] = a[1];
      d[vr(2, g)] = b[0];
      d[vr(3, g)] = b[1];
      d[vr(4, g)] = e;
    }
  }
};

// the backend of an instantiation
template <int S, int FUSE, int NG, bool RESOLVED, class POL, bool MSG = false>
using DevWalk = std::conditional_t<kMfma16<S, NG, (FUSE > 1 && S / FUSE == 4)>, PlannedWalk<S, FUSE, NG, RESOLVED, POL, MSG>,
                                   CountedWalk<S, FUSE, NG, RESOLVED, POL>>;

// Maps the 64 sites of this wave (symbol of taxon t at gcodes[t * gstride], per lane) for all rate classes: one walk of
// the tree (cmx_walk.h) per class.  Classes [c_begin, c_end) are processed; c_after is the class of the first pass that
// follows this call (its first operator is requested by the last operator op here).  With finalize, on return
// cnt[(b*K+k)*64 + lane] holds the final counts n(b, site, k) and the scalars are per lane; without (class-split
// observed mode) only part[] and L_out = sum of p_c L_c over the processed classes are produced.
// part: [C][B*K][64] per-class joint counts (written once each, summed at the end: no read-modify-write in the loop).
template <int S, int FUSE, int NG, bool RESOLVED, class POL, bool MSG = false>
__device__ __forceinline__ void map_sites_wave(const MapArgs& a, double* __restrict__ wsM, double* __restrict__ wsU,
                                               double* __restrict__ part, double* __restrict__ cnt, int lds_off,
                                               const uint8_t* __restrict__ gcodes, size_t gstride, int lane,
                                               typename DevWalk<S, FUSE, NG, RESOLVED, POL, MSG>::State& os, double& L_out, double& pr_out, int& rc_out,
                                               double& norm_out, int c_begin, int c_end, int c_after, bool finalize) {
  const DevModel& m = a.m;
  using Walk = DevWalk<S, FUSE, NG, RESOLVED, POL, MSG>;
  static_assert(Walk::kCherryMsg == MSG, "the message table serves the planned walk");
  constexpr bool kTables = Walk::kCherryTables;   // (the launcher guarantees m.msched_r then)
  const ConstModel cm(m, kTables || MSG);   // (MSG: the resolved stream, likewise)
  constexpr int kSites = 16 * NG;      // sites per wave (NG site groups of 16; an S-vector is S / 4 * NG doubles per lane)
  // site of this lane inside the wave's block for per-site scalars and arrays: NG = 4: the lane itself; NG = 1: lanes
  // l, l ^ 16, l ^ 32 and l ^ 48 all carry site l & 15 and do the per-site work redundantly (identical values)
  const int sidx = NG == 4 ? lane : (lane & 15);
  const int C = m.C, K = m.K;
  double Lsum = 0.0, prsum = 0.0, best = -1.0;
  int bestc = 0;
  Walk be(os, cm, a);
  be.pi = m.pi;
  be.wsM = wsM;
  be.wsU = wsU;
  be.gcodes = gcodes;
  be.gstride = gstride;
  be.stage = cmx_smem + lds_off;                                 // two operator buffers
  be.cslot = be.stage + 2 * MatStage<S>::BYTES;                  // two symbol slots
  be.cslot2 = be.cslot + 2 * kCodeSlotBytes;                     // ... and two for the second leaf of a cherry-table op
  be.vslot = be.cslot2 + 2 * kCodeSlotBytes;                     // ... and, with kLdsSlot, one workspace vector
  be.lds_stage = lds_addr(be.stage);                             // wave-uniform LDS byte addresses (SGPRs)
  be.lds_codes = lds_addr(be.cslot);
  be.lds_codes2 = lds_addr(be.cslot2);
  be.lane = lane;
  {  // symbols of op 0 if it is a leaf op (the previous site block could not request them).  Everything this wave
     // wrote before (simulated symbols) is in L2 first; the request is not counted, so drain it here.
    const int tx0 = cm.msched[1];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tx0 >= 0) {
      if (kTables && (tx0 & 0x40000000)) {
        code_dma(gcodes + (size_t)cherry_taxon1(tx0) * gstride, be.cslot + os.par * kCodeSlotBytes);
        code_dma(gcodes + (size_t)cherry_taxon2(tx0) * gstride, be.cslot2 + os.par * kCodeSlotBytes);
      } else {
        code_dma(gcodes + (size_t)tx0 * gstride, be.cslot + os.par * kCodeSlotBytes);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  for (int c = c_begin; c < c_end; ++c) {
    be.begin_class(a, c, c_end, c_after);
    const double pc = FUSE > 1 ? 1.0 : cm.probs[c];  // fused: the class probabilities are folded into the count operators
    be.pc = pc;
    be.pcnt = part + (size_t)c * m.B * K * kSites;   // wave-uniform; the lane's site is added at each use
    be.begin_pass();
    walk_pass(be, m.NV, K);
    if constexpr (FUSE == 1) {
      const double Lc = be.Lg[0];
      Lsum += pc * Lc;
      prsum += cm.rates[c] * pc * Lc;
      if (pc * Lc > best) { best = pc * Lc; bestc = c; }  // first maximum wins (getRateClassWithMaxPostProbPerSite)
    } else {
#pragma unroll
      for (int g = 0; g < FUSE; ++g) {
        const int cc = c * FUSE + g;
        if (cc < m.C0) {
          const double pg = cm.probs[cc];
          Lsum += pg * be.Lg[g];
          prsum += cm.rates[cc] * pg * be.Lg[g];
          if (pg * be.Lg[g] > best) { best = pg * be.Lg[g]; bestc = cc; }
        }
      }
    }
  }
  if (!finalize) {   // class-split mode: the pass's sums, its best class and that class's weight
    L_out = Lsum;
    pr_out = prsum;
    rc_out = bestc;
    norm_out = best;
    return;
  }
  // ---------------- sum the classes in class order, divide by the site likelihood, norm (computeNormForSite)
  // Rows r = b*K + k are taken sixteen at a time and classes four at a time so that 64 independent loads are in flight
  // (this phase is pure L2 latency); the sums run in the same order as a plain (b, k, c) loop nest.
  double nrm = 0.0, tot = 0.0;
  const int BK = m.B * K;
  int kk = 0;  // r % K
  constexpr int RC = 16;
  for (int r0 = 0; r0 < BK; r0 += RC) {
    double v[RC];
#pragma unroll
    for (int u = 0; u < RC; ++u) v[u] = 0.0;
    int c = 0;
    for (; c + 4 <= C; c += 4) {
      double t[4][RC];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double* pp = part + ((size_t)(c + q) * BK + r0) * kSites + sidx;
#pragma unroll
        for (int u = 0; u < RC; ++u) t[q][u] = state_load<POL::p_load>(pp + (size_t)(r0 + u < BK ? u : 0) * kSites);
      }
#pragma unroll
      for (int u = 0; u < RC; ++u) v[u] = (((v[u] + t[0][u]) + t[1][u]) + t[2][u]) + t[3][u];
    }
    for (; c < C; ++c) {
      const double* pp = part + ((size_t)c * BK + r0) * kSites + sidx;
#pragma unroll
      for (int u = 0; u < RC; ++u) v[u] += state_load<POL::p_load>(pp + (size_t)(r0 + u < BK ? u : 0) * kSites);
    }
#pragma unroll
    for (int u = 0; u < RC; ++u) {
      if (r0 + u < BK) {
        const double q = v[u] / Lsum;
        state_store<POL::t_store>(q, cnt + ((size_t)(r0 + u) * kSites + sidx));
        tot += q;
        if (++kk == K) {
          nrm = __builtin_fma(tot, tot, nrm);
          tot = 0.0;
          kk = 0;
        }
      }
    }
  }
  L_out = Lsum;
  pr_out = prsum / Lsum;
  rc_out = bestc;
  norm_out = sqrt(nrm);
}

// LDS per mapping wave: two operator stage buffers + four symbol slots (two per leaf of a cherry-table op), and one
// workspace vector of ng site groups for the instantiations with an LDS slot (DevWalk::kLdsSlot)
template <int S>
constexpr int map_lds_fixed(int fuse, int ng) {
  return 2 * MatStage<S>::BYTES + 4 * kCodeSlotBytes + (map_lds_slot(S, fuse, ng) ? S / 4 * ng * kWave * 8 : 0);
}
static int map_lds_per_wave(int S, int fuse, int ng) {
  return S == 20 ? map_lds_fixed<20>(fuse, ng) : (S == 16 ? map_lds_fixed<16>(fuse, ng) : map_lds_fixed<4>(fuse, ng));
}
static_assert(kWavesPerBlock * map_lds_fixed<20>(1, 4) <= 160 * 1024 / map_waves_per_simd(20), "the protein walk's workgroup fits its share of a CU's LDS");

// How blocks reach the waves: the block a wave maps after block sb.  Without a queue the fixed share, block
// sb + nwaves.  With one, the next block nobody has taken: the counter starts at nwaves (every wave's first block is its own
// index, no atomic), lane 0 draws with one vector atomic and the index is made wave-uniform; a wave leaves at the first index
// past the last block.  One wave-uniform branch between two blocks, outside the walk: the atomic is issued after the block's
// epilogue, CountedState::vs does not count it (an uncounted VMEM instruction only makes wait_vm stricter), and the wait for its
// result drains it with the operator DMA the block's last op left in flight -- (class 0, entry 0), right for any next block.
// Which wave maps a block changes no output: workspace, part and cnt0 / cnt1 are keyed by wave, tiles and per-site results by block.
__device__ __forceinline__ size_t next_block(unsigned long long* queue, size_t sb, int nwaves, int lane) {
  if (queue == nullptr) return sb + nwaves;
  unsigned long long t = 0;
  if (lane == 0) t = atomicAdd(queue, 1ull);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)t);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(t >> 32));
  return (size_t)(((unsigned long long)hi << 32) | lo);
}

template <int S, int MODE_ARG, int FUSE, int NG = map_ng(S)>
__global__ __launch_bounds__(kWave * kWavesPerBlock, map_waves_per_simd(S)) void map_kernel(const MapArgs a) {
  constexpr int MODE = map_mode_base(MODE_ARG);     // what the kernel does; MSG: how its walk gets a cherry's message
  constexpr bool MSG = map_mode_msg(MODE_ARG);
  constexpr int VL = S / 4 * NG, kSites = 16 * NG;
  using POL = StatePolicy<S, MODE, FUSE, NG>;
  const DevModel& m = a.m;
  // the null's alignments are fully resolved: class-fused nucleotide models walk them with the cherry tables' stream
  using Walk = DevWalk<S, FUSE, NG, true, POL, MSG>;   // (its State is the same for every alignment it walks)
  constexpr bool kTables = (MODE == kModeNull || MODE == kModeNullPatterns) && Walk::kCherryTables;
  const ConstModel cm(m, kTables || MSG);
  const int lane = threadIdx.x & (kWave - 1);
  const int sidx = NG == 4 ? lane : (lane & 15);   // site of this lane in the wave's block
  // wave index through readfirstlane: the compiler cannot see that threadIdx.x >> 6 is wave-uniform and would keep every
  // per-wave base pointer below as a per-lane 64-bit VGPR pair (spilled, and reloaded from scratch in the hot loop)
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = blockIdx.x * kWavesPerBlock + wib;
  const int nwaves = gridDim.x * kWavesPerBlock;
  double* wsD = a.ws.D + (size_t)wave * m.NIW * VL * kWave;
  double* wsU = a.ws.U + (size_t)wave * m.NIW * VL * kWave;
  double* cnt0 = a.ws.cnt + (size_t)wave * 2 * m.B * m.K * kSites;
  double* cnt1 = cnt0 + (size_t)m.B * m.K * kSites;
  double* part = a.ws.part + (size_t)wave * m.C * m.B * m.K * kSites;
  // LDS per wave: two operator stage buffers, then four symbol slots, then the vector slot if any (map_lds_fixed)
  const int lds_off = wib * a.lds_per_wave;
  const size_t nblocks = (a.nsites + kSites - 1) / kSites;
  // request the first op's operator (class 0, entry 0); every op then requests the next one
  typename Walk::State os;
  os.par = 0;
  {
    const int c0 = (MODE == kModeObservedSplit) ? wave % m.C : 0;   // class of this wave's first pass
    mat_dma<S>(m.MAT + (size_t)c0 * m.MC * MatStage<S>::UNIT + cm.msched[0], cmx_smem + lds_off, lane);
  }
  // ... and entry 1.  (Written out here, not a call on the backend: behind a function boundary hipcc promotes the stream
  // pointer to the entry's two values and rebuilds their address in the caller without `inbounds`, and thirteen kernels
  // that are to keep their text merge the stream's first scalar loads otherwise.)
  if constexpr (kMfma16<S, NG, Walk::DIAG>) {   // the planned walk: the same in every copy
    plan_entry((cmx_cplan)(MSG ? a.plan_r : m.plan) + 1, os);
  } else {
    os.vs = MatStage<S>::ROWS;
    os.cur_seq = os.vs;
    os.pre_mat = cm.msched[2];   // (the stream is padded with copies of its first entries)
    os.pre_tx = cm.msched[3];
  }
  if (MODE == kModeObservedSplit) {
    const size_t ntasks = nblocks * (size_t)m.C, BK = (size_t)m.B * m.K;
    for (size_t task = wave; task < ntasks; task += nwaves) {
      const size_t sb = task / m.C;
      const int c = (int)(task % m.C);
      const size_t site = sb * kSites + sidx;
      const size_t s = site < a.nsites ? site : a.nsites - 1;
      double L, pr, nrm;
      int rc;
      map_sites_wave<S, FUSE, NG, false, POL>(a, wsD, wsU, a.split_part + sb * m.C * BK * kSites, nullptr, lds_off, a.aln + s, a.ld, lane, os, L, pr,
                        rc, nrm, c, c + 1, (int)((task + nwaves) % m.C), false);
      state_store<POL::split_store>(L, a.split_lc + (task * kSites + sidx));
      state_store<POL::split_store>(pr, a.split_lc + ((ntasks + task) * kSites + sidx));
      state_store<POL::split_store>(nrm, a.split_lc + ((2 * ntasks + task) * kSites + sidx));          // weight of the pass's best class
      state_store<POL::split_store>((double)rc, a.split_lc + ((3 * ntasks + task) * kSites + sidx));   // ... and its index
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }
  if constexpr (MODE == kModeNullPatterns) {
    // lane = pattern p (numbered in first-occurrence order): the column of its first site g, walked exactly as
    // the null mode walks a site of a pair; per pattern what observed mode writes per site
    const size_t npat = *a.npat;
    const size_t nb = (npat + kSites - 1) / kSites;
    for (size_t sb = wave; sb < nb; sb = next_block(a.queue, sb, nwaves, lane)) {
      const size_t p = sb * kSites + sidx;
      const bool active = p < npat;
      const size_t g = a.rep_site[active ? p : npat - 1];
      const size_t rh = g / a.rep_ram, j = g - rh * a.rep_ram;   // rh = rep_local * 2 + h
      double L, pr, nrm;
      int rc;
      // tile sb of the pattern table is this wave's count block: the class-sum epilogue writes the final counts there,
      // once, with its own row stride (lanes past npat write their clamped copy into the last tile's spare columns)
      double* tile = a.counts + sb * ((size_t)m.B * m.K * kSites);
      map_sites_wave<S, FUSE, NG, true, POL, MSG>(a, wsD, wsU, part, tile, lds_off, a.supplied + rh * (size_t)m.T * a.rep_ram + j, a.rep_ram,
                                        lane, os, L, pr, rc, nrm, 0, m.C, 0, true);
      if (active) {
        a.post_rate[p] = pr;
        a.rate_class[p] = rc;
        a.norm[p] = nrm;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }
  for (size_t sb = wave; sb < nblocks; sb = next_block(a.queue, sb, nwaves, lane)) {
    const size_t site = sb * kSites + sidx;
    const bool active = site < a.nsites;
    const size_t s = active ? site : a.nsites - 1;
    if (MODE == kModeObserved) {
      double L, pr, nrm;
      int rc;
      map_sites_wave<S, FUSE, NG, false, POL>(a, wsD, wsU, part, cnt0, lds_off, a.aln + s, a.ld, lane, os, L, pr, rc, nrm, 0, m.C, 0, true);
      if (active) {
        if (a.logL) a.logL[s] = log(L);
        if (a.post_rate) a.post_rate[s] = pr;
        if (a.rate_class) a.rate_class[s] = rc;
        if (a.norm) a.norm[s] = nrm;
        if (a.counts)
          for (int r = 0; r < m.B * m.K; ++r) {
            const double q = state_load<POL::t_load>(&cnt0[(size_t)r * kSites + sidx]);
            a.counts[(size_t)r * a.ldc + s] = q;
          }
      }
    } else {
      // null pair q = s: replicate rep, column j; simulated-site index g_h = ((rep*2 + h)*rep_ram + j).
      // Only the minima over the two batches leave the loop (AnalysisTools.cpp:643-652) -- fewer live registers.
      double prmin = 0.0, nmin = 0.0;
      int rcmin = 0;
      for (int h = 0; h < 2; ++h) {
        const size_t rep_local = s / a.rep_ram, j = s % a.rep_ram;
        const uint8_t* gbase;
        size_t gstride;
        // the alignments were simulated by simulate_chain_kernel / simulate_blocked_kernel (cmx_null_simulate_dev) or
        // supplied by the caller: [replicate][batch][taxon][rep_ram]
        gbase = a.supplied + ((rep_local * 2 + h) * (size_t)m.T) * a.rep_ram + j;
        gstride = a.rep_ram;
        double L, pr, nrm;
        int rc;
        map_sites_wave<S, FUSE, NG, true, POL, MSG>(a, wsD, wsU, part, h ? cnt1 : cnt0, lds_off, gbase, gstride, lane, os, L, pr, rc, nrm, 0, m.C, 0, true);
        if (h == 0) { prmin = pr; nmin = nrm; rcmin = rc; }
        else { prmin = pr < prmin ? pr : prmin; nmin = nrm < nmin ? nrm : nmin; rcmin = rc < rcmin ? rc : rcmin; }
      }
      const double stat = pair_stat_strided(a.stat_kind, a.stat_param, m.B, m.K, cnt0 + sidx, (size_t)kSites, cnt1 + sidx, (size_t)kSites, a.stat_mean);
      if (active) {
        a.null_stat[s] = stat;
        if (a.null_rcmin) a.null_rcmin[s] = rcmin;
        if (a.null_prmin) a.null_prmin[s] = prmin;
        if (a.null_nmin) a.null_nmin[s] = nmin;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last op left an operator DMA in flight
}

template <int S, int MODE, int FUSE, int NG = map_ng(S)>
static hipError_t launch_map_as(const MapArgs& a, dim3 grid, dim3 block, size_t lds, int lim, hipStream_t stream) {
  // per launch: the attribute belongs to the current device (a process may hold contexts on several)
  const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&map_kernel<S, MODE, FUSE, NG>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, lim);
  if (ea != hipSuccess) return ea;
  hipLaunchKernelGGL((map_kernel<S, MODE, FUSE, NG>), grid, block, lds, stream, a);
  return hipGetLastError();
}
template <int S, int FUSE>
static hipError_t launch_map_mode(int mode, const MapArgs& a, dim3 grid, dim3 block, size_t lds, int lim, hipStream_t stream) {
  switch (mode) {
    case kModeObserved: return launch_map_as<S, kModeObserved, FUSE>(a, grid, block, lds, lim, stream);
    case kModeObservedSplit: return launch_map_as<S, kModeObservedSplit, FUSE>(a, grid, block, lds, lim, stream);
    case kModeNullPatterns: return launch_map_as<S, kModeNullPatterns, FUSE>(a, grid, block, lds, lim, stream);
    case kModeNullMsg:
      if constexpr (S == 20 && FUSE == 1) return launch_map_as<S, kModeNullMsg, FUSE>(a, grid, block, lds, lim, stream);
      else return hipErrorInvalidValue;
    case kModeNullPatternsMsg:
      if constexpr (S == 20 && FUSE == 1) return launch_map_as<S, kModeNullPatternsMsg, FUSE>(a, grid, block, lds, lim, stream);
      else return hipErrorInvalidValue;
    default: return launch_map_as<S, kModeNull, FUSE>(a, grid, block, lds, lim, stream);
  }
}

hipError_t launch_map(const MapArgs& a_in, int mode, int grid_blocks, hipStream_t stream) {
  dim3 grid(grid_blocks), block(kWave * kWavesPerBlock);
  MapArgs a = a_in;
  const bool split16 = a.m.S == 20 && a.m.fuse == 1 && mode == kModeObservedSplit && a.split_sites == 16;
  a.lds_per_wave = map_lds_per_wave(a.m.S, a.m.fuse, split16 ? 1 : map_ng(a.m.S));
  const size_t lds = (size_t)kWavesPerBlock * (size_t)a.lds_per_wave;
  const int lim = 160 * 1024 / map_waves_per_simd(a.m.S);  // dynamic LDS a workgroup may use (that many workgroups per CU)
  if ((int)lds > lim) return hipErrorInvalidValue;
  // (the null instantiations of the class-fused layouts read the cherry-table walk's stream)
  if ((mode == kModeNull || mode == kModeNullPatterns) && a.m.fuse > 1 && a.m.msched_r == nullptr) return hipErrorInvalidValue;
  // (... and those of a model with a cherry message table the resolved stream, its planned copy and the table)
  if (map_mode_msg(mode) && (a.m.S != 20 || a.m.fuse != 1 || !a.m.msched_r || !a.plan_r || !a.cherry_msg)) return hipErrorInvalidValue;
  if (a.m.S == 20 && a.m.fuse == 1 && a.m.plan == nullptr) return hipErrorInvalidValue;   // the 64-site protein walk reads the planned stream
  if (map_mode_base(mode) == kModeNullPatterns && (!a.rep_site || !a.npat || !a.counts || !a.post_rate || !a.rate_class || !a.norm)) return hipErrorInvalidValue;
  // 16-site wave-tasks (one site group): small alignments, four times the waves
  if (split16)
    return launch_map_as<20, kModeObservedSplit, 1, 1>(a, grid, block, lds, lim, stream);
  if (a.m.S == 20 && a.m.fuse == 1) return launch_map_mode<20, 1>(mode, a, grid, block, lds, lim, stream);
  if (a.m.S == 20 && a.m.fuse == 5) return launch_map_mode<20, 5>(mode, a, grid, block, lds, lim, stream);
  if (a.m.S == 16 && a.m.fuse == 4) return launch_map_mode<16, 4>(mode, a, grid, block, lds, lim, stream);
  if (a.m.S == 4 && a.m.fuse == 1) return launch_map_mode<4, 1>(mode, a, grid, block, lds, lim, stream);
  return hipErrorInvalidValue;
}

// a launch's block counter, set on the launch's own stream right before it (next_block): one thread, one store
__global__ void map_queue_init_kernel(unsigned long long* queue, unsigned long long first) { *queue = first; }

hipError_t launch_map_queue_init(unsigned long long* queue, unsigned long long first, hipStream_t stream) {
  hipLaunchKernelGGL(map_queue_init_kernel, dim3(1), dim3(1), 0, stream, queue, first);
  return hipGetLastError();
}

// class-split observed mode: sums the per-class results in class order exactly as map_sites_wave's own epilogue does.
// 64 sites x 16 branch lanes per workgroup (round 4; one thread per site walked B x C dependent loads, 0.2 ms for 2 000
// sites): thread (site, w) sums the classes of the branches b = w mod 16 and leaves each branch's total in LDS, then the
// site's first thread adds the squares in branch order -- every sum runs in the order of the plain (b, k, c) loop nest.
constexpr int kFinBranchLanes = 16, kFinChunk = 128;
__global__ __launch_bounds__(64 * kFinBranchLanes) void map_finalize_kernel(const MapArgs a) {
  const DevModel& m = a.m;
  __shared__ double tots[kFinChunk][64];
  const int tx = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t s = (size_t)blockIdx.x * 64 + tx;
  const bool live = s < a.nsites;
  const size_t sc = live ? s : a.nsites - 1;
  const size_t kS = (size_t)a.split_sites;   // sites per wave-task of the mapping kernel
  const size_t sb = sc / kS, lane = sc % kS, BK = (size_t)m.B * m.K;
  const size_t nblocks = (a.nsites + kS - 1) / kS, ntasks = nblocks * (size_t)m.C;
  double Lsum = 0.0, prsum = 0.0, best = -1.0;
  int bestc = 0;
  for (int c = 0; c < m.C; ++c) {
    const size_t t = sb * m.C + c;
    Lsum += a.split_lc[t * kS + lane];
    prsum += a.split_lc[(ntasks + t) * kS + lane];
    const double bv = a.split_lc[(2 * ntasks + t) * kS + lane];
    if (bv > best) { best = bv; bestc = (int)a.split_lc[(3 * ntasks + t) * kS + lane]; }
  }
  const double* part = a.split_part + sb * m.C * BK * kS + lane;
  double nrm = 0.0;
  for (int b0 = 0; b0 < m.B; b0 += kFinChunk) {
    const int be = b0 + kFinChunk < m.B ? b0 + kFinChunk : m.B;
    for (int b = b0 + w; b < be; b += kFinBranchLanes) {
      double tot = 0.0;
      for (int k = 0; k < m.K; ++k) {
        const size_t r = (size_t)b * m.K + k;
        double v = 0.0;
        for (int c = 0; c < m.C; ++c) v += part[((size_t)c * BK + r) * kS];
        v /= Lsum;
        if (a.counts && live) a.counts[r * a.ldc + s] = v;
        tot += v;
      }
      tots[b - b0][tx] = tot;
    }
    __syncthreads();
    if (w == 0)
      for (int b = b0; b < be; ++b) nrm = __builtin_fma(tots[b - b0][tx], tots[b - b0][tx], nrm);
    __syncthreads();
  }
  if (w != 0 || !live) return;
  if (a.logL) a.logL[s] = log(Lsum);
  if (a.post_rate) a.post_rate[s] = prsum / Lsum;
  if (a.rate_class) a.rate_class[s] = bestc;
  if (a.norm) a.norm[s] = sqrt(nrm);
}

hipError_t launch_map_finalize(const MapArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(map_finalize_kernel, dim3((unsigned)((a.nsites + 63) / 64)), dim3(64 * kFinBranchLanes), 0, stream, a);
  return hipGetLastError();
}

// Rows S0 .. S0+A-1 of every transposed leaf operator: sum of the rows of the states compatible with ambiguity id a
// (what the DR likelihood's leaf initialisation does for B/Z/X/gap).  One thread per (class, leaf operator, a, x);
// a row has `rowlen` values (= S0, or S0 * fuse for the class-fused nucleotide layout).
__global__ void extend_leaf_rows_kernel(double* MAT, int C, int MC, int first_leaf, int nleaf, int S0, int rowlen, int A,
                                        int unit, int stride /* doubles between rows: leaf_row_stride */, const uint32_t* __restrict__ masks) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)C * nleaf * A * rowlen;
  if (i >= total) return;
  const int x = (int)(i % rowlen);
  const int a = (int)((i / rowlen) % A);
  const int l = (int)((i / ((size_t)rowlen * A)) % nleaf);
  const int c = (int)(i / ((size_t)rowlen * A * nleaf));
  double* M = MAT + ((size_t)c * MC + first_leaf + l) * unit;
  const uint32_t mk = masks ? masks[S0 + a] : 0xffffffffu;
  double v = 0.0;
  for (int z = 0; z < S0; ++z)
    if ((mk >> z) & 1u) v += M[(size_t)z * stride + x];
  M[(size_t)(S0 + a) * stride + x] = v;
}

hipError_t launch_extend_leaf_rows(const DevModel& m, const uint32_t* d_masks, hipStream_t stream) {
  const int A = max_ambig(m.S0), nleaf = m.T + m.K * m.T;
  const size_t total = (size_t)m.C * nleaf * A * m.S;
  hipLaunchKernelGGL(extend_leaf_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, m.MAT, m.C, m.MC,
                     ClassBlock{m.NI, m.K, m.T, 0}.first_leaf(), nleaf, m.S0, m.S, A, mat_unit(m.S), leaf_row_stride(m.S), d_masks);
  return hipGetLastError();
}

// The cherry message table of a 20-state model (cmx_layout.h, cmx_walk.h: kCherryMsg), filled by the walk's own code so that
// a gathered row is the bits the walk would compute.  One wave per (cherry, class, 64 symbol pairs): the pairs take the place
// of the wave's 64 sites -- "site" j of block b shows the symbols (p / 20, p % 20), p = 64 b + j -- and the wave runs what
// walk_cherry_message runs without a table: lset<3>(l1), lmul<3, 3>(l2), mv<3, 1, false>(node) on the three operators copied
// from MAT into LDS, with the 64-site protein walk's leaf_apply and matvec_stage (the 16x16x4 path).  It stores R1 in the
// row layout of the gather.  Pairs past 399 (the last block) repeat pair 399 and store nothing.
constexpr int kCherryMsgBlocks = (kCherryMsgPairs + kWave - 1) / kWave;
__global__ __launch_bounds__(kWave) void cherry_msg_kernel(const double* __restrict__ MAT, int C, int MC, const int* __restrict__ ops,
                                                          uint8_t* __restrict__ table) {
  constexpr int S = 20, NG = 4, VL = S / 4 * NG, OPB = MatStage<S>::BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t smem[3 * OPB + 2 * kCodeSlotBytes];
  const int lane = threadIdx.x, blk = blockIdx.x, c = blockIdx.y, ci = blockIdx.z;
  for (int o = 0; o < 3; ++o) {   // P_l1^T, P_l2^T (leaf operators), P_c (packed): 16-byte pieces
    const d2* src = reinterpret_cast<const d2*>(MAT + ((size_t)c * MC + ops[4 * ci + o]) * MatStage<S>::UNIT);
    d2* dst = reinterpret_cast<d2*>(smem + o * OPB);
    for (int i = lane; i < OPB / 16; i += kWave) dst[i] = src[i];
  }
  const int pair = blk * kWave + lane, pc = pair < kCherryMsgPairs ? pair : kCherryMsgPairs - 1;
  uint32_t* slot1 = reinterpret_cast<uint32_t*>(smem + 3 * OPB);   // one dword per site, as a code slot of the walk
  uint32_t* slot2 = slot1 + kWave;
  slot1[lane] = (uint32_t)(pc / S);
  slot2[lane] = (uint32_t)(pc % S);
  __syncthreads();
  double R1[VL], R3[VL];
  (void)leaf_apply<S, LEAF_SET, NG, false>(smem, reinterpret_cast<const uint8_t*>(slot1) + 4 * (lane & 15), lane, R3, R3);
  (void)leaf_apply<S, LEAF_MUL, NG, false>(smem + OPB, reinterpret_cast<const uint8_t*>(slot2) + 4 * (lane & 15), lane, R3, R3);
  NoRequest req;
  matvec_stage<S, false, NG, false>(smem + 2 * OPB, lane, R3, R1, req);
  uint8_t* tab = table + ((size_t)ci * C + c) * kCherryMsgTableBytes + (lane >> 4) * kCherryMsgQuadBytes;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int p = blk * kWave + 16 * g + (lane & 15);   // the pair whose states 4 sb + (lane >> 4) this lane holds in group g
    if (p < kCherryMsgPairs) {
      double* q = reinterpret_cast<double*>(tab + (size_t)p * kCherryMsgRowBytes);
#pragma unroll
      for (int sb = 0; sb < S / 4; ++sb) q[sb] = R1[vreg<S, NG, false>(sb, g)];
    }
  }
}

hipError_t launch_cherry_msg(const DevModel& m, const int* d_ops, int cherries, uint8_t* d_table, hipStream_t stream) {
  if (m.S != 20 || m.fuse != 1 || cherries <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cherry_msg_kernel, dim3(kCherryMsgBlocks, m.C, cherries), dim3(kWave), 0, stream, m.MAT, m.C, m.MC, d_ops, d_table);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ listed pairs and groups
// pair_diag_kernel and group_stat_kernel stay in this file: they score pairs through the same per-lane statistic
// (cmx_pairstat.h) as the null-mode walk, and the code hipcc emits for map_kernel<S, kModeNull> depends on their presence in
// the translation unit (compiled elsewhere: same registers and scratch, 5 to 63 more instructions).
// statistic of the pairs (j of data set 1, j of data set 2), j < n, and the minima the null file carries
// (AnalysisTools.cpp:728-732): counts are branch-major [B*K][ld]
__global__ void pair_diag_kernel(int kind, double param, int B, int K, const double* __restrict__ c1, size_t ld1,
                                 const double* __restrict__ c2, size_t ld2, size_t n, const int32_t* __restrict__ rc1,
                                 const int32_t* __restrict__ rc2, const double* __restrict__ pr1,
                                 const double* __restrict__ pr2, const double* __restrict__ nm1,
                                 const double* __restrict__ nm2, double* __restrict__ stat, int32_t* __restrict__ rcmin,
                                 double* __restrict__ prmin, double* __restrict__ nmin, const double* __restrict__ mv,
                                 const double* __restrict__ w) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (stat) stat[j] = w ? pair_stat_weighted(kind, param, B, K, c1 + j, ld1, c2 + j, ld2, mv, w)
                        : pair_stat_strided(kind, param, B, K, c1 + j, ld1, c2 + j, ld2, mv);
  if (rcmin) rcmin[j] = rc1[j] < rc2[j] ? rc1[j] : rc2[j];
  if (prmin) prmin[j] = pr1[j] < pr2[j] ? pr1[j] : pr2[j];
  if (nmin) nmin[j] = nm1[j] < nm2[j] ? nm1[j] : nm2[j];
}

hipError_t launch_pair_diag(const Stat& st, const double* c1, size_t ld1, const SiteCols& s1, const double* c2, size_t ld2,
                            const SiteCols& s2, size_t n, const PairOut& out, hipStream_t stream) {
  hipLaunchKernelGGL(pair_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, st.kind, st.param, st.B, st.K, c1, ld1,
                     c2, ld2, n, s1.rc, s2.rc, s1.pr, s2.pr, s1.nm, s2.nm, out.stat, out.rcmin, out.prmin, out.nmin, st.d_mean, st.d_w);
  return hipGetLastError();
}

// Statistic of a group of sites, Statistic::getValueForGroup: the smallest pairwise value over the group
// (AbstractMinimumStatistic, CoMap/Statistics.h:121-133) or, for Compensation, the closed form of Statistics.h:267-294.
// One wave per group; group g owns sites[offsets[g] .. offsets[g+1]) (columns of the branch-major counts).
// w (or null): normalised branch weights; the Compensation closed form then sums w t^2 (Statistics.h:275-285) as
// (weight_factor * t)^2, the pairs use pair_stat_weighted.
__global__ __launch_bounds__(kWave) void group_stat_kernel(int kind, double param, int B, int K, const double* __restrict__ counts,
                                                          size_t ld, const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ sites, double* __restrict__ out,
                                                          const double* __restrict__ mv, const double* __restrict__ w) {
  const size_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int32_t* mem = sites + offsets[g];
  const int m = (int)(offsets[g + 1] - offsets[g]);
  if (kind == CMX_STAT_COMPENSATION) {
    double sumnorms = 0.0, sq2 = 0.0;
    for (int j = 0; j < m; ++j) {
      double q = 0.0;
      for (int b = lane; b < B; b += kWave) {
        double t = 0.0;
        for (int k = 0; k < K; ++k) t += counts[((size_t)b * K + k) * ld + mem[j]];
        if (w) t *= weight_factor(kind, w[b]);
        q += t * t;
      }
      for (int off = 32; off; off >>= 1) q += __shfl_xor(q, off);
      sumnorms += sqrt(q);
    }
    for (int b = lane; b < B; b += kWave) {
      double t = 0.0;
      for (int j = 0; j < m; ++j)
        for (int k = 0; k < K; ++k) t += counts[((size_t)b * K + k) * ld + mem[j]];
      if (w) t *= weight_factor(kind, w[b]);
      sq2 += t * t;
    }
    for (int off = 32; off; off >>= 1) sq2 += __shfl_xor(sq2, off);
    if (lane == 0) out[g] = 1.0 - sqrt(sq2) / sumnorms;
    return;
  }
  // pairs (i, j), j < i, in the reference's order; "val < mini" with a NaN val never wins, so NaN pairs are skipped
  double best = __builtin_inf();
  const int npairs = m * (m - 1) / 2;
  for (int p = lane; p < npairs; p += kWave) {
    int i = (int)((1.0 + sqrt(1.0 + 8.0 * (double)p)) / 2.0);
    while (i * (i - 1) / 2 > p) --i;
    while ((i + 1) * i / 2 <= p) ++i;
    const int j = p - i * (i - 1) / 2;
    const double v = w ? pair_stat_weighted(kind, param, B, K, counts + mem[i], ld, counts + mem[j], ld, mv, w)
                       : pair_stat_strided(kind, param, B, K, counts + mem[i], ld, counts + mem[j], ld, mv);
    if (v < best) best = v;
  }
  for (int off = 32; off; off >>= 1) {
    const double o = __shfl_xor(best, off);
    if (o < best) best = o;
  }
  if (lane == 0) out[g] = best;
}

hipError_t launch_group_stats(const Stat& st, const double* d_counts, size_t ld, const int64_t* d_offsets, const int32_t* d_sites,
                              size_t ngroups, double* d_out, hipStream_t stream) {
  if (ngroups == 0) return hipSuccess;
  hipLaunchKernelGGL(group_stat_kernel, dim3((unsigned)ngroups), dim3(kWave), 0, stream, st.kind, st.param, st.B, st.K, d_counts, ld,
                     d_offsets, d_sites, d_out, st.d_mean, st.d_w);
  return hipGetLastError();
}

}  // namespace cmx
