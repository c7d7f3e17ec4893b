// Shared host/device declarations of the MI355X engine (internal; the public surface is include/comap_mi355x.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/comap_mi355x.h"
#include <stddef.h>
#include <stdint.h>

#include "cmx_layout.h"

namespace cmx {

constexpr int kWave = 64;           // gfx950 wavefront
constexpr int kWavesPerBlock = 4;   // mapping kernels: 4 independent waves per 256-thread workgroup
// A mapping wave walks four site groups of 16: lane = site.  (The 16-site class-split launch of small alignments is the one
// other shape, one site group; fewer groups per wave with more waves per SIMD were measured and rejected)
constexpr int map_ng(int) { return 4; }
constexpr int map_sites_per_wave(int S) { return 16 * map_ng(S); }
// Resident mapping waves per SIMD: nucleotide vectors are 8 registers, the kernel is latency-bound and more waves help;
// the other layouts need the 256-register budget of two waves.
// (three waves per SIMD were tried for the 16-state class-fused nucleotide layout -- vectors of 32 registers: at 168
// registers the kernel spills 213 of them and the cfg 4 launch went from 7.7 to 10.7 ms)
constexpr int map_waves_per_simd(int S) { return S == 4 ? 3 : 2; }
// Which mapping instantiations keep one workspace vector per wave in LDS (cmx_walk.h, kLdsSlot): the 64-site walk of the
// 20-state unfused layout.  9 088 B of stage buffers and symbol slots + 10 240 B = 19 328 B per wave, 77 312 B per
// workgroup, two workgroups per CU.
constexpr bool map_lds_slot(int S, int fuse, int ng) { return S == 20 && fuse == 1 && ng == 4; }

// Device-resident model + tree program.  All pointers are device pointers.
struct DevModel {
  int S, C, K, nn, B, T, NI, NIW, NV, root;  // NI internal nodes (operator slots), NIW workspace slots (+ pseudo nodes), NV visited nodes
  // S, C are the DEVICE view: with fuse > 1 (nucleotides, >= 4 rate classes) S = S0 * fuse concatenated per-class states
  // and C = ceil(C0 / fuse) passes; S0, C0 are the model's own state and class counts (simulator, rates, probs, pi)
  int S0, C0, fuse;
  // tree (wave-uniform, read through the scalar cache; simulator only)
  const int* taxon_of;     // [nn]  alignment row of a leaf, -1 for internal nodes
  const int* parent;       // [nn]
  // matrices, [C][MC][mat_unit(S)]: per class a block of packed P | packed (P o N^k) | leaf P^T | leaf (P o N^k)^T | cherry
  // tables (cmx_layout.h: ClassBlock); a matrix use DMAs mat_unit(S)*8 bytes from MAT + (class*MC + index)*mat_unit(S) into LDS
  double* MAT;
  int MC;
  // tree walk of one rate-class pass (cmx_walk.h; built by cmx_host_tree.cpp, checked by cmx_host_verify.cpp)
  const int* nrec;         // [NV][16] per-visited-node records
  const int* msched;       // operator uses in program order: pairs (element offset in the class block, taxon or -1),
                           // followed by copies of its first two pairs (the op two ahead is read without a wrap test)
  int nmv;                 // number of pairs
  // the stream of the walk over resolved alignments (the null's) where it differs from msched, or null: the cherry-table
  // walk's (class-fused nucleotide models), or the 64-site protein walk's with the cherry message table (cmx_walk.h:
  // kCherryMsg; the kernels read its first entries here and the planned copy at MapArgs::plan_r)
  const int* msched_r;
  int nmv_r;
  // the planned stream of the 64-site protein walk (cmx_layout.h: PlanEntry): planned_stream_copies(C) copies of nmv + 2
  // entries; null for every other model.  (In the slot of the load schedule the device once read: the kernel-argument
  // layout is the parent's, and with it the text of the kernels that do not read the plan.)
  const PlanEntry* plan;
  // simulator: running sums of the rows of P, [C][nn][S(x)][S], and a 32-entry guide table per row (see draw_guided)
  const double* CP;
  const uint8_t* CPG;      // [C][nn][S(x)][32]
  const int* simg;         // [nsimg][16] groups of four nodes of equal depth: nodes | parents | taxa (or -1) | pad
  int nsimg;
  const int* simord;       // [nn - 1] the non-root nodes level by level: a node's parent was drawn a whole level earlier
  // continuous-rate simulator: eigensystems of the generators [NM][S*S] / [NM][S], generator and length of each branch
  const double *eigV, *eigVi, *eigLam;
  const int* model_of;     // [B]
  const double* blen;      // [nn]
  const double* pi;        // [S]
  const double* rates;     // [C]
  const double* probs;     // [C]
  const double* cum_pi;    // [S]
  const double* cum_probs; // [C]
};

// Read-only, wave-uniform metadata (tree program, schedules, pi, class rates) is read through the CONSTANT address
// space so that hipcc emits s_load (scalar cache, lgkmcnt) instead of global_load + v_readfirstlane: the latter would
// queue every dependent tree-walk step behind the HBM prefetches outstanding on vmcnt.
typedef const int __attribute__((address_space(4)))* cmx_cint;
typedef const double __attribute__((address_space(4)))* cmx_cdbl;

// Per-wave workspace strides (in elements); every wave owns one slice of each array.
struct Workspace {
  double* D;        // [waves][NIW][S][64]  messages M_n = P_n D_n of internal nodes (inside pass)
  double* U;        // [waves][NIW][S][64]  outside messages arriving at internal nodes
  double* cnt;      // [waves][2][B*K][64]  final counts of the wave's sites (two batches for the null)
  double* part;     // [waves][C][B*K][64]  per-class joint counts, summed in class order at the end
  uint8_t* st;      // unused (null): no wave simulates its own sites any more; the slot keeps the kernel-argument layout
  uint8_t* aln;     // unused (null): as st
  int waves;
};

// kModeObservedSplit: one (site block, rate class) per wave-task for small alignments (an alignment of 2 000 sites is
// 32 site blocks: one task per wave would be four class passes of pure latency), classes summed by map_finalize_kernel
// kModeNullPatterns: the fused null's distinct columns: lane = pattern, walked as kModeNull walks a site, with
// counts / post rate / norm / rate class written per pattern as in observed mode; the pairs are scored afterwards
// kModeNullMsg / kModeNullPatternsMsg: kModeNull / kModeNullPatterns of a 20-state model with a cherry message table
// (cmx_layout.h): the walk gathers an inlined cherry's message from the table (cmx_walk.h: kCherryMsg) and follows the
// resolved stream (DevModel::msched_r, MapArgs::plan_r).  Own modes, so that the other instantiations keep their symbols.
enum MapMode { kModeObserved = 0, kModeNull = 1, kModeObservedSplit = 2, kModeNullPatterns = 3, kModeNullMsg = 4, kModeNullPatternsMsg = 5 };
constexpr bool map_mode_msg(int mode) { return mode == kModeNullMsg || mode == kModeNullPatternsMsg; }
constexpr int map_mode_base(int mode) { return mode == kModeNullMsg ? (int)kModeNull : (mode == kModeNullPatternsMsg ? (int)kModeNullPatterns : mode); }

struct MapArgs {
  DevModel m;
  Workspace ws;
  // observed mode
  const uint8_t* aln;      // [T][ld]
  size_t ld;
  size_t nsites;           // observed: sites; null: (rep_end-rep_begin)*rep_ram null pairs
  double* counts;          // [B*K][ldc] or null
  size_t ldc;
  double* logL;            // [nsites] or null
  double* post_rate;
  int32_t* rate_class;
  double* norm;
  // class-split observed mode: [nblocks][C][B*K][64] per-class counts, [2][nblocks][C][64] p_c L_c and r_c p_c L_c
  double* split_part;
  double* split_lc;
  int split_sites;         // sites per wave-task of the class-split launch: map_sites_per_wave(S), or 16 for small alignments
  int lds_per_wave;        // bytes of dynamic LDS per wave (set by launch_map)
  // null mode
  int stat_kind;
  double stat_param;       // discrete-MI threshold
  const double* stat_mean; // CorrectedCorrelation: [2][B] mean vectors of the two operands (device), else null
  // (the two slots once held the in-kernel simulator's seed and first replicate: the kernel-argument layout is the parent's)
  const PlanEntry* plan_r; // kModeNullMsg / kModeNullPatternsMsg: the planned copy of the resolved stream (layout of DevModel::plan), else null
  const uint8_t* cherry_msg;   // ... and the cherry message table behind its node index (cmx_layout.h: cherry_msg_header_bytes), else null
  size_t rep_ram;
  const uint8_t* supplied; // [nrep][2][T][rep_ram] or null
  double* null_stat;       // [nsites]
  int32_t* null_rcmin;
  double* null_prmin;
  double* null_nmin;
  // pattern mode (appended: the fields above keep their kernel-argument offsets): the pass's site of the first occurrence
  // of every pattern, and the number of patterns (device; the grid is sized for every site its own pattern)
  const uint32_t* rep_site;
  const uint32_t* npat;
  // ... counts is then the tile-major pattern table: tile p / kSites is [B*K][kSites] doubles, pattern p its column p % kSites
  // (kSites patterns per wave: the block map_sites_wave's epilogue writes)
  // how blocks reach the waves (appended as well).  Null: wave w maps blocks w, w + nwaves, ...  Otherwise a
  // device counter the launch's stream has set to nwaves: a wave maps block w first, then the blocks it draws from the counter
  // (next_block, cmx_map.hip).  kModeObservedSplit ignores it.
  unsigned long long* queue;
};
// The code hipcc emits for the mapping kernels depends on where these structures' fields sit in the kernel argument
// (DESIGN.md 4.5.4): an unused field keeps its slot.
static_assert(sizeof(DevModel) == 256 && sizeof(Workspace) == 56 && sizeof(MapArgs) == 520 && offsetof(MapArgs, rep_site) == 496 &&
                  offsetof(MapArgs, queue) == 512 && offsetof(MapArgs, plan_r) == 432 && offsetof(MapArgs, cherry_msg) == 440,
              "kernel-argument layout of the mapping kernels");

// ---- the pair stage's shapes: host structures (the kernels keep taking their pointers one by one, as with MicaSide)
// how a block of pairs lies in the matrix of all pairs (the kernels' `int intra`): two data sets, every pair; one data set, pairs
// j <= i are NaN; a row block of one data set's upper triangle, pairs j <= i are left to the caller, who never reads them
enum PairMode : int { kPairRectangle = 0, kPairOneSet = 1, kPairUpperRows = 2 };
// A statistic with its parameters resolved for one call (resolve_stat, cmx_ctx.h): the DiscreteMI threshold,
// CorrectedCorrelation's mean vectors or the MI bounds on the device, the branch weights.
struct Stat {
  int kind = 0;                      // as the caller named it
  int gk = 0;                        // CorrectedCorrelation -> Correlation: the same Gram and epilogue
  int B = 0, K = 0;
  double param = 0.0;                // DiscreteMI: the threshold
  const double* d_mean = nullptr;    // CorrectedCorrelation: [2][B]
  const double* d_w = nullptr;       // the context's weights where the kind uses them
  int nb = 0;                        // DiscreteMI with bounds
  const double* d_bounds = nullptr;
  bool mi() const { return kind == CMX_STAT_DISCRETE_MI_BOUNDS; }
};
// One data set as the pair kernels read it: the Gram operand X [Bp][ldx] with the per-site vectors s and r, or (MI with
// bounds) the class words [B][ldx] with the per-site out-of-range flags.
struct PairOperand {
  double *X = nullptr, *s = nullptr, *r = nullptr;
  uint32_t* cls = nullptr;
  uint8_t* bad = nullptr;
  size_t n = 0, ldx = 0;
  PairOperand rows(size_t i0, size_t nrows) const {   // the sites [i0, i0 + nrows) as an operand of their own (a row block's rows)
    return {X ? X + i0 : X, s ? s + i0 : s, r ? r + i0 : r, cls ? cls + i0 : cls, bad ? bad + i0 : bad, nrows, ldx};
  }
};
inline int pair_Bp(int B) { return (B + 3) / 4 * 4; }
// one data set's per-site columns: rate class, posterior rate, norm
struct SiteCols { const int32_t* rc = nullptr; const double *pr = nullptr, *nm = nullptr; };
// the four results of a pair (a null: an entry per pair): statistic, smaller rate class, posterior rate and norm; null: not asked for
struct PairOut {
  double* stat = nullptr;
  int32_t* rcmin = nullptr;
  double *prmin = nullptr, *nmin = nullptr;
  PairOut at(size_t o) const { return {stat + o, rcmin ? rcmin + o : nullptr, prmin ? prmin + o : nullptr, nmin ? nmin + o : nullptr}; }
};
// the clustering null's Gram: nblk independent site blocks (grid.z) of the operands' n sites each, block z at site offset
// z * zsite of s / r, its operand at z * zx, its output at z * zout
struct GramBatch { size_t nblk, zsite, zout, zx; };
// what a row pass keeps between its calls: the runs' counts (then offsets) and the scan's temporary (null: the call only sizes it)
struct RowScan { unsigned long long* rowcount = nullptr; void* tmp = nullptr; size_t tmp_bytes = 0; };

// launchers by source file (cmx_map.hip; pair_diag and group_stats are there for map_kernel's sake)
hipError_t launch_map(const MapArgs& a, int mode, int grid_blocks, hipStream_t stream);
// sets a block counter (MapArgs::queue) to `first` on the stream of the launch that will draw from it
hipError_t launch_map_queue_init(unsigned long long* queue, unsigned long long first, hipStream_t stream);
hipError_t launch_map_finalize(const MapArgs& a, hipStream_t stream);
// fills rows S.. of every leaf operator from d_masks[S .. S+max_ambig(S)) (null: every state compatible)
hipError_t launch_extend_leaf_rows(const DevModel& m, const uint32_t* d_masks, hipStream_t stream);
// fills the cherry message table of a 20-state model (cmx_layout.h) with the walk's own code: d_ops [cherries][4] = matrix index
// in a class block of the leaf operators of l1 and l2 and of the cherry's P, pad; d_table: the rows behind the header
hipError_t launch_cherry_msg(const DevModel& m, const int* d_ops, int cherries, uint8_t* d_table, hipStream_t stream);
// pairs (j of data set 1, j of data set 2), j < n: the members of `out` that are set
hipError_t launch_pair_diag(const Stat& st, const double* c1, size_t ld1, const SiteCols& s1, const double* c2, size_t ld2,
                            const SiteCols& s2, size_t n, const PairOut& out, hipStream_t stream);
hipError_t launch_group_stats(const Stat& st, const double* d_counts, size_t ld, const int64_t* d_offsets, const int32_t* d_sites,
                              size_t ngroups, double* d_out, hipStream_t stream);
// (cmx_simulate.hip)
hipError_t launch_simulate(const DevModel& m, uint64_t seed, uint64_t g0, size_t n, uint8_t* d_aln, size_t ld,
                           int32_t* d_classes, uint8_t* d_states, hipStream_t stream, size_t rep_ram = 0, uint64_t gstep = 0);
hipError_t launch_simulate_continuous(const DevModel& m, uint64_t seed, uint64_t g0, size_t n, double alpha, double p_inv,
                                      uint8_t* d_aln, size_t ld, double* d_rates, uint8_t* d_states, hipStream_t stream);
// when the null's simulator launches simulate_chain_kernel instead of the gather kernel (the sizes are the caller's:
// cmx_debug_sim_sites, cmx_api_ctx.cpp)
struct SimChoice {
  const uint8_t* simtab;        // HostModel::simtab on the device, or null: the model has none and takes the gather kernel
  long long min_sites;          // sites of a launch from which the chain kernel runs; < 0: the built-in constant
  long long four_batch_sites;   // ... from which it draws four batches per workgroup; < 0: the built-in constant
};
hipError_t launch_simulate_blocked(const DevModel& m, uint64_t seed, uint64_t g0, size_t nsites, size_t blk, uint8_t* d_aln,
                                   uint8_t* d_states, size_t chunk, hipStream_t stream, const SimChoice& choice);
// (cmx_pairs.hip) the operand of st.gk into o (d_mvec: this data set's mean vector or null; blk: an operand block per `blk` sites,
// 0: one block); the statistic of all pairs of a's and b's sites, rows irow0 .. of the full matrix
hipError_t launch_pair_prep(const Stat& st, const double* d_counts, size_t n, size_t ldc, const double* d_mvec, size_t blk,
                            const PairOperand& o, hipStream_t stream);
hipError_t launch_pair_gram(const Stat& st, const PairOperand& a, const PairOperand& b, PairMode mode, double* d_out, size_t ldo,
                            const GramBatch& z, size_t irow0, hipStream_t stream);
// (cmx_stat_mi.hip) DiscreteMI with a bounds vector: class words [B][ldx] (class | marginal count << 16) + per-site
// out-of-range flags; all-pairs block, diagonal pairs, groups
hipError_t launch_mi_classify(const Stat& st, const double* d_counts, size_t n, size_t ldc, const PairOperand& o, hipStream_t stream);
hipError_t launch_mi_pairs_block(int B, const PairOperand& a, const PairOperand& b, PairMode mode, double* d_out, size_t ldo,
                                 size_t irow0, hipStream_t stream);
hipError_t launch_mi_pairs_diag(int B, const PairOperand& a, const PairOperand& b, size_t n, double* d_out, hipStream_t stream);
hipError_t launch_mi_group(int B, const PairOperand& g, const int64_t* d_offsets, const int32_t* d_sites, size_t ngroups,
                           double* d_out, hipStream_t stream);
// (cmx_variants.hip over cmx_plain.h) the plain kernels: one thread per (site, class), (site, branch) or (site, internal node) over per-node
// vectors in a global scratch.  Four uses: nijt.average = no; nijt.joint = no (the two marginal mappings); the default
// mapping, likelihood and site scalars of the alphabets the matrix-core walk does not serve (states padded to
// kPlainStates); marginal ancestral states.
// PlainMode: which LegacySubstitutionMappingTools function (CoETools.cpp:395-405); Joint is the default mapping
// (computeSubstitutionVectors: averaged, joint), built for kPlainStates only
enum class PlainMode : int { NoAvg = 0 /* NoAveraging */, Marginal = 1, NoAvgMarginal = 2 /* NoAveragingMarginal */, Joint = 3 };
struct PlainArgs {
  int S, C, K, nn, B, root;
  PlainMode mode;
  int Sreal;              // states of the alphabet; < S on the plain path, whose operators are padded with zeros to S = 64
  const double* PN;       // [C][B][K][S*S] joint counts P o N^k (PlainMode::Joint)
  const double* rates;    // [C] (site scalars)
  double *logL, *post_rate;   // [ld...] per site, optional: likelihood, posterior rate, rate class (plain path)
  int32_t* rate_class;
  const int *first_child, *next_sib, *taxon_of, *parent;
  const double* P;        // [C][B][S*S] row-major transition matrices
  const double* N1;       // [B][K][S*S] conditional counts at the branch length itself
  const double* NC;       // [C][B][K][S*S] conditional counts at r_c t_b (PlainMode::Marginal)
  const double *pi, *probs;
  const uint32_t* masks;  // compatibility masks of the codes >= S (NULL: every state)
  const uint8_t* aln;
  size_t ld, site0, nsites, chunk;   // chunk: sites per pass (plain_sites_per_pass)
  double *D, *M, *U, *Up;  // [C][nn][S][chunk], carved from the scratch by the launchers
  double* counts;          // [B*K][ldc]
  size_t ldc;
};
static_assert(sizeof(PlainArgs) == 240 && offsetof(PlainArgs, mode) == 24 && offsetof(PlainArgs, counts) == 224,
              "kernel-argument layout of the plain kernels");
// doubles of the four per-node vectors of `chunk` sites, and the sites of a pass that keeps them under budget_bytes: whole
// workgroups of 256 sites, at least one.  balanced: passes of equal size rounded up to 256 (ancestral states); otherwise full
// passes and a remainder (the mapping)
size_t plain_node_doubles(int S, int C, int nn, size_t chunk);
size_t plain_sites_per_pass(int S, int C, int nn, size_t nsites, size_t budget_bytes, bool balanced);
// the exponents of a context with per-site likelihood scaling (cmx_set_likelihood_scaling): int32s of the inside
// and the outside vectors' exponents of `chunk` sites (eD, then eU), outside the pass budget
size_t plain_exponent_ints(int C, int nn, size_t chunk);
// scratch: plain_node_doubles(a.S, a.C, a.nn, a.chunk) doubles; exps: null, or plain_exponent_ints(a.C, a.nn, a.chunk) int32s for
// the scaled kernels (every mode and the site scalars at 4, 20 and kPlainStates states); d_norm (or null) over all
// nsites_total sites after the last pass
hipError_t launch_plain_map(PlainArgs a, size_t nsites_total, double* scratch, int32_t* exps, double* d_norm, hipStream_t stream);
// asr.method = marginal (cmx_ancestral_states*): states [n_inner][lds], optional posterior [n_inner][Sreal][ldp]
hipError_t launch_ancestral(PlainArgs a, size_t nsites_total, double* scratch, int32_t* exps, const int* d_inner, int n_inner,
                            uint8_t* d_states, size_t lds, double* d_post, size_t ldp, hipStream_t stream);
// computeNormForSite over branch-major counts [B*K][ldc] of n sites (what launch_plain_map ends with)
hipError_t launch_counts_norm(const double* d_counts, size_t ldc, int B, int K, size_t n, double* d_norm, hipStream_t stream);
// the site scalars of one pass of the plain path (site_scalars_kernel on the root's a.D; a.S == kPlainStates), for the wide mapping
hipError_t launch_plain_site_scalars(const PlainArgs& pass, hipStream_t stream);
// the same under likelihood scaling (scaled_site_scalars_kernel; a.S == 20 or kPlainStates), eD / eU: the pass's exponents
hipError_t launch_scaled_site_scalars(const PlainArgs& pass, int32_t* eD, int32_t* eU, hipStream_t stream);
// (cmx_map_wide.hip) PlainMode::Joint and the site scalars on the f64 matrix instruction: the pass structure, the scratch and
// the arithmetic of launch_plain_map, which it replaces by default at kPlainStates states without likelihood scaling and, with
// it, at kPlainStates and at 20 states.  Operators packed by wide_op_offset / wide20_op_offset (cmx_layout.h), uploaded beside
// the plain ones.
struct WideOps {
  const double* P;    // [C][B] transition matrices
  const double* PT;   // [C][B] their transposes
  const double* PN;   // [C][B][K] joint counts P o N^k
};
int map_wide_plain(int on);     // cmx_debug_map_wide_plain: set (on >= 0) / query, returns the previous state
int map_scaled_plain(int on);   // cmx_debug_map_scaled_plain, likewise
// part: the per-class partial counts [C][B*K][chunk] and the likelihoods [chunk] (unscaled: wide_part_doubles doubles), with
// likelihood scaling the likelihoods' int32 exponents [chunk] behind them (wide_scaled_part_bytes bytes)
size_t wide_part_doubles(int C, int B, int K, size_t chunk);
size_t wide_scaled_part_bytes(int C, int B, int K, size_t chunk);
// exps: null, or the plain_exponent_ints(a.C, a.nn, a.chunk) int32s of launch_plain_map for the scaled kernels
hipError_t launch_wide_map(PlainArgs a, const WideOps& o, size_t nsites_total, double* scratch, int32_t* exps, double* part,
                           double* d_norm, hipStream_t stream);
// (cmx_map_wide20.hip) its 20-state shape, scaled only; launch_wide_map dispatches to it
hipError_t launch_wide20_scaled_map(const PlainArgs& a, const WideOps& o, size_t nsites_total, double* scratch, int32_t* exps, double* part,
                                    double* d_norm, hipStream_t stream);
// (cmx_mica_post.hip) Mica post-processing
hipError_t launch_mica_average(const double* d_mi, size_t n, size_t ld, double* d_avg, double* d_full, hipStream_t stream);
hipError_t launch_mica_zscore(int which, const double* d_mi, size_t n, size_t ld, const double* d_avg, const double* d_full,
                              const double* d_key, double* d_stat, double* d_outkey, hipStream_t stream);
// (cmx_mica_perm.hip) the permutation test for 4 / 20 states; the taxon limit of both families is mica_perm_max_taxa(),
// cmx_mica_perm.h
hipError_t launch_mica_colcount(const uint8_t* d_aln, int T, size_t n, size_t ld, int A, const uint8_t* d_emap, uint16_t* d_cnt,
                                uint16_t* d_ext, uint8_t* d_hasamb, int* d_bad, hipStream_t stream);
hipError_t launch_mica_colorder(const uint8_t* d_aln, int T, size_t n, size_t ld, int A, const uint8_t* d_emap, const uint16_t* d_ext,
                                uint16_t* d_order, hipStream_t stream);
// LDS of one wave of the kernel for pairs with non-states, `namb` distinct ones at most in a column (0: it does not fit one workgroup)
size_t mica_perm_general_lds(int T, int A, int namb);
// d_F: the fixed-point table of the pairs with non-states (L^2 T + 1 entries), or null when every column is resolved
// (d_order, d_emask, d_ewgt, L, namb are not read then)
hipError_t launch_mica_perm(int A, int T, const uint8_t* d_aln, size_t ld, size_t n, const uint16_t* d_colcnt, const uint8_t* d_hasamb,
                            const uint8_t* d_emap, const uint16_t* d_ext, const uint16_t* d_order, const uint32_t* d_emask,
                            const uint32_t* d_ewgt, const long long* d_dF, const long long* d_F, uint32_t L, int namb, uint32_t max_perm,
                            uint64_t seed, size_t pair_begin, size_t pair_end, double* d_pvalue, int32_t* d_nperm, int cu_count,
                            hipStream_t stream);
// (cmx_mica_perm_wide.hip) the permutation test for alphabets other than 4 / 20 states: no mask table, codes >= A are unknowns
hipError_t launch_mica_permw_classify(int A, int T, const uint8_t* d_aln, size_t ld, size_t n, uint16_t* d_end, uint16_t* d_unk,
                                      uint8_t* d_flag, uint16_t* d_order, int* d_any, hipStream_t stream);
// d_F: the fixed-point table of the unknowns' path (A^2 T + 1 entries), or null when no column has unknowns
hipError_t launch_mica_permw(int A, int T, const uint8_t* d_aln, size_t ld, size_t n, const uint16_t* d_end, const uint16_t* d_unk,
                             const uint8_t* d_flag, const uint16_t* d_order, const long long* d_dF, const long long* d_F,
                             uint32_t max_perm, uint64_t seed, size_t pair_begin, size_t pair_end, double* d_pvalue, int32_t* d_nperm,
                             int cu_count, hipStream_t stream);
// (cmx_cluster.hip)
size_t hclust_lds_bytes(int n);
size_t cluster_props_lds_bytes(int n);
hipError_t launch_dist_finish(int dist_kind, double* d_D, size_t n, size_t ld, size_t mat_stride, size_t batch,
                              hipStream_t stream);
hipError_t launch_hclust(int linkage, double* d_D, size_t n, size_t ld, size_t mat_stride, size_t batch, double* d_rmin,
                         int* d_nn, int32_t* d_merge, double* d_dmax, int32_t* d_size, hipStream_t stream);
hipError_t launch_cluster_props(int dist_kind, int n, int B, int K, size_t batch, const int32_t* d_merge, const double* d_dmax,
                                const double* d_norm, const double* d_counts, size_t ldc, size_t site_stride, double* d_sigma,
                                double* d_stat, double* d_nmin, hipStream_t stream);
// (cmx_null_patterns.hip) the fused null's patterns.  Sites g of a pass: [replicate][batch][taxon][rep_ram] alignments,
// g = (rep * 2 + batch) * rep_ram + j.  Columns are copied site-major, null_pattern_row_bytes(T) bytes each.
size_t null_pattern_row_bytes(int T);
hipError_t null_pattern_tmp_bytes(size_t n, int hash_bits, size_t* bytes);   // rocPRIM temporary of a pass of n sites
struct NullPatternBufs {
  uint64_t *key, *key_s;   // [n] column hashes (low hash_bits bits), sorted
  uint32_t *g, *g_s;       // [n] site index, in hash order
  uint8_t* col;            // [n][row bytes] packed columns
  uint32_t* head;          // [n] sorted position of the first element of each sorted element's run
  uint32_t* incl;          // [n] inclusive sum over g of "g is the first site of its run": pattern of a first site + 1
  uint32_t* pat_of;        // [n] pattern of site g
  uint32_t* rep_site;      // [n] first site of pattern p (the first incl[n - 1] entries)
  unsigned long long* total;   // patterns of every pass so far are added here
  void* tmp;
  size_t tmp_bytes;
};
// key + packed copy, stable radix sort of (hash, g), run flags, the two scans, pattern numbers in first-occurrence order
hipError_t launch_null_patterns(const uint8_t* d_sup, int T, size_t rep_ram, size_t n, int hash_bits, const NullPatternBufs& b,
                                hipStream_t stream);
// Correlation / Covariance: mean over branches and sum of squared deviations of every pattern of the pass (pattern_moments),
// one thread per pattern, after the mapping; npat on the device, the grid sized for cap patterns
hipError_t launch_null_pattern_moments(int B, int K, const double* counts, int tile_sites, int tile_row, const uint32_t* npat,
                                       size_t cap, double* pat_mean, double* pat_ss, hipStream_t stream);
// statistic and minima of pair q = (rep, j) from the patterns of sites (rep, 0, j) and (rep, 1, j); counts in tiles of
// [B*K][tile_row] doubles, tile_sites patterns each (MapArgs); pat_mean / pat_ss for Correlation and Covariance; pat: the
// patterns' columns
hipError_t launch_null_pattern_pairs(const Stat& st, const double* counts, int tile_sites, int tile_row, const double* pat_mean,
                                     const double* pat_ss, const SiteCols& pat, const uint32_t* pat_of, size_t rep_ram, size_t npairs,
                                     const PairOut& out, hipStream_t stream);
// (cmx_rows.hip)
hipError_t launch_max_reduce(const double* d_x, size_t n, double* d_out, hipStream_t stream);
hipError_t launch_null_classify(const double* d_stat, const double* d_nmin, size_t nnull, const double* d_maxnorm,
                                int nclasses, uint32_t* d_cls, uint32_t* d_hist, hipStream_t stream);
// The null distribution prepared for p-value lookups: statistics sorted by (class, value), and per class a table of
// bins of equal width in the statistic's value, one bin per kNullBinSize sorted values: bins[b] = index of the first value
// of the class that falls into bin b or later.  A lookup computes its bin and searches the few values inside it.
constexpr int kNullBinShift = 3, kNullBinSize = 1 << kNullBinShift;
constexpr int kPairRowSegs = 8;   // waves per row in the pair-row passes (pair_rows_kernel)
struct NullClass {
  uint32_t off, ns;         // the class's stretch of `sorted`
  uint32_t nb, boff;        // number of bins (>= 1), and where its nb + 1 entries start in `bins`
  double lo, scale;         // bin of v = clamp(floor((v - lo) * scale), 0, nb - 1)
};
struct NullTable {
  const double* sorted;     // [nnull] ascending inside each class, classes in order
  const NullClass* cls;     // [nclasses]
  const uint32_t* bins;     // [(nnull >> kNullBinShift) + 2 * nclasses + 2]
  const double* maxnorm;    // upper bound of the Domain of the norms
  int nclasses;
};
hipError_t launch_null_index(const double* d_sorted, const uint32_t* d_hist, int nclasses, size_t nnull, NullClass* d_cls,
                             uint32_t* d_bins, hipStream_t stream);
// nrows rows irow0 .. of the full matrix
hipError_t launch_pvalues(const double* d_stat, size_t ldo, const double* d_norms, size_t n, const NullTable& nt, double* d_pvalue,
                          int32_t* d_nsim, size_t irow0, size_t nrows, hipStream_t stream);
hipError_t sort_null_by_class(void* d_tmp, size_t& tmp_bytes, double* d_stat_in, double* d_stat_tmp, uint32_t* d_cls_in,
                              uint32_t* d_cls_tmp, size_t n, hipStream_t stream);
hipError_t launch_pair_rows(const double* d_stat, size_t ldo, const double* d_pvalue, const int32_t* d_nsim, size_t n, const SiteCols& s,
                            const cmx_pair_filters& f, RowScan& scan /* rowcount [nrows * kPairRowSegs + 1] */, cmx_pair_row* d_rows,
                            size_t capacity, unsigned long long* d_count, size_t irow0, size_t nrows, const unsigned long long* d_base,
                            const NullTable* d_inline_null, hipStream_t stream);
hipError_t launch_pair_compact(const double* d_stat, size_t ldo, size_t n, const double* d_norm, const NullTable* nt, cmx_pair_compact* d_out,
                               size_t capacity, hipStream_t stream, size_t irow0, size_t nrows, size_t row_begin);
hipError_t launch_inter_rows(const double* d_stat, size_t ldo, size_t n2, const SiteCols& s1, const SiteCols& s2, const cmx_inter_filters& f,
                             RowScan& scan /* rowcount [nrows + 1] */, cmx_pair_row* d_rows, size_t capacity, unsigned long long* d_count,
                             size_t irow0, size_t nrows, const unsigned long long* d_base, hipStream_t stream);
// (cmx_mica.hip)
hipError_t launch_mi_pairs(int A, int T, const uint32_t* d_masks, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2,
                           size_t ld2, const int64_t* d_idx1, const int64_t* d_idx2, size_t npairs, double* d_mi,
                           double* d_hj, hipStream_t stream);
// The column stage.  mica_path alone decides which kernels serve a call -- the LDS-table kernel only; beside it the four-wave
// or the eight-wave protein kernel, the four-wave or the one-column-per-tile nucleotide kernel; or none (hipErrorInvalidValue):
// cmx_mi_columns_dev requests scratch from it, launch_mi_columns dispatches on it.  Every size the host shares with a Mica
// kernel is a function beside that kernel (mica_ftab_entries, mica4_info_words, mica4_image_bytes, the *_lds_bytes).
// Alphabets other than 4 / 20 states (cmx_mica_wide.hip): the matrix-core kernel of that file, or its plain kernel alone (above
// 2 047 taxa, or under cmx_debug_mica_wide_plain).
enum MicaPath { kMicaTables, kMicaProtein4, kMicaProtein8, kMicaDna4, kMicaDna1, kMicaWide, kMicaWidePlain, kMicaRefused };
MicaPath mica_path(int A, int T, size_t n1, size_t n2);
constexpr int mica_padded_taxa(int T) { return (T + 31) / 32 * 32; }   // whole MFMA steps of 32 taxa
constexpr int kMicaLdsF2 = 4096;   // entries of f2 the weighted four-wave kernel keeps in LDS (m < 4096: cells of up to ten taxa)
constexpr int kMicaCodePad = 64;   // columns of "no row" symbols behind the last column of C / Cs (the four-wave kernels read whole tiles: 12 / 64 columns)
// scratch of one alignment on the MFMA paths (device pointers; null where the path does not read it)
struct MicaSide {
  size_t n;          // columns
  int8_t* H;         // [n][32][Tp] one-hot int8 (kMicaDna1)
  uint8_t* C;        // [n + kMicaCodePad][Tp] one-hot row of each taxon (state, A = unknown, 63 = none); kMicaWide: [n][Tp], state or 255 = none
  uint8_t* flag;     // [n] column has ambiguous symbols other than "unknown" (-> LDS-table kernel)
  uint8_t* gap;      // [n] column has unknowns (gap / X / N: compatible with every state; handled on the matrix cores)
  double* S;         // [n] sum_a f(count_a)
  unsigned* info;    // [mica4_info_words(n)] per block of three SORTED columns: not-served and has-unknowns bits (kMicaProtein4, as the four below)
  unsigned* order;   // [n] original column of a sorted position (columns without unknowns first, stable)
  uint8_t* Cs;       // [n + kMicaCodePad][Tp] symbol bytes in sorted order
  double* Ss;        // [n] column sums in sorted order
  int* cnt;          // [n][A] integer state counts (kMicaWide, kMicaWidePlain, as the next)
  int* unk;          // [n] unknowns of the column
};
struct MicaWork {
  MicaSide s[2];     // the two alignments (n always set, the rest as mica_path(A, T, s[0].n, s[1].n) needs it); intra layout: s[1] == s[0]
  double* ftab;      // [mica_ftab_entries(A, T)] (mica_ftable_kernel)
  int* anyflag;      // some column of either alignment has ambiguous symbols
  void* img2;        // [mica4_image_bytes(Tp, s[1].n)] the second alignment's expanded operands by tile (kMicaProtein4)
  int Tp;            // mica_padded_taxa(T)
};
size_t mica_ftab_entries(int A, int T);
// dynamic LDS beyond the 64 KiB a kernel may use unasked
template <class K>
hipError_t mica_allow_lds(K* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
hipError_t launch_mi_columns(int A, int T, const uint32_t* d_masks, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2,
                             size_t ld2, int intra, double* d_mi, double* d_hj, size_t ldo, double* d_h1, double* d_h2,
                             const MicaWork& work, hipStream_t stream);
// (cmx_mica_wide.hip) alphabets other than 4 / 20 states, up to 64: codes >= A are unknowns, there is no mask table
int mica_wide_plain(int on);                          // cmx_debug_mica_wide_plain: set (on >= 0) / query, returns the previous state
size_t micaw_ftab_entries(int A, int T);               // doubles of its two tables (micaw_ftable_kernel)
size_t micaw_tiles(int A, size_t n1, size_t n2);      // workgroups of the matrix-core kernel (a 32-bit grid)
hipError_t launch_mi_pairs_wide(int A, int T, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2, size_t ld2,
                                const int64_t* d_idx1, const int64_t* d_idx2, size_t npairs, double* d_mi, double* d_hj,
                                hipStream_t stream);
hipError_t launch_mi_columns_wide(int A, int T, const uint8_t* d_aln1, size_t ld1, const uint8_t* d_aln2, size_t ld2, int intra,
                                  double* d_mi, double* d_hj, size_t ldo, double* d_h1, double* d_h2, const MicaWork& work,
                                  hipStream_t stream);
// (cmx_mica4.hip) the four-wave kernels (unknowns included; partial ambiguity codes are not served): proteins, nucleotides
size_t mica4_info_words(size_t n);
size_t mica4_image_bytes(int Tp, size_t n2);
hipError_t launch_mica4(int T, const MicaWork& wk, int intra, double* d_mi, double* d_hj, size_t ldo, hipStream_t stream);
hipError_t launch_mica_dna4(int T, const MicaWork& wk, int intra, double* d_mi, double* d_hj, size_t ldo, hipStream_t stream);
// (cmx_window.hip) The sliding-window conditional p-values of R/CoMapFunctions.R:168-215: the null as a wavelet
// matrix.  All n null entries are indexed; the dropped ones (a NaN statistic or Nmin) sort behind the nkept kept ones in both
// orders, so no query range or rank ever reaches them.
struct WindowHead {          // on the device: what the build finds out about the null
  uint32_t nkept, pad;
  double ws;                 // (max nmin - min nmin) * window / 2 over the kept entries; 0 when there are none
  double nmin_min, nmin_max; // NaN when there are none
};
struct WindowIndex {
  const double* nmin;        // [n] the Nmin of the entries, ascending
  const double* stat;        // [n] the statistics, ascending: position = rank
  const uint2* levels;       // [L][units] per level {ones before the unit, the unit's 32 bits}: bit of an entry = bit L-1-l of its rank
  const uint32_t* zeros;     // [L] zero bits of the level
  const WindowHead* head;
  uint32_t n, units;         // units = ceil(n / 32) + 1: a rank query at position n reads the last one
  int L;                     // max(1, ceil(log2 n))
};
inline int window_levels(size_t n) { int L = 1; while (((size_t)1 << L) < n) ++L; return L; }
inline size_t window_units(size_t n) { return (n + 31) / 32 + 1; }
// the build's temporaries, all [n] but cnt / ones [units]; d_tmp == nullptr: only tmp_bytes (rocPRIM's) is set
struct WindowBuild {
  uint64_t *key_a, *key_b;
  uint32_t *val_a, *val_b, *seq_a, *seq_b, *cnt, *ones;
  void* tmp;
  size_t tmp_bytes;
};
hipError_t launch_window_build(const double* d_null_stat, const double* d_null_nmin, size_t n, double window, WindowBuild& b, double* d_nmin,
                               double* d_stat, uint2* d_levels, uint32_t* d_zeros, WindowHead* d_head, hipStream_t stream);
hipError_t launch_window_test(const WindowIndex& ix, const double* d_stat, const double* d_nmin, size_t nq, const cmx_window_params& p,
                              double* d_pvalue, uint32_t* d_count, uint32_t* d_nobs, hipStream_t stream);
// per site the window of its norm as positions [lo, hi) of the index: the pair loop's m = min(norm_i, norm_j) is one of them
hipError_t launch_window_site_bounds(const WindowIndex& ix, const double* d_norm, size_t n, uint32_t* d_lo, uint32_t* d_hi, hipStream_t stream);
// the record pass of cmx_intra_window_range_dev: launch_pair_compact's rows, positions and arguments
hipError_t launch_pair_window(const double* d_stat, size_t ldo, size_t n, const double* d_norm, const WindowIndex& ix, const uint32_t* d_lo,
                              const uint32_t* d_hi, int lower, cmx_pair_window* d_out, size_t capacity, hipStream_t stream, size_t irow0,
                              size_t nrows, size_t row_begin);
}  // namespace cmx
