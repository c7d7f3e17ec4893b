// What every stage of the C-ABI's host orchestration (cmx_api_*.cpp) shares: the context, error handling, the named scratch
// buffers and their guard, the device temporaries of the host-pointer entry points, and what fills the pair stage's shapes of
// cmx_device.h -- a statistic resolved for one call, a data set as the pair kernels read it, the four result buffers of a null.
// Internal: nothing here is exported (the library's ABI is include/comap_mi355x.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/comap_mi355x.h"
#include "cmx_device.h"
#include "cmx_host_model.h"

using namespace cmx;

#pragma GCC visibility push(hidden)

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;     // capacity the callers may use (the allocation is kGuardBytes longer under the guard)
  size_t logical = 0;   // guard only: what the last caller asked for; the canary sits at [logical, logical + kGuardBytes)
  bool guarded = false; // allocated with room for the canary (a buffer from before the guard was switched on is not)
  size_t allocs = 0;    // how often it was allocated: what a caller that keeps content across calls keys that content on
};

// F[m] = round(m ln m 2^sh), m <= M, of Mica's permutation test (perm_table, cmx_api_mica.cpp): up to 2^26 entries with a
// logarithm each, so the host copy is kept per (M, sh) and the device copy per allocation of the scratch buffer that holds it
struct PermTable {
  std::vector<long long> host;
  size_t M = 0;
  int sh = -1;
  size_t allocs = 0;    // DevBuf::allocs of the buffer `host` was uploaded to (0: none)
};

struct cmx_ctx {
  int device = 0;
  bool has_model = false;
  HostModel hm;
  DevModel dm{};
  Workspace ws{};       // null-distribution launches (persistent grid: 1 wave per SIMD on every CU)
  Workspace ws_obs{};   // observed-alignment launches: own slices, so both kinds can overlap on two streams
  int obs_blocks = 0;
  int cu_count = 0, waves = 0, grid_blocks = 0;
  size_t ws_bytes = 0;
  // block counters of the queued mapping launches (MapArgs::queue, map_queue_take): a ring of kMapQueueRing 64-bit words,
  // allocated with the workspace; the next launch takes word map_queue_turn % kMapQueueRing
  unsigned long long* map_queue = nullptr;
  unsigned map_queue_turn = 0;
  std::vector<void*> model_allocs;
  std::map<std::string, DevBuf> scratch;
  struct GuardedFixed { std::string name; void* p; size_t bytes; };
  std::vector<GuardedFixed> guarded_fixed;   // CMX_SCRATCH_GUARD: the per-wave workspaces, each with a canary after its last byte
  uint32_t* d_default_masks = nullptr;
  const uint8_t* d_simtab = nullptr;   // HostModel::simtab (null: the model has none)
  // the cherry message table of a 20-state model (cmx_layout.h; null: none) behind its node index, and the planned copy of the
  // resolved stream (MapArgs::cherry_msg / plan_r of the null's launches; the stream itself is dm.msched_r)
  uint8_t* d_cherry_msg = nullptr;
  const PlanEntry* d_plan_r = nullptr;
  unsigned stat_mean_turn = 0;
  // host copies of asynchronously uploaded parameter blocks (mean vectors, MI bounds): the source of a hipMemcpyAsync must
  // outlive the copy, and the caller's array need not
  std::vector<double> param_host[8];
  bool leaf_rows_custom = false;   // the leaf operators' ambiguity rows were built from a caller's mask table
  bool map_average = true;         // nijt.average (cmx_set_mapping_options); false: the no-averaging mapping of cmx_variants.hip
  bool map_joint = true;           // nijt.joint; false: the ...Marginal variants of cmx_variants.hip
  // cmx_set_likelihood_scaling: every mapping, null and ancestral-state call goes through the scaled entry points of the
  // plain kernels (cmx_variants.hip), the walk and the fused null are not used
  bool scaling = false;
  // Statistic::setWeights (cmx_set_statistic_weights): the normalised branch weights, host copy + device copy (B doubles,
  // allocated at the first set); empty = unweighted
  std::vector<double> stat_w;
  double* d_stat_w = nullptr;
  // Mica's permutation test: host-side sources of its asynchronous table uploads (they must outlive the copies, also
  // when a later call fails), and the fixed-point table of each family's pairs with non-states (scratch "perm_F": 4 / 20
  // states, "permw_F": the other alphabets -- a caller that alternates keeps both)
  std::vector<long long> perm_dF_host;
  std::vector<uint8_t> perm_tab_host;
  PermTable perm_F, permw_F;
  // cmx_window_null_dev: the index of the sliding-window p-values (scratch "win_*"), read by every later window call
  struct WindowKept { bool built = false; WindowIndex ix{}; } window;
  // cmx_intra_gram_prefetch_dev: the Gram blocks kept for the next cmx_intra_compact_range_dev with the same arguments
  struct GramKept { bool valid = false; int kind = 0; const double* counts = nullptr; size_t n = 0, ldc = 0, row_begin = 0, row_end = 0; const double* stat = nullptr; } gram_kept;
  const double *va_P = nullptr, *va_N1 = nullptr, *va_NC = nullptr;   // their operators, uploaded at first use
  const double *va_PN = nullptr, *va_pi = nullptr;                     // plain path: joint counts and frequencies, padded (va_PN also: scaled mapping at 4 / 20 states)
  const int *va_first = nullptr, *va_next = nullptr;
  WideOps va_wide{};   // va_P, its transpose and va_PN once more, packed for the wide mapping (cmx_map_wide.hip): plain path, or 20 states at the first scaled use
  const int* asr_inner = nullptr;   // cmx_ancestral_states*: the internal nodes, ascending (uploaded at first use)
  int asr_n_inner = 0;
  // the fused null's distinct columns (cmx_set_null_patterns): -1 automatic, 0 off, 1 on; what the last null mapped
  int null_patterns = -1;
  int null_depth = 0;                         // > 0 inside the simulating null's own pass loop (one null, several calls)
  unsigned long long null_mapped_host = 0;    // sites the last null mapped site by site
  bool null_mapped_dev = false;               // ... plus the patterns counted on the device (scratch "pat_total")
  mutable std::string err;
};

#define CMX_TRY(expr)                                                                                        \
  do {                                                                                                       \
    cmx_status s_ = (expr);                                                                                  \
    if (s_ != CMX_OK) return s_;                                                                             \
  } while (0)

#define HIP_TRY(ctx, expr)                                                                                   \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) {                                                                                  \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                                        \
      return CMX_ERR_DEVICE;                                                                                 \
    }                                                                                                        \
  } while (0)

// process-wide state, defined in cmx_api_ctx.cpp
extern thread_local std::string g_create_error;
extern std::atomic<int> g_guard;                       // CMX_SCRATCH_GUARD: -1 not decided yet (environment read at the first context)
extern std::mutex g_guard_mu;
extern std::vector<std::string> g_guard_failures;      // buffers found trampled, in the order found
extern std::map<std::string, size_t> g_guard_shrink;   // test hook: logical size override per buffer name
extern std::atomic<int> g_cherry_msg;                  // cmx_debug_cherry_msg: 0 = contexts created from now on get no cherry message table
extern std::atomic<int> g_pat_hash_bits;               // cmx_debug_null_hash_bits: the fused null's column hash keeps only its low bits
extern std::atomic<int> g_map_queue;                   // cmx_debug_map_queue: 0 = every mapping launch keeps the strided block assignment
extern std::atomic<int> g_map_small_blocks;                 // cmx_debug_map_small_blocks: 0 = no 16-site blocks in the class-split launch
extern std::atomic<long long> g_sim_min_sites;         // cmx_debug_sim_sites: sites of a launch from which simulate_chain_kernel runs (< 0: built in)
extern std::atomic<long long> g_sim_four_batch_sites;  // ... from which it draws four batches per workgroup (< 0: built in)
extern std::atomic<int> g_map_grid;                    // cmx_debug_map_grid: workgroups a new context's mapping launches may use (0: no cap)

inline cmx_status fail(cmx_ctx* ctx, cmx_status s, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return s;
}

inline cmx_status need_model(cmx_ctx* ctx) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!ctx->has_model) return fail(ctx, CMX_ERR_INVALID, "this context was created without a model/tree");
  return CMX_OK;
}

inline cmx_status need_window(cmx_ctx* ctx, const char* who) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!ctx->window.built) return fail(ctx, CMX_ERR_INVALID, std::string(who) + ": no window index was built (cmx_window_null_dev comes first)");
  return CMX_OK;
}

// model tables: uploaded once, released with the context
template <class T>
cmx_status upload(cmx_ctx* ctx, const std::vector<T>& h, const T** d) {
  void* p = nullptr;
  const size_t bytes = sizeof(T) * (h.empty() ? 1 : h.size());
  HIP_TRY(ctx, hipMalloc(&p, bytes));
  ctx->model_allocs.push_back(p);
  if (!h.empty()) HIP_TRY(ctx, hipMemcpy(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
  *d = static_cast<const T*>(p);
  return CMX_OK;
}

// the scratch guard (cmx_api_ctx.cpp): a canary of kGuardBytes after what the caller asked for
constexpr size_t kGuardBytes = 4096;
bool guard_on();
void guard_record(const std::string& what);
hipError_t guard_arm(void* base, size_t logical);
bool guard_intact(const void* base, size_t logical, size_t* first_bad);   // the device must be idle

// grow-only named scratch buffers (allocated on first use, released with the context): `bytes` bytes, or `count` elements
cmx_status scratch(cmx_ctx* ctx, const char* name, size_t bytes, void** out);
template <class T>
cmx_status scratch(cmx_ctx* ctx, const char* name, size_t count, T** out) {
  void* p = nullptr;
  CMX_TRY(scratch(ctx, name, sizeof(T) * count, &p));
  *out = static_cast<T*>(p);
  return CMX_OK;
}

struct TmpDev {  // RAII device temporaries for the host-pointer entry points
  std::vector<void*> ptrs;
  std::vector<size_t> sizes;   // guard only
  ~TmpDev();
  hipError_t alloc_bytes(void** p, size_t bytes);
  template <class T>
  cmx_status alloc(cmx_ctx* ctx, T** p, size_t count) {
    HIP_TRY(ctx, alloc_bytes((void**)p, sizeof(T) * count));
    return CMX_OK;
  }
  template <class T>
  cmx_status upload(cmx_ctx* ctx, T** p, const T* host, size_t count) {   // blocking
    CMX_TRY(alloc(ctx, p, count));
    HIP_TRY(ctx, hipMemcpy(*p, host, sizeof(T) * count, hipMemcpyHostToDevice));
    return CMX_OK;
  }
  // counts of n sites, site-major [n][BK] on the host (the reference's mapping[i][b][k]) -> branch-major [BK][n] on the device
  cmx_status upload_branch_major(cmx_ctx* ctx, double** p, const double* sm, size_t n, size_t BK);
};
// blocking copy to the host; a null host pointer is an output the caller did not ask for
template <class T>
cmx_status download(cmx_ctx* ctx, T* host, const T* dev, size_t count) {
  if (host) HIP_TRY(ctx, hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost));
  return CMX_OK;
}

// the four results of a null (PairOut, n pairs) as device temporaries, and their way back to the host
inline cmx_status alloc_out(cmx_ctx* ctx, TmpDev& tmp, size_t n, PairOut* d) {
  CMX_TRY(tmp.alloc(ctx, &d->stat, n));
  CMX_TRY(tmp.alloc(ctx, &d->prmin, n));
  CMX_TRY(tmp.alloc(ctx, &d->nmin, n));
  return tmp.alloc(ctx, &d->rcmin, n);
}
inline cmx_status fetch_out(cmx_ctx* ctx, size_t n, const PairOut& d, const PairOut& host) {   // host.stat is never null
  CMX_TRY(download(ctx, host.stat, d.stat, n));
  CMX_TRY(download(ctx, host.rcmin, d.rcmin, n));
  CMX_TRY(download(ctx, host.prmin, d.prmin, n));
  return download(ctx, host.nmin, d.nmin, n);
}

inline cmx_status check_kind(cmx_ctx* ctx, int kind) {
  if (kind < CMX_STAT_CORRELATION || kind > CMX_STAT_SCALAR_PRODUCT) return fail(ctx, CMX_ERR_INVALID, "unknown statistic kind");
  return CMX_OK;
}

// the context's weights on the device when `kind` uses them (DESIGN A.7, weighted), else null.  Cosubstitution, the
// discrete MI kinds and the scalar product ignore them as the reference does (Statistics.h:230-245, 307-327).
inline const double* stat_weights(const cmx_ctx* ctx, int kind) {
  if (ctx->stat_w.empty()) return nullptr;
  switch (kind) {
    case CMX_STAT_CORRELATION: case CMX_STAT_CORRECTED_CORRELATION: case CMX_STAT_COVARIANCE: case CMX_STAT_COSINUS:
    case CMX_STAT_COMPENSATION: case CMX_STAT_EUCLIDIAN_DISTANCE:
      return ctx->d_stat_w;
  }
  return nullptr;
}

// the simulator's counter layout (cmx_philox.h philox_uniform): 47 bits of simulated-site index, 17 bits of draw index
inline cmx_status rng_range(cmx_ctx* ctx, uint64_t g_end, const char* who) {
  if (g_end > (1ull << 47) || (uint64_t)ctx->hm.nn + 2 > (1ull << 17))
    return fail(ctx, CMX_ERR_UNSUPPORTED, std::string(who) + ": simulated-site index beyond 2^47 or more than 2^17 - 2 nodes");
  return CMX_OK;
}


// cmx_api_ctx.cpp.  The block counter of a mapping launch of `grid` workgroups over at most nblocks site blocks (pattern mode:
// the blocks of the pass's sites, the waves read the pattern count), for MapArgs::queue: null when there is nothing to balance
// (nblocks <= waves: every wave holds at most one block) or under cmx_debug_map_queue(0); otherwise the context's next ring
// word, set to the launch's wave count on `stream` -- call it right before launch_map on that stream.
constexpr unsigned kMapQueueRing = 256;
cmx_status map_queue_take(cmx_ctx* ctx, size_t nblocks, int grid, hipStream_t stream, unsigned long long** queue);

// cmx_api_map.cpp.  full_grid: the whole-chip workspace of the null launches (the engine's own simulate -> map pipelines)
// instead of the quarter-chip slice of the observed alignments
cmx_status map_sites_impl(cmx_ctx* ctx, const uint8_t* d_aln, size_t nsites, size_t ld, const uint32_t* d_masks, double* d_counts,
                          size_t ldc, double* d_logL, double* d_post_rate, int32_t* d_rate_class, double* d_norm, void* stream,
                          bool full_grid);

// ---- the pair stage's shapes (Stat, PairOperand: cmx_device.h) as cmx_api_pairs.cpp fills them
// params: the DiscreteMI threshold, or CorrectedCorrelation's mean vectors or the MI bounds, uploaded on the caller's stream (one
// turn of the context's rotating parameter buffers); the branch weights are the context's
cmx_status resolve_stat(cmx_ctx* ctx, int kind, const double* params, void* stream, Stat* out);
// prepared on `st` into the scratch buffers of `slot`: "1" / "2" (pair_X1 .., mi_cls_1 ..), "gram" (gram_X1 ..), or a tag of
// the MI classes alone ("n1", "n2", "g").  The second data set ("2") takes the second mean vector.  block: the n sites are
// replicates of `block` sites each, an operand block per replicate (clustering); 0: one block.
cmx_status pair_operand(cmx_ctx* ctx, const Stat& sk, const double* d_counts, size_t n, size_t ldc, const char* slot, hipStream_t st,
                        PairOperand* out, size_t block = 0);
// rows [i0, i0 + rb) of `a` against all of `b` -> out[rb][ldo] (kPairUpperRows: the block's global row i0 places the diagonal)
cmx_status pair_block(cmx_ctx* ctx, const Stat& sk, const PairOperand& a, size_t i0, size_t rb, const PairOperand& b, PairMode mode,
                      double* out, size_t ldo, hipStream_t st);
// the row blocks of the pair loop: <= 256 MiB of statistics of n columns, whole 64-row tiles
inline size_t pair_row_block(size_t n, size_t rows) {
  size_t RB = ((size_t)256 << 20) / (8 * n) / 64 * 64;
  return std::max<size_t>(64, std::min<size_t>(RB, (rows + 63) / 64 * 64));
}

#pragma GCC visibility pop
