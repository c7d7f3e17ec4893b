// C-ABI of the engine (include/comap_mi355x.h).  Host-side orchestration only: uploads the prepared model,
// owns the per-wave workspace, launches the HIP kernels.  There is no CPU compute path: without a HIP device every
// compute entry point fails with CMX_ERR_DEVICE.
// This file: the context, the scratch buffers and their guard, settings and debug hooks.  The stages are in
// cmx_api_map.cpp, cmx_api_null.cpp, cmx_api_pairs.cpp, cmx_api_mica.cpp and cmx_api_cluster.cpp.
#include "cmx_ctx.h"
#include "cmx_host_parts.h"   // children(), OPER_P: the cherry message table's operators

thread_local std::string g_create_error;

// CMX_SCRATCH_GUARD=1 (or cmx_debug_scratch_guard(1)): every scratch buffer, per-wave workspace and temporary is
// allocated kGuardBytes longer, the bytes after what the caller asked for hold a canary, and scratch() (before it hands a
// buffer out again), cmx_synchronize, cmx_scratch_check and cmx_ctx_destroy verify it and name the buffer that was
// written past its end.  Round 3: a scratch buffer sized [nn][rep_ram] for a kernel that writes [nn][nrep * rep_ram] lived
// through a round of green tests on allocator slack.  Debug mode: every check synchronises the device.
constexpr int kGuardByte = 0xC5;
std::atomic<int> g_guard{-1};
std::mutex g_guard_mu;
std::vector<std::string> g_guard_failures;
std::map<std::string, size_t> g_guard_shrink;

std::atomic<int> g_lds_slot{1};         // cmx_debug_lds_slot: 0 = the mapping walk's LDS slot is planned empty (A/B runs, tests)
std::atomic<int> g_cherry_msg{1};       // cmx_debug_cherry_msg: 0 = no cherry message table, the null of a 20-state model walks the plain stream (A/B runs, tests)
std::atomic<int> g_pat_hash_bits{64};   // (tests force collisions with it)
std::atomic<int> g_map_queue{1};        // cmx_debug_map_queue: 0 = strided block assignment in every mapping launch (A/B runs, tests)
std::atomic<int> g_map_small_blocks{1};      // cmx_debug_map_small_blocks: 0 = the class-split launch of a protein alignment keeps 64-site blocks (tests)
std::atomic<long long> g_sim_min_sites{-1};          // cmx_debug_sim_sites (tests: the chain kernel's shapes at small sizes)
std::atomic<long long> g_sim_four_batch_sites{-1};
std::atomic<int> g_map_grid{0};         // cmx_debug_map_grid: cap of a new context's grid_blocks / obs_blocks (tests: many rounds of blocks on few waves)

bool guard_on() {
  int g = g_guard.load();
  if (g < 0) {
    const char* e = getenv("CMX_SCRATCH_GUARD");
    g = (e && e[0] == '1') ? 1 : 0;
    g_guard.store(g);
  }
  return g == 1;
}

void guard_record(const std::string& what) {
  std::lock_guard<std::mutex> lk(g_guard_mu);
  g_guard_failures.push_back(what);
  std::fprintf(stderr, "CMX_SCRATCH_GUARD: %s\n", what.c_str());
}

hipError_t guard_arm(void* base, size_t logical) {
  return hipMemset(static_cast<char*>(base) + logical, kGuardByte, kGuardBytes);
}

// true when the canary after `logical` bytes is intact; the device must be idle
bool guard_intact(const void* base, size_t logical, size_t* first_bad) {
  static thread_local std::vector<unsigned char> h(kGuardBytes);
  if (hipMemcpy(h.data(), static_cast<const char*>(base) + logical, kGuardBytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
  for (size_t i = 0; i < kGuardBytes; ++i)
    if (h[i] != (unsigned char)kGuardByte) { if (first_bad) *first_bad = i; return false; }
  return true;
}

// grow-only named scratch buffers (allocated on first use, released with the context)
cmx_status scratch(cmx_ctx* ctx, const char* name, size_t bytes, void** out) {
  DevBuf& b = ctx->scratch[name];
  if (guard_on()) {
    // the previous user's canary is checked before the buffer is handed out again (it may move with the size asked for)
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (b.p && !b.guarded) {   // allocated before the guard was switched on: no room for a canary, start over
      HIP_TRY(ctx, hipFree(b.p));
      b.p = nullptr;
      b.bytes = 0;
    }
    size_t off = 0;
    if (b.p && !guard_intact(b.p, b.logical, &off)) {
      const std::string msg = std::string("buffer 'scratch:") + name + "' was written past its end (" + std::to_string(b.logical) +
                              " bytes asked for, first bad byte at +" + std::to_string(off) + ")";
      guard_record(msg);
      (void)guard_arm(b.p, b.logical);
      return fail(ctx, CMX_ERR_INTERNAL, "CMX_SCRATCH_GUARD: " + msg);
    }
    size_t logical = bytes ? bytes : 16;
    {
      std::lock_guard<std::mutex> lk(g_guard_mu);
      auto it = g_guard_shrink.find(name);
      if (it != g_guard_shrink.end() && it->second < logical) logical = it->second;   // test hook: pretend the caller asked for less
    }
    if (b.bytes < bytes || !b.p) {
      if (b.p) HIP_TRY(ctx, hipFree(b.p));
      b.p = nullptr;
      b.bytes = 0;
      HIP_TRY(ctx, hipMalloc(&b.p, (bytes ? bytes : 16) + kGuardBytes));
      b.bytes = bytes;
      b.guarded = true;
      ++b.allocs;
    }
    b.logical = logical;
    HIP_TRY(ctx, guard_arm(b.p, b.logical));
    *out = b.p;
    return CMX_OK;
  }
  if (b.bytes < bytes) {
    if (b.p) HIP_TRY(ctx, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    HIP_TRY(ctx, hipMalloc(&b.p, bytes ? bytes : 16));
    b.bytes = bytes;
    b.guarded = false;
    ++b.allocs;
  }
  *out = b.p;
  return CMX_OK;
}

TmpDev::~TmpDev() {
  if (!sizes.empty()) {
    (void)hipDeviceSynchronize();
    for (size_t i = 0; i < ptrs.size(); ++i) {
      size_t off = 0;
      if (!guard_intact(ptrs[i], sizes[i], &off))
        guard_record("temporary #" + std::to_string(i) + " of a host-pointer entry point was written past its end (" +
                     std::to_string(sizes[i]) + " bytes asked for, first bad byte at +" + std::to_string(off) + ")");
    }
  }
  for (void* p : ptrs) (void)hipFree(p);
}

hipError_t TmpDev::alloc_bytes(void** p, size_t bytes) {
  if (!bytes) bytes = 16;
  const bool g = guard_on();
  hipError_t e = hipMalloc(p, bytes + (g ? kGuardBytes : 0));
  if (e != hipSuccess) return e;
  ptrs.push_back(*p);
  if (g) {
    sizes.push_back(bytes);
    e = guard_arm(*p, bytes);
  }
  return e;
}

cmx_status TmpDev::upload_branch_major(cmx_ctx* ctx, double** p, const double* sm, size_t n, size_t BK) {
  std::vector<double> bm(BK * n);
  for (size_t i = 0; i < n; ++i)
    for (size_t r = 0; r < BK; ++r) bm[r * n + i] = sm[i * BK + r];
  return upload(ctx, p, bm.data(), bm.size());
}

// verify every guarded buffer of a context (device idle); the first trampled one is named in ctx->err
static cmx_status guard_verify_all(cmx_ctx* ctx) {
  if (!guard_on()) return CMX_OK;
  cmx_status rc = CMX_OK;
  auto bad = [&](const std::string& name, size_t logical, size_t off) {
    const std::string msg = "buffer '" + name + "' was written past its end (" + std::to_string(logical) + " bytes asked for, first bad byte at +" + std::to_string(off) + ")";
    guard_record(msg);
    if (rc == CMX_OK) { ctx->err = "CMX_SCRATCH_GUARD: " + msg; rc = CMX_ERR_INTERNAL; }
  };
  size_t off = 0;
  for (auto& kv : ctx->scratch)
    if (kv.second.p && kv.second.guarded && !guard_intact(kv.second.p, kv.second.logical, &off)) {
      bad("scratch:" + kv.first, kv.second.logical, off);
      (void)guard_arm(kv.second.p, kv.second.logical);   // report an overflow once, not at every later check
    }
  for (auto& f : ctx->guarded_fixed)
    if (!guard_intact(f.p, f.bytes, &off)) {
      bad(f.name, f.bytes, off);
      (void)guard_arm(f.p, f.bytes);
    }
  return rc;
}


const char* cmx_version(void) { return "comap_mi355x 0.1 (gfx950)"; }

const char* cmx_last_error(const cmx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

cmx_status cmx_ctx_create(const cmx_model* model, const cmx_tree* tree, int device, cmx_ctx** out) {
  if (!out) return CMX_ERR_INVALID;
  *out = nullptr;
  cmx_ctx* ctx = new cmx_ctx();
  ctx->device = device;
  if (const char* e = getenv("CMX_NULL_PATTERNS")) ctx->null_patterns = e[0] == '0' ? 0 : (e[0] == '1' ? 1 : -1);   // A/B runs
  auto bail = [&](cmx_status s) {
    g_create_error = ctx->err;
    cmx_ctx_destroy(ctx);
    return s;
  };
  if ((model == nullptr) != (tree == nullptr)) {
    ctx->err = "model and tree must be given together (both NULL creates a context for cmx_mi_columns only)";
    return bail(CMX_ERR_INVALID);
  }
  if (model) {
    int code = CMX_OK;
    ctx->hm.lds_slot = g_lds_slot.load() != 0;
    ctx->hm.cherry_msg = g_cherry_msg.load() != 0;
    std::string msg = build_host_model(model, tree, &ctx->hm, &code);
    if (!msg.empty()) {
      ctx->err = msg;
      return bail((cmx_status)code);
    }
    ctx->has_model = true;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    ctx->err = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
               "); this engine has no CPU path";
    return bail(CMX_ERR_DEVICE);
  }
  if (device < 0 || device >= ndev) {
    ctx->err = "device index out of range";
    return bail(CMX_ERR_INVALID);
  }
  auto dev_init = [&]() -> cmx_status {
    HIP_TRY(ctx, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(ctx, CMX_ERR_UNSUPPORTED, std::string("built for gfx950 only, device is ") + prop.gcnArchName);
    ctx->cu_count = prop.multiProcessorCount;
    std::vector<uint32_t> dm(256);
    for (int i = 0; i < 256; ++i) dm[i] = i < 32 ? (1u << i) : 0xffffffffu;
    const uint32_t* p = nullptr;
    CMX_TRY(upload(ctx, dm, &p));
    ctx->d_default_masks = const_cast<uint32_t*>(p);
    if (!ctx->has_model) return CMX_OK;
    const HostModel& h = ctx->hm;
    DevModel& d = ctx->dm;
    d.S = h.dS; d.C = h.dC; d.S0 = h.S; d.C0 = h.C; d.fuse = h.fuse; d.K = h.K; d.nn = h.nn; d.B = h.B; d.T = h.T; d.NI = h.NI; d.NIW = h.NIW; d.NV = h.NV; d.root = h.root;
#define UP(field) CMX_TRY(upload(ctx, h.field, &d.field))
    UP(taxon_of); UP(parent);
    if (!h.plain) {
      // (alphabets other than 4 / 20 states get none of this: their sites are mapped by the plain kernels of cmx_variants.hip
      // on scratch buffers -- map_plain -- with no operator stream and no per-wave workspaces)
      const double* mat = nullptr;
      CMX_TRY(upload(ctx, h.MAT, &mat));
      d.MAT = const_cast<double*>(mat);
      d.MC = h.MC;
      // device copy of an operator stream: operator indices premultiplied to element offsets, and the first two entries
      // repeated after the last one so that "the entry two ops ahead" never needs a wrap test
      auto up_stream = [&](const std::vector<int>& stream, const int** dev, int* nmv) -> cmx_status {
        std::vector<int> ms(stream);
        const int unit = mat_unit(h.dS);
        for (size_t i = 0; i < ms.size(); i += 2) ms[i] *= unit;
        const size_t n2 = ms.size();
        for (size_t i = 0; i < 4; ++i) ms.push_back(ms[i % n2]);
        *nmv = (int)(stream.size() / 2);
        return upload(ctx, ms, dev);
      };
      CMX_TRY(up_stream(h.msched, &d.msched, &d.nmv));
      d.msched_r = nullptr;
      d.nmv_r = 0;
      if (!h.msched_r.empty()) CMX_TRY(up_stream(h.msched_r, &d.msched_r, &d.nmv_r));   // the cherry-table walk's stream
      d.plan = nullptr;
      if (!h.wait_imm.empty()) CMX_TRY(upload(ctx, planned_stream(h), &d.plan));   // the 64-site protein walk reads this one
      if (h.n_cherry_msg > 0) {
        // the resolved walk of the null with the cherry message table (cmx_layout.h): its stream, its planned copy, and the
        // table behind its node index; cherry_msg_kernel fills the rows below, after the leaf operators are complete
        CMX_TRY(up_stream(h.msched_m, &d.msched_r, &d.nmv_r));
        CMX_TRY(upload(ctx, planned_stream(h, true), &ctx->d_plan_r));
        const size_t head = cherry_msg_header_bytes(h.nn), bytes = head + h.cherry_msg_bytes();
        void* p = nullptr;
        HIP_TRY(ctx, hipMalloc(&p, bytes));
        ctx->model_allocs.push_back(p);
        ctx->d_cherry_msg = static_cast<uint8_t*>(p);
        std::vector<int> ref(head / sizeof(int), -1);
        for (int n = 0; n < h.nn; ++n) ref[n] = h.taxon_of[n] >= 0 ? h.taxon_of[n] : h.cherry_of[n];
        HIP_TRY(ctx, hipMemcpy(p, ref.data(), head, hipMemcpyHostToDevice));
      }
      UP(nrec);
    }
    UP(simg); UP(simord);
    d.nsimg = (int)(h.simg.size() / 16);
    UP(eigV); UP(eigVi); UP(eigLam); UP(model_of); UP(blen);
    ctx->d_simtab = nullptr;
    if (!h.simtab.empty()) CMX_TRY(upload(ctx, h.simtab, &ctx->d_simtab));
    UP(CP); UP(CPG); UP(pi); UP(rates); UP(probs); UP(cum_pi); UP(cum_probs);
#undef UP
    if (h.plain) return CMX_OK;   // simulator tables and tree only
    // ambiguity rows of the leaf operators: default "every state compatible" until a call brings a mask table
    HIP_TRY(ctx, launch_extend_leaf_rows(d, nullptr, nullptr));
    if (ctx->d_cherry_msg) {
      const ClassBlock blk = h.block();
      std::vector<int> ops((size_t)h.n_cherry_msg * 4, 0);
      for (int n = 0; n < h.nn; ++n) {
        const int ci = h.cherry_of[n];
        if (ci < 0) continue;
        const std::vector<int> ch = children(h, n);   // an inlined cherry: two leaves, in the records' order
        ops[4 * (size_t)ci] = blk.leaf(h.taxon_of[ch[0]], OPER_P);
        ops[4 * (size_t)ci + 1] = blk.leaf(h.taxon_of[ch[1]], OPER_P);
        ops[4 * (size_t)ci + 2] = blk.internal(h.slot[n], OPER_P);
      }
      const int* d_ops = nullptr;
      CMX_TRY(upload(ctx, ops, &d_ops));
      HIP_TRY(ctx, launch_cherry_msg(d, d_ops, h.n_cherry_msg, ctx->d_cherry_msg + cherry_msg_header_bytes(h.nn), nullptr));
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    ctx->leaf_rows_custom = false;
    // ambiguity masks default: code c >= S compatible with every state; fix the table for this S
    for (int i = 0; i < 256; ++i) dm[i] = i < h.S ? (1u << i) : ((h.S >= 32) ? 0xffffffffu : ((1u << h.S) - 1u));
    HIP_TRY(ctx, hipMemcpy(ctx->d_default_masks, dm.data(), sizeof(uint32_t) * 256, hipMemcpyHostToDevice));
    // per-wave workspaces: 1 wave per SIMD on every CU for the null; a quarter of that for observed alignments
    ctx->grid_blocks = ctx->cu_count * map_waves_per_simd(h.dS);   // 4-wave workgroups, that many per CU
    ctx->waves = ctx->grid_blocks * kWavesPerBlock;
    ctx->obs_blocks = std::max(1, ctx->grid_blocks / 4);
    if (const int cap = g_map_grid.load()) {
      ctx->grid_blocks = std::min(ctx->grid_blocks, cap);
      ctx->waves = ctx->grid_blocks * kWavesPerBlock;
      ctx->obs_blocks = std::min(ctx->obs_blocks, cap);
    }
    auto alloc_ws = [&](Workspace* ws, size_t w, size_t* bytes) -> cmx_status {
      const size_t ks = (size_t)map_sites_per_wave(h.dS);   // sites per mapping wave
      const size_t bD = w * h.NIW * h.dS * ks * sizeof(double);
      const size_t bC = w * 2 * h.B * h.K * ks * sizeof(double);
      const size_t bP = w * h.dC * h.B * h.K * ks * sizeof(double);
      const bool g = guard_on();
      auto one = [&](const char* nm, void** p, size_t bytes) -> cmx_status {
        HIP_TRY(ctx, hipMalloc(p, bytes + (g ? kGuardBytes : 0)));
        if (g) {
          HIP_TRY(ctx, guard_arm(*p, bytes));
          ctx->guarded_fixed.push_back({std::string(ws == &ctx->ws ? "workspace:" : "workspace_obs:") + nm, *p, bytes});
        }
        return CMX_OK;
      };
      CMX_TRY(one("D", (void**)&ws->D, bD));
      CMX_TRY(one("U", (void**)&ws->U, bD));
      CMX_TRY(one("cnt", (void**)&ws->cnt, bC));
      CMX_TRY(one("part", (void**)&ws->part, bP));
      ws->waves = (int)w;
      *bytes += 2 * bD + bC + bP;
      return CMX_OK;
    };
    ctx->ws_bytes = 0;
    CMX_TRY(alloc_ws(&ctx->ws, (size_t)ctx->waves, &ctx->ws_bytes));
    CMX_TRY(alloc_ws(&ctx->ws_obs, (size_t)ctx->obs_blocks * kWavesPerBlock, &ctx->ws_bytes));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->map_queue, sizeof(unsigned long long) * kMapQueueRing));   // map_queue_take
    return CMX_OK;
  };
  cmx_status s = dev_init();
  if (s != CMX_OK) return bail(s);
  *out = ctx;
  return CMX_OK;
}

void cmx_ctx_destroy(cmx_ctx* ctx) {
  if (!ctx) return;
  if (guard_on() && hipSetDevice(ctx->device) == hipSuccess && hipDeviceSynchronize() == hipSuccess)
    (void)guard_verify_all(ctx);   // destroy cannot fail: findings go to stderr and to cmx_debug_scratch_guard_failures
  for (void* p : ctx->model_allocs) (void)hipFree(p);
  if (ctx->d_stat_w) (void)hipFree(ctx->d_stat_w);
  if (ctx->map_queue) (void)hipFree(ctx->map_queue);
  for (auto& kv : ctx->scratch) if (kv.second.p) (void)hipFree(kv.second.p);
  for (Workspace* ws : {&ctx->ws, &ctx->ws_obs}) {
    if (ws->D) (void)hipFree(ws->D);
    if (ws->U) (void)hipFree(ws->U);
    if (ws->cnt) (void)hipFree(ws->cnt);
    if (ws->part) (void)hipFree(ws->part);
  }
  delete ctx;
}

cmx_status map_queue_take(cmx_ctx* ctx, size_t nblocks, int grid, hipStream_t stream, unsigned long long** queue) {
  *queue = nullptr;
  const size_t nwaves = (size_t)grid * kWavesPerBlock;
  if (nblocks <= nwaves || g_map_queue.load() == 0) return CMX_OK;
  // A word is reused kMapQueueRing queued launches later: the ring assumes fewer than kMapQueueRing queued mapping launches
  // of one context in flight at a time, over all streams (a launch is done with its word when its kernel ends).  Two
  // launches in flight on two streams -- the observed mapping beside the null -- therefore never share a counter.
  unsigned long long* q = ctx->map_queue + ctx->map_queue_turn++ % kMapQueueRing;
  HIP_TRY(ctx, launch_map_queue_init(q, (unsigned long long)nwaves, stream));
  *queue = q;
  return CMX_OK;
}

cmx_status cmx_get_info(const cmx_ctx* ctx, cmx_info* info) {
  if (!ctx || !info) return CMX_ERR_INVALID;
  std::memset(info, 0, sizeof(*info));
  info->nstates = ctx->hm.S; info->nclasses = ctx->hm.C; info->ntypes = ctx->hm.K; info->nnodes = ctx->hm.nn;
  info->nbranches = ctx->hm.B; info->ntaxa = ctx->hm.T; info->ninternal = ctx->hm.NI;
  info->device = ctx->device; info->cu_count = ctx->cu_count; info->waves = ctx->waves;
  info->workspace_bytes = ctx->ws_bytes;
  info->device_states = ctx->hm.dS; info->device_classes = ctx->hm.dC;
  info->products_per_pass = (int32_t)ctx->hm.n_products; info->leaf_ops_per_pass = (int32_t)ctx->hm.n_leaf_ops;
  info->ws_loads_per_pass = (int32_t)ctx->hm.n_loads; info->ws_stores_per_pass = (int32_t)ctx->hm.n_stores;
  info->products_per_pass_null = (int32_t)ctx->hm.n_products_r; info->leaf_ops_per_pass_null = (int32_t)ctx->hm.n_leaf_ops_r;
  info->cherry_tables = ctx->hm.msched_r.empty() ? 0 : ctx->hm.ncherry;
  return CMX_OK;
}

cmx_status cmx_get_transition_matrices(const cmx_ctx* ctx, double* P) {
  if (!ctx || !P || !ctx->has_model) return CMX_ERR_INVALID;
  std::memcpy(P, ctx->hm.P.data(), sizeof(double) * ctx->hm.P.size());
  return CMX_OK;
}

cmx_status cmx_debug_walk(const cmx_model* model, const cmx_tree* tree, int32_t* nrec, size_t nrec_cap, size_t* nrec_n,
                          int32_t* ldsched, size_t ld_cap, size_t* ld_n, int32_t* msched, size_t m_cap, size_t* m_n,
                          int32_t* slot_of_node, uint64_t* stats /*[8]: loads, stores, products, leaf ops per pass; products, leaf ops of the cherry-table walk, cherries with tables; LDS-slot transfers*/) {
  HostModel hm;
  int code = CMX_OK;
  hm.lds_slot = g_lds_slot.load() != 0;
  hm.cherry_msg = g_cherry_msg.load() != 0;
  const std::string msg = build_host_model(model, tree, &hm, &code);
  if (!msg.empty()) {
    g_create_error = msg;
    return (cmx_status)code;
  }
  if (hm.nrec.size() > nrec_cap || hm.ldsched.size() > ld_cap || hm.msched.size() > m_cap) {
    g_create_error = "cmx_debug_walk: buffers too small";
    return CMX_ERR_INVALID;
  }
  std::memcpy(nrec, hm.nrec.data(), hm.nrec.size() * sizeof(int32_t));
  std::memcpy(ldsched, hm.ldsched.data(), hm.ldsched.size() * sizeof(int32_t));
  std::memcpy(msched, hm.msched.data(), hm.msched.size() * sizeof(int32_t));
  *nrec_n = hm.nrec.size(); *ld_n = hm.ldsched.size(); *m_n = hm.msched.size();
  if (slot_of_node) std::memcpy(slot_of_node, hm.slot.data(), hm.slot.size() * sizeof(int32_t));
  if (stats) {
    stats[0] = hm.n_loads; stats[1] = hm.n_stores; stats[2] = hm.n_products; stats[3] = hm.n_leaf_ops;
    stats[4] = hm.n_products_r; stats[5] = hm.n_leaf_ops_r; stats[6] = hm.msched_r.empty() ? 0 : (uint64_t)hm.ncherry;
    stats[7] = (uint64_t)hm.n_lds_loads | ((uint64_t)hm.n_lds_stores << 20) | ((uint64_t)hm.n_lds_copies << 40);
  }
  return CMX_OK;
}

cmx_status cmx_debug_wait_plan(const cmx_model* model, const cmx_tree* tree, int32_t* distance, int32_t* immediate, size_t cap, size_t* n) {
  HostModel hm;
  int code = CMX_OK;
  hm.lds_slot = g_lds_slot.load() != 0;
  hm.cherry_msg = g_cherry_msg.load() != 0;
  const std::string msg = build_host_model(model, tree, &hm, &code);
  if (!msg.empty()) {
    g_create_error = msg;
    return (cmx_status)code;
  }
  if (hm.wait_imm.size() > cap) {
    g_create_error = "cmx_debug_wait_plan: buffers too small";
    return CMX_ERR_INVALID;
  }
  std::memcpy(distance, hm.wait_dist.data(), hm.wait_dist.size() * sizeof(int32_t));
  std::memcpy(immediate, hm.wait_imm.data(), hm.wait_imm.size() * sizeof(int32_t));
  *n = hm.wait_imm.size();
  return CMX_OK;
}

int cmx_debug_wait_skew(int entry) { return wait_plan_skew(entry); }

// what cmx_get_cherry_msg_info and cmx_debug_cherry_msg_walk report (include/comap_mi355x.h)
static void cherry_msg_stats(const HostModel& hm, uint64_t* stats) {
  const bool on = hm.n_cherry_msg > 0;
  stats[0] = (uint64_t)hm.n_cherry_msg; stats[1] = on ? (uint64_t)hm.cherry_msg_bytes() : 0;
  stats[2] = on ? hm.msg.products : hm.n_products; stats[3] = on ? hm.msg.leaf_ops : hm.n_leaf_ops; stats[4] = hm.msg.gathers;
  stats[5] = on ? hm.msg.loads : hm.n_loads; stats[6] = on ? hm.msg.stores : hm.n_stores;
  stats[7] = on ? hm.msg.lds_loads : hm.n_lds_loads; stats[8] = on ? hm.msg.lds_stores : hm.n_lds_stores; stats[9] = on ? hm.msg.lds_copies : hm.n_lds_copies;
  stats[10] = (uint64_t)kCherryMsgMaxBytes; stats[11] = 0;
}

cmx_status cmx_get_cherry_msg_info(const cmx_ctx* ctx, uint64_t* stats) {
  if (!ctx || !stats || !ctx->has_model) return CMX_ERR_INVALID;
  cherry_msg_stats(ctx->hm, stats);
  return CMX_OK;
}

cmx_status cmx_debug_cherry_msg_walk(const cmx_model* model, const cmx_tree* tree, uint64_t* stats, int32_t* msched, size_t m_cap, size_t* m_n,
                                     int32_t* distance, int32_t* immediate) {
  HostModel hm;
  int code = CMX_OK;
  hm.lds_slot = g_lds_slot.load() != 0;
  hm.cherry_msg = g_cherry_msg.load() != 0;
  const std::string msg = build_host_model(model, tree, &hm, &code);
  if (!msg.empty()) {
    g_create_error = msg;
    return (cmx_status)code;
  }
  if (!stats || !m_n || hm.msched_m.size() > m_cap) {
    g_create_error = "cmx_debug_cherry_msg_walk: a buffer is missing or too small";
    return CMX_ERR_INVALID;
  }
  cherry_msg_stats(hm, stats);
  *m_n = hm.msched_m.size();
  if (msched) std::memcpy(msched, hm.msched_m.data(), hm.msched_m.size() * sizeof(int32_t));
  if (distance) std::memcpy(distance, hm.wait_dist_m.data(), hm.wait_dist_m.size() * sizeof(int32_t));
  if (immediate) std::memcpy(immediate, hm.wait_imm_m.data(), hm.wait_imm_m.size() * sizeof(int32_t));
  return CMX_OK;
}

cmx_status cmx_debug_cherry_msg_table(cmx_ctx* ctx, double* table, size_t cap, int32_t* cherries) {
  CMX_TRY(need_model(ctx));
  const HostModel& h = ctx->hm;
  const size_t need = (size_t)h.C * h.n_cherry_msg * kCherryMsgPairs * 20;
  if (!ctx->d_cherry_msg || !table || cap < need) return fail(ctx, CMX_ERR_INVALID, "cmx_debug_cherry_msg_table: no table, or the buffer is missing or too small");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  std::vector<double> raw(h.cherry_msg_bytes() / sizeof(double));
  HIP_TRY(ctx, hipMemcpy(raw.data(), ctx->d_cherry_msg + cherry_msg_header_bytes(h.nn), h.cherry_msg_bytes(), hipMemcpyDeviceToHost));
  const size_t tab = kCherryMsgTableBytes / sizeof(double);
  for (int c = 0; c < h.C; ++c)
    for (int ci = 0; ci < h.n_cherry_msg; ++ci)
      for (int p = 0; p < kCherryMsgPairs; ++p)
        for (int x = 0; x < 20; ++x)
          table[(((size_t)c * h.n_cherry_msg + ci) * kCherryMsgPairs + p) * 20 + x] = raw[((size_t)ci * h.C + c) * tab + cherry_msg_offset(p, x)];
  if (cherries)
    for (int n = 0; n < h.nn; ++n)
      if (h.cherry_of[n] >= 0) {
        const std::vector<int> ch = children(h, n);
        int32_t* o = cherries + 3 * (size_t)h.cherry_of[n];
        o[0] = n; o[1] = ch[0]; o[2] = ch[1];
      }
  return CMX_OK;
}

cmx_status cmx_debug_sim_tables(const cmx_model* model, const cmx_tree* tree, double* cum, size_t cum_cap, uint8_t* guide,
                                size_t guide_cap, uint8_t* blocks, size_t blocks_cap, size_t* blocks_bytes, int32_t* row) {
  HostModel hm;
  int code = CMX_OK;
  const std::string msg = build_host_model(model, tree, &hm, &code);
  if (!msg.empty()) {
    g_create_error = msg;
    return (cmx_status)code;
  }
  const size_t ncum = (size_t)hm.C * hm.nn * hm.S * hm.S, nguide = (size_t)hm.C * hm.nn * hm.S * 32;   // (CP's padding is not part of it)
  if (blocks_bytes) *blocks_bytes = hm.simtab.size();
  if (row) *row = sim_thr_row(hm.S);
  if (!cum && !guide && !blocks) return CMX_OK;   // the sizes only
  if (!cum || !guide || !blocks || cum_cap < ncum || guide_cap < nguide || blocks_cap < hm.simtab.size()) {
    g_create_error = "cmx_debug_sim_tables: a buffer is missing or too small";
    return CMX_ERR_INVALID;
  }
  std::memcpy(cum, hm.CP.data(), ncum * sizeof(double));
  std::memcpy(guide, hm.CPG.data(), nguide);
  if (!hm.simtab.empty()) std::memcpy(blocks, hm.simtab.data(), hm.simtab.size());
  return CMX_OK;
}

cmx_status cmx_synchronize(cmx_ctx* ctx) {
  if (!ctx) return CMX_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  return guard_verify_all(ctx);
}

cmx_status cmx_scratch_check(cmx_ctx* ctx) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!guard_on()) return fail(ctx, CMX_ERR_UNSUPPORTED, "the scratch guard is off (CMX_SCRATCH_GUARD=1 or cmx_debug_scratch_guard(1) before the context is created)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  return guard_verify_all(ctx);
}

int cmx_debug_scratch_guard(int on) {
  const int was = guard_on() ? 1 : 0;
  if (on >= 0) g_guard.store(on ? 1 : 0);
  return was;
}

int cmx_debug_lds_slot(int on) {
  const int was = g_lds_slot.load();
  if (on >= 0) g_lds_slot.store(on ? 1 : 0);
  return was;
}

int cmx_debug_cherry_msg(int on) {
  const int was = g_cherry_msg.load();
  if (on >= 0) g_cherry_msg.store(on ? 1 : 0);
  return was;
}

int cmx_debug_map_queue(int on) {
  const int was = g_map_queue.load();
  if (on >= 0) g_map_queue.store(on ? 1 : 0);
  return was;
}

void cmx_debug_sim_sites(long long min_sites, long long four_batch_sites) {
  if (min_sites >= -1) g_sim_min_sites.store(min_sites);
  if (four_batch_sites >= -1) g_sim_four_batch_sites.store(four_batch_sites);
}

int cmx_debug_map_small_blocks(int on) {
  const int was = g_map_small_blocks.load();
  if (on >= 0) g_map_small_blocks.store(on ? 1 : 0);
  return was;
}

int cmx_debug_map_grid(int workgroups) {
  const int was = g_map_grid.load();
  if (workgroups >= 0) g_map_grid.store(workgroups);
  return was;
}

size_t cmx_debug_scratch_guard_failures(char* buf, size_t cap, int clear) {
  std::lock_guard<std::mutex> lk(g_guard_mu);
  const size_t n = g_guard_failures.size();
  if (buf && cap) {
    std::string all;
    for (const std::string& f : g_guard_failures) { all += f; all += '\n'; }
    std::snprintf(buf, cap, "%s", all.c_str());
  }
  if (clear) g_guard_failures.clear();
  return n;
}

void cmx_debug_scratch_shrink(const char* name, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_guard_mu);
  if (!name) { g_guard_shrink.clear(); return; }
  if (bytes == 0) g_guard_shrink.erase(name);
  else g_guard_shrink[name] = bytes;
}

cmx_status cmx_set_null_patterns(cmx_ctx* ctx, int on) {
  CMX_TRY(need_model(ctx));
  ctx->null_patterns = on < 0 ? -1 : (on ? 1 : 0);
  return CMX_OK;
}

int cmx_debug_null_hash_bits(int bits) {
  const int was = g_pat_hash_bits.load();
  if (bits > 0) g_pat_hash_bits.store(bits > 64 ? 64 : bits);
  return was;
}

// nijt.average / nijt.joint of CoETools.cpp:393-394 ("really for benchmarking only" there)
cmx_status cmx_set_mapping_options(cmx_ctx* ctx, int average, int joint) {
  CMX_TRY(need_model(ctx));
  ctx->map_average = average != 0;
  ctx->map_joint = joint != 0;
  return CMX_OK;
}

// per-site likelihood scaling: host state only, read by the next mapping, null or ancestral-state call
cmx_status cmx_set_likelihood_scaling(cmx_ctx* ctx, int on) {
  CMX_TRY(need_model(ctx));
  ctx->scaling = on != 0;
  return CMX_OK;
}

cmx_status cmx_get_likelihood_scaling(const cmx_ctx* ctx, int32_t* on) {
  if (!ctx || !on) return CMX_ERR_INVALID;
  *on = ctx->scaling ? 1 : 0;
  return CMX_OK;
}

// Statistic::setWeights / deleteWeights (CoMap/Statistics.h:83-104, 135-140): stored divided by their sum, in the
// reference's summation order.  Validated before any device work; the device copy is written once here, after the
// device has drained (a kernel of an earlier call on any stream may still read the previous weights).
cmx_status cmx_set_statistic_weights(cmx_ctx* ctx, const double* w, size_t nbranches) {
  CMX_TRY(need_model(ctx));
  std::vector<double> wn;
  if (w) {
    if (nbranches != (size_t)ctx->hm.B)
      return fail(ctx, CMX_ERR_INVALID, "cmx_set_statistic_weights: " + std::to_string(nbranches) + " weights for " +
                                            std::to_string(ctx->hm.B) + " branches (DimensionException)");
    double sum = 0.0;
    for (size_t b = 0; b < nbranches; ++b) {
      if (!std::isfinite(w[b]))
        return fail(ctx, CMX_ERR_INVALID, "cmx_set_statistic_weights: weight " + std::to_string(b) + " is not finite");
      if (w[b] < 0.0)
        return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_set_statistic_weights: weight " + std::to_string(b) + " is negative");
      sum += w[b];
    }
    if (!(sum > 0.0) || !std::isfinite(sum))
      return fail(ctx, CMX_ERR_INVALID, "cmx_set_statistic_weights: the weights must have a positive, finite sum");
    wn.resize(nbranches);
    for (size_t b = 0; b < nbranches; ++b) wn[b] = w[b] / sum;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_stat_w) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_stat_w, sizeof(double) * ctx->hm.B));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(ctx->d_stat_w, wn.data(), sizeof(double) * nbranches, hipMemcpyHostToDevice));
  }
  ctx->stat_w.swap(wn);
  ctx->gram_kept.valid = false;   // kept Gram blocks were scored with the previous weights
  return CMX_OK;
}

cmx_status cmx_get_statistic_weights(const cmx_ctx* ctx, double* w_out, int32_t* has_weights) {
  if (!ctx || !has_weights) return CMX_ERR_INVALID;
  *has_weights = ctx->stat_w.empty() ? 0 : 1;
  if (w_out) std::copy(ctx->stat_w.begin(), ctx->stat_w.end(), w_out);
  return CMX_OK;
}
