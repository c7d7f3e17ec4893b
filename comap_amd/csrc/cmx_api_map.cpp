// C-ABI, mapping stage: substitution mapping of observed alignments and its variants, ancestral states, the simulators.
#include "cmx_ctx.h"

// What a mapping reads ([T][ld] codes; masks null: every code >= nstates is an unknown) and writes (counts [B*K][ldc], the rest
// per site, each optional), as map_sites_impl is given it: the walk's MapArgs and the plain stage's PlainArgs are filled from these.
struct MapIn { const uint8_t* aln; size_t nsites, ld; const uint32_t* masks; };
struct MapOut { double* counts; size_t ldc; double *norm, *logL, *post_rate; int32_t* rate_class; };
// pass budgets of the plain stage's per-node vectors (plain_sites_per_pass): the mapping fills its passes, ancestral states balance theirs
constexpr size_t kPlainMapScratchBytes = (size_t)1 << 30, kAsrScratchBytes = (size_t)2 << 30;

// S x S matrices padded with zeros to SP x SP (the plain path's kernels run at kPlainStates states)
static std::vector<double> pad_mats(const std::vector<double>& m, int S, int SP) {
  if (S == SP) return m;
  const size_t nm = m.size() / ((size_t)S * S);
  std::vector<double> o(nm * (size_t)SP * SP, 0.0);
  for (size_t q = 0; q < nm; ++q)
    for (int x = 0; x < S; ++x)
      for (int y = 0; y < S; ++y) o[(q * SP + x) * SP + y] = m[(q * S + x) * S + y];
  return o;
}

// 64 x 64 row-major matrices packed for the wide mapping (wide_op_offset, cmx_layout.h), or their transposes
static std::vector<double> pack_wide(const std::vector<double>& m, bool transpose) {
  constexpr int SP = kPlainStates;
  std::vector<double> o(m.size());
  for (size_t q = 0; q < m.size() / ((size_t)SP * SP); ++q)
    for (int x = 0; x < SP; ++x)
      for (int y = 0; y < SP; ++y)
        o[q * SP * SP + (transpose ? wide_op_offset(y, x) : wide_op_offset(x, y))] = m[(q * SP + x) * SP + y];
  return o;
}

// 20 x 20 row-major matrices packed for the 20-state shape of the wide mapping (wide20_op_offset: 32 x 20, rows 20 .. 31 zero)
static std::vector<double> pack_wide20(const std::vector<double>& m, bool transpose) {
  constexpr int S = 20, U = kWide20Rows * S;
  const size_t nm = m.size() / ((size_t)S * S);
  std::vector<double> o(nm * U, 0.0);
  for (size_t q = 0; q < nm; ++q)
    for (int x = 0; x < S; ++x)
      for (int y = 0; y < S; ++y) o[q * U + (transpose ? wide20_op_offset(y, x) : wide20_op_offset(x, y))] = m[(q * S + x) * S + y];
  return o;
}

// the operators of the plain kernels (cmx_variants.hip), uploaded at the first use by the mapping variants or by the
// ancestral states (padded with zeros to kPlainStates on the plain path)
static cmx_status upload_variant_operators(cmx_ctx* ctx) {
  const HostModel& h = ctx->hm;
  const int SD = h.plain ? kPlainStates : h.S;
  if (!ctx->va_P) {
    CMX_TRY(upload(ctx, pad_mats(h.P, h.S, SD), &ctx->va_P));
    CMX_TRY(upload(ctx, pad_mats(h.N1, h.S, SD), &ctx->va_N1));
    CMX_TRY(upload(ctx, pad_mats(h.NC, h.S, SD), &ctx->va_NC));
    CMX_TRY(upload(ctx, h.first_child, &ctx->va_first));
    CMX_TRY(upload(ctx, h.next_sib, &ctx->va_next));
    if (h.plain) {
      std::vector<double> pi(SD, 0.0);
      std::copy(h.pi.begin(), h.pi.end(), pi.begin());
      const std::vector<double> P = pad_mats(h.P, h.S, SD), PN = pad_mats(h.PN, h.S, SD);
      CMX_TRY(upload(ctx, PN, &ctx->va_PN));
      CMX_TRY(upload(ctx, pi, &ctx->va_pi));
      CMX_TRY(upload(ctx, pack_wide(P, false), &ctx->va_wide.P));
      CMX_TRY(upload(ctx, pack_wide(P, true), &ctx->va_wide.PT));
      CMX_TRY(upload(ctx, pack_wide(PN, false), &ctx->va_wide.PN));
    }
  }
  // the scaled default mapping at 4 / 20 states reads the joint counts too: at its first use, whatever was uploaded before
  if (ctx->scaling && !ctx->va_PN) CMX_TRY(upload(ctx, h.PN, &ctx->va_PN));
  // and at 20 states the three operators of its matrix-core kernels (cmx_map_wide.hip), packed
  if (ctx->scaling && h.S == 20 && !ctx->va_wide.P) {
    CMX_TRY(upload(ctx, pack_wide20(h.P, false), &ctx->va_wide.P));
    CMX_TRY(upload(ctx, pack_wide20(h.P, true), &ctx->va_wide.PT));
    CMX_TRY(upload(ctx, pack_wide20(h.PN, false), &ctx->va_wide.PN));
  }
  return CMX_OK;
}

// the model and alignment fields of the plain kernels' arguments (operators uploaded); the caller sets the mode, the
// outputs and the sites per pass
static PlainArgs plain_args(cmx_ctx* ctx, const MapIn& in) {
  const HostModel& h = ctx->hm;
  PlainArgs a{};
  a.S = h.plain ? kPlainStates : h.S; a.Sreal = h.S; a.C = h.C; a.K = h.K; a.nn = h.nn; a.B = h.B; a.root = h.root;
  a.first_child = ctx->va_first; a.next_sib = ctx->va_next; a.taxon_of = ctx->dm.taxon_of; a.parent = ctx->dm.parent;
  a.P = ctx->va_P; a.N1 = ctx->va_N1; a.NC = ctx->va_NC; a.PN = ctx->va_PN; a.pi = h.plain ? ctx->va_pi : ctx->dm.pi; a.probs = ctx->dm.probs;
  a.rates = ctx->dm.rates;
  a.masks = in.masks; a.aln = in.aln; a.ld = in.ld;
  return a;
}

// Does a mapping go through the plain stage (cmx_variants.hip)?  Other alphabets than 4 / 20 states: for any output.
// 4 / 20 states: for the counts or the norms under a non-default option (cmx_set_mapping_options); the scalars stay the walk's.
// With likelihood scaling (cmx_set_likelihood_scaling) the walk is not used: every alphabet, any output.
static bool plain_stage_wanted(const cmx_ctx* ctx, const MapOut& out) {
  const bool counts = out.counts || out.norm;
  if (ctx->hm.plain || ctx->scaling) return counts || out.logL || out.post_rate || out.rate_class;
  return counts && !(ctx->map_average && ctx->map_joint);
}

// The plain stage of a mapping.  full_grid names the caller as in map_sites_impl: the engine's own null / clustering /
// candidate pipelines (true) and the public observed-alignment mapping (false) may run on two streams at once, so each has
// its own scratch -- the averaged path keeps ws and ws_obs apart for the same reason.
static cmx_status map_plain(cmx_ctx* ctx, const MapIn& in, MapOut out, void* stream, bool full_grid) {
  const HostModel& h = ctx->hm;
  CMX_TRY(upload_variant_operators(ctx));
  if (!out.counts && out.norm) {   // only the norms were asked for: they still need the counts
    CMX_TRY(scratch(ctx, full_grid ? "va_counts_null" : "va_counts_obs", (size_t)h.B * h.K * in.nsites, &out.counts));
    out.ldc = in.nsites;
  }
  PlainArgs a = plain_args(ctx, in);
  using M = PlainMode;
  a.mode = ctx->map_joint ? (ctx->map_average ? M::Joint : M::NoAvg) : (ctx->map_average ? M::Marginal : M::NoAvgMarginal);
  if (h.plain || ctx->scaling) { a.logL = out.logL; a.post_rate = out.post_rate; a.rate_class = out.rate_class; }   // else (4 / 20 states) the walk wrote them
  a.chunk = plain_sites_per_pass(a.S, h.C, h.nn, in.nsites, kPlainMapScratchBytes, false);
  a.counts = out.counts; a.ldc = out.ldc;
  double* buf;
  CMX_TRY(scratch(ctx, full_grid ? "va_nodes_null" : "va_nodes_obs", plain_node_doubles(a.S, h.C, h.nn, a.chunk), &buf));
  int32_t* exps = nullptr;   // likelihood scaling: the exponents beside the vectors, per caller like them
  if (ctx->scaling) CMX_TRY(scratch(ctx, full_grid ? "va_exps_null" : "va_exps_obs", plain_exponent_ints(h.C, h.nn, a.chunk), &exps));
  // the default mapping on the matrix-core kernels of cmx_map_wide.hip: the plain path's alphabets without scaling unless
  // cmx_debug_map_wide_plain forces the plain kernels, and with scaling these and 20 states unless
  // cmx_debug_map_scaled_plain does (each read at each call; neither touches the other's calls)
  const bool wide = a.mode == M::Joint && (ctx->scaling ? (h.plain || h.S == 20) && !map_scaled_plain(-1) : h.plain && !map_wide_plain(-1));
  if (wide) {
    void* part;
    const size_t bytes = ctx->scaling ? wide_scaled_part_bytes(h.C, h.B, h.K, a.chunk) : sizeof(double) * wide_part_doubles(h.C, h.B, h.K, a.chunk);
    CMX_TRY(scratch(ctx, full_grid ? "va_part_null" : "va_part_obs", bytes, &part));
    HIP_TRY(ctx, launch_wide_map(a, ctx->va_wide, in.nsites, buf, exps, (double*)part, out.norm, (hipStream_t)stream));
    return CMX_OK;
  }
  HIP_TRY(ctx, launch_plain_map(a, in.nsites, buf, exps, out.norm, (hipStream_t)stream));
  return CMX_OK;
}

int cmx_debug_map_wide_plain(int on) { return map_wide_plain(on); }
int cmx_debug_map_scaled_plain(int on) { return map_scaled_plain(on); }

// ------------------------------------------------------------------------------------------------ mapping
// The matrix-core walk of a 4- or 20-state mapping (cmx_map.hip).  full_grid: use the whole-chip workspace of the null launches
// instead of the quarter-chip slice reserved for observed alignments (which exists so that a caller can overlap the observed
// mapping with cmx_null_intra_dev on a second stream).  Only the engine's own simulate -> map pipelines (inter null, clustering
// null, candidate groups) ask for it: they are blocking calls on the null stream and map hundreds of thousands of simulated sites.
static cmx_status map_walk(cmx_ctx* ctx, const MapIn& in, const MapOut& out, void* stream, bool full_grid) {
  const size_t nsites = in.nsites;
  const int max_blocks = full_grid ? ctx->grid_blocks : ctx->obs_blocks;
  MapArgs a{};
  a.m = ctx->dm; a.ws = full_grid ? ctx->ws : ctx->ws_obs; a.aln = in.aln; a.ld = in.ld; a.nsites = nsites;
  // ambiguity ids S .. S+max_ambig(S)-1: rebuild the extra rows of the leaf operators when the table changes.
  // Not for the engine's own pipelines (full_grid): their simulated alignments are fully resolved and never read those
  // rows, and rebuilding them on the null's stream would race with an observed mapping of ambiguous codes that a caller
  // has in flight on a second stream.  leaf_rows_custom stays as it is, so the next public call without a table still
  // restores the default rows.
  if (!full_grid && (in.masks || ctx->leaf_rows_custom)) {
    HIP_TRY(ctx, launch_extend_leaf_rows(ctx->dm, in.masks, (hipStream_t)stream));
    ctx->leaf_rows_custom = in.masks != nullptr;
  }
  a.counts = out.counts; a.ldc = out.ldc; a.logL = out.logL; a.post_rate = out.post_rate; a.rate_class = out.rate_class; a.norm = out.norm;
  size_t ks = (size_t)map_sites_per_wave(ctx->hm.dS);
  size_t nblocks = (nsites + ks - 1) / ks;
  const size_t obs_waves = (size_t)max_blocks * kWavesPerBlock;
  if (nblocks * (size_t)ctx->hm.dC <= obs_waves && ctx->hm.dC > 1) {
    // small alignment: one (site block, class) per wave, classes summed by a second kernel (same arithmetic order)
    // Proteins, when even that leaves most of the chip idle: 16-site blocks (one site group per wave) -- four times the
    // tasks, a quarter of the matrix work per operator op, and a wave's slices of the workspaces are a quarter as large,
    // so 4 * obs_waves of them fit the same allocation
    // (cmx_debug_map_small_blocks(0) keeps the 64-site blocks: the only road to map_kernel<20, split, 1, NG = 4>, for tests)
    if (ctx->hm.dS == 20 && ctx->hm.fuse == 1 && g_map_small_blocks.load() != 0 && ((nsites + 15) / 16) * (size_t)ctx->hm.dC <= 4 * obs_waves) {
      ks = 16;
      nblocks = (nsites + ks - 1) / ks;
    }
    a.split_sites = (int)ks;
    const size_t ntasks = nblocks * (size_t)ctx->hm.dC, BK = (size_t)ctx->hm.B * ctx->hm.K;
    // (per caller, like the workspaces: the public observed mapping and the engine's own pipelines may overlap on two streams)
    CMX_TRY(scratch(ctx, full_grid ? "split_part_null" : "split_part_obs", ntasks * BK * ks, &a.split_part));
    CMX_TRY(scratch(ctx, full_grid ? "split_lc_null" : "split_lc_obs", 4 * ntasks * ks, &a.split_lc));
    const int grid = (int)((ntasks + kWavesPerBlock - 1) / kWavesPerBlock);
    HIP_TRY(ctx, launch_map(a, kModeObservedSplit, grid, (hipStream_t)stream));
    HIP_TRY(ctx, launch_map_finalize(a, (hipStream_t)stream));
    return CMX_OK;
  }
  const size_t blocks_needed = (nblocks + kWavesPerBlock - 1) / kWavesPerBlock;
  const int grid = (int)std::min<size_t>(blocks_needed, (size_t)max_blocks);
  CMX_TRY(map_queue_take(ctx, nblocks, grid, (hipStream_t)stream, &a.queue));
  HIP_TRY(ctx, launch_map(a, kModeObserved, grid, (hipStream_t)stream));
  return CMX_OK;
}

// a mapping: the walk at 4 / 20 states (unless the context scales its likelihoods), then (or instead) the plain stage where
// it is wanted
cmx_status map_sites_impl(cmx_ctx* ctx, const uint8_t* d_aln, size_t nsites, size_t ld, const uint32_t* d_masks, double* d_counts,
                          size_t ldc, double* d_logL, double* d_post_rate, int32_t* d_rate_class, double* d_norm, void* stream,
                          bool full_grid) {
  CMX_TRY(need_model(ctx));
  if (!d_aln || nsites == 0 || ld < nsites) return fail(ctx, CMX_ERR_INVALID, "cmx_map_sites: bad alignment arguments");
  if (d_counts && ldc < nsites) return fail(ctx, CMX_ERR_INVALID, "cmx_map_sites: ldc < nsites");
  if (d_counts && d_counts == ctx->gram_kept.counts) ctx->gram_kept.valid = false;   // the vectors the kept Gram blocks were made from are rewritten
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->hm.plain && d_masks)   // (codon models)
    return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_map_sites: no ambiguity table for alphabets other than 4 / 20 states (codes >= nstates are unknowns)");
  const MapIn in{d_aln, nsites, ld, d_masks};
  const MapOut out{d_counts, ldc, d_norm, d_logL, d_post_rate, d_rate_class};
  if (!ctx->hm.plain && !ctx->scaling) CMX_TRY(map_walk(ctx, in, out, stream, full_grid));
  return plain_stage_wanted(ctx, out) ? map_plain(ctx, in, out, stream, full_grid) : CMX_OK;
}

cmx_status cmx_map_sites_dev(cmx_ctx* ctx, const uint8_t* d_aln, size_t nsites, size_t ld, const uint32_t* d_masks,
                             double* d_counts, size_t ldc, double* d_logL, double* d_post_rate, int32_t* d_rate_class,
                             double* d_norm, void* stream) {
  return map_sites_impl(ctx, d_aln, nsites, ld, d_masks, d_counts, ldc, d_logL, d_post_rate, d_rate_class, d_norm, stream, false);
}

// the host-pointer entry points' alignment rules (who names the entry point in the message): [T][ld] codes, every code a
// state or one of the nmasks masks; a mask table only for 4 / 20 states, at most max_ambig(S) ambiguity ids
static cmx_status check_host_alignment(cmx_ctx* ctx, const char* who, const uint8_t* aln, size_t nsites, size_t ld,
                                       const uint32_t* masks, size_t nmasks) {
  CMX_TRY(need_model(ctx));
  const std::string w(who);
  if (!aln || nsites == 0 || ld < nsites) return fail(ctx, CMX_ERR_INVALID, w + ": bad alignment arguments");
  const HostModel& h = ctx->hm;
  if (masks && h.plain)
    return fail(ctx, CMX_ERR_UNSUPPORTED, w + ": no ambiguity table for alphabets other than 4 / 20 states (codes >= nstates are unknowns)");
  if (masks && nmasks > (size_t)(h.S + max_ambig(h.S)))
    return fail(ctx, CMX_ERR_UNSUPPORTED, w + ": at most " + std::to_string(max_ambig(h.S)) +
                                              " ambiguity ids (codes >= nstates) are supported for this alphabet");
  // every code must be a state or a known mask (the reference throws BadCharException at alignment parsing)
  for (int t = 0; t < h.T; ++t)
    for (size_t i = 0; i < nsites; ++i) {
      const unsigned c = aln[(size_t)t * ld + i];
      if (c >= (unsigned)h.S && masks && c >= nmasks) return fail(ctx, CMX_ERR_INVALID, w + ": alignment code without a mask");
    }
  return CMX_OK;
}

// the checked alignment as [T][nsites] device temporaries, the mask table (if any) padded to 256 entries of "every state"
static cmx_status upload_host_alignment(cmx_ctx* ctx, TmpDev& tmp, const uint8_t* aln, size_t nsites, size_t ld, const uint32_t* masks,
                                        size_t nmasks, uint8_t** d_aln, uint32_t** d_masks) {
  const HostModel& h = ctx->hm;
  CMX_TRY(tmp.alloc(ctx, d_aln, (size_t)h.T * nsites));
  HIP_TRY(ctx, hipMemcpy2D(*d_aln, nsites, aln, ld, nsites, h.T, hipMemcpyHostToDevice));
  if (masks) {
    std::vector<uint32_t> mk(256, h.S >= 32 ? 0xffffffffu : ((1u << h.S) - 1u));
    for (size_t i = 0; i < nmasks && i < 256; ++i) mk[i] = masks[i];
    CMX_TRY(tmp.upload(ctx, d_masks, mk.data(), 256));
  }
  return CMX_OK;
}

cmx_status cmx_map_sites(cmx_ctx* ctx, const uint8_t* aln, size_t nsites, size_t ld, const uint32_t* masks,
                         size_t nmasks, double* counts, double* logL, double* post_rate, int32_t* rate_class,
                         double* norm) {
  CMX_TRY(check_host_alignment(ctx, "cmx_map_sites", aln, nsites, ld, masks, nmasks));
  const HostModel& h = ctx->hm;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  uint8_t* d_aln = nullptr;
  uint32_t* d_masks = nullptr;
  double *d_counts = nullptr, *d_logL = nullptr, *d_pr = nullptr, *d_norm = nullptr;
  int32_t* d_rc = nullptr;
  const size_t BK = (size_t)h.B * h.K;
  CMX_TRY(upload_host_alignment(ctx, tmp, aln, nsites, ld, masks, nmasks, &d_aln, &d_masks));
  if (counts) CMX_TRY(tmp.alloc(ctx, &d_counts, BK * nsites));
  CMX_TRY(tmp.alloc(ctx, &d_logL, nsites));
  CMX_TRY(tmp.alloc(ctx, &d_pr, nsites));
  CMX_TRY(tmp.alloc(ctx, &d_norm, nsites));
  CMX_TRY(tmp.alloc(ctx, &d_rc, nsites));
  CMX_TRY(cmx_map_sites_dev(ctx, d_aln, nsites, nsites, d_masks, d_counts, nsites, d_logL, d_pr, d_rc, d_norm, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (counts) {  // branch-major [B*K][N] -> site-major [N][B][K] (reference layout mapping[i][b][k])
    std::vector<double> bm(BK * nsites);
    CMX_TRY(download(ctx, bm.data(), d_counts, bm.size()));
    for (size_t r = 0; r < BK; ++r)
      for (size_t i = 0; i < nsites; ++i) counts[i * BK + r] = bm[r * nsites + i];
  }
  CMX_TRY(download(ctx, logL, d_logL, nsites));
  CMX_TRY(download(ctx, post_rate, d_pr, nsites));
  CMX_TRY(download(ctx, norm, d_norm, nsites));
  return download(ctx, rate_class, d_rc, nsites);
}

// asr.method = marginal (CoMap/CoMap.cpp:169-197): the inside / outside kernels of the mapping variants, then
// ancestral_kernel (cmx_variants.hip).  Scratch of its own ("asr_nodes", not the mapping's "va_nodes_*"), so it may run on
// a stream beside a mapping or a null; it reads the caller's mask table directly and leaves the leaf operators' ambiguity
// rows and the kept Gram blocks alone.  Sites per pass: the four per-node vectors of a pass stay under kAsrScratchBytes,
// the passes balanced and rounded up to whole workgroups.  need_inner_nodes: the rows of the result, uploaded at the first use.
static cmx_status need_inner_nodes(cmx_ctx* ctx) {
  if (ctx->asr_inner) return CMX_OK;
  std::vector<int> inner;
  for (int n = 0; n < ctx->hm.nn; ++n)
    if (ctx->hm.first_child[n] >= 0) inner.push_back(n);
  CMX_TRY(upload(ctx, inner, &ctx->asr_inner));
  ctx->asr_n_inner = (int)inner.size();
  return CMX_OK;
}

cmx_status cmx_ancestral_states_dev(cmx_ctx* ctx, const uint8_t* d_aln, size_t nsites, size_t ld, const uint32_t* d_masks,
                                    uint8_t* d_states, size_t lds, double* d_post, size_t ldp, void* stream) {
  CMX_TRY(need_model(ctx));
  const HostModel& h = ctx->hm;
  if (!d_aln || nsites == 0 || ld < nsites) return fail(ctx, CMX_ERR_INVALID, "cmx_ancestral_states: bad alignment arguments");
  if (d_masks && h.plain)
    return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_ancestral_states: no ambiguity table for alphabets other than 4 / 20 states (codes >= nstates are unknowns)");
  if (!d_states) return fail(ctx, CMX_ERR_INVALID, "cmx_ancestral_states: states is NULL");
  if (lds < nsites) return fail(ctx, CMX_ERR_INVALID, "cmx_ancestral_states: lds < nsites");
  if (d_post && ldp < nsites) return fail(ctx, CMX_ERR_INVALID, "cmx_ancestral_states: ldp < nsites");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  CMX_TRY(upload_variant_operators(ctx));
  CMX_TRY(need_inner_nodes(ctx));
  PlainArgs a = plain_args(ctx, MapIn{d_aln, nsites, ld, d_masks});
  a.chunk = plain_sites_per_pass(a.S, h.C, h.nn, nsites, kAsrScratchBytes, true);
  double* buf;
  CMX_TRY(scratch(ctx, "asr_nodes", plain_node_doubles(a.S, h.C, h.nn, a.chunk), &buf));
  int32_t* exps = nullptr;
  if (ctx->scaling) CMX_TRY(scratch(ctx, "asr_exps", plain_exponent_ints(h.C, h.nn, a.chunk), &exps));
  HIP_TRY(ctx, launch_ancestral(a, nsites, buf, exps, ctx->asr_inner, ctx->asr_n_inner, d_states, lds, d_post, ldp, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_ancestral_states(cmx_ctx* ctx, const uint8_t* aln, size_t nsites, size_t ld, const uint32_t* masks, size_t nmasks,
                                uint8_t* states, double* post) {
  CMX_TRY(check_host_alignment(ctx, "cmx_ancestral_states", aln, nsites, ld, masks, nmasks));
  if (!states) return fail(ctx, CMX_ERR_INVALID, "cmx_ancestral_states: states is NULL");
  const HostModel& h = ctx->hm;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  uint8_t* d_aln = nullptr;
  uint32_t* d_masks = nullptr;
  uint8_t* d_states = nullptr;
  double* d_post = nullptr;
  CMX_TRY(upload_host_alignment(ctx, tmp, aln, nsites, ld, masks, nmasks, &d_aln, &d_masks));
  CMX_TRY(need_inner_nodes(ctx));
  const int n_inner = ctx->asr_n_inner;
  CMX_TRY(tmp.alloc(ctx, &d_states, (size_t)n_inner * nsites));
  if (post) CMX_TRY(tmp.alloc(ctx, &d_post, (size_t)n_inner * h.S * nsites));
  CMX_TRY(cmx_ancestral_states_dev(ctx, d_aln, nsites, nsites, d_masks, d_states, nsites, d_post, nsites, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, states, d_states, (size_t)n_inner * nsites));
  if (post) {   // [n_inner][S][N] -> [n_inner][N][S]
    std::vector<double> pm((size_t)n_inner * h.S * nsites);
    CMX_TRY(download(ctx, pm.data(), d_post, pm.size()));
    for (int q = 0; q < n_inner; ++q)
      for (int x = 0; x < h.S; ++x)
        for (size_t i = 0; i < nsites; ++i) post[((size_t)q * nsites + i) * h.S + x] = pm[((size_t)q * h.S + x) * nsites + i];
  }
  return CMX_OK;
}

// ------------------------------------------------------------------------------------------------ simulator
cmx_status cmx_simulate_dev(cmx_ctx* ctx, uint64_t seed, uint64_t g0, size_t n, uint8_t* d_aln, size_t ld, int32_t* d_classes,
                            void* stream) {
  CMX_TRY(need_model(ctx));
  if (!d_aln || n == 0 || ld < n) return fail(ctx, CMX_ERR_INVALID, "cmx_simulate: bad arguments");
  CMX_TRY(rng_range(ctx, g0 + n, "cmx_simulate"));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // node states of the n sites: a scratch of their own per stream would be needed to overlap two simulations of one
  // context; calls on one context are serialised by the caller (header)
  uint8_t* d_st;
  int32_t* d_cls = d_classes;
  CMX_TRY(scratch(ctx, "sim_states", (size_t)ctx->hm.nn * ld, &d_st));
  if (!d_cls) CMX_TRY(scratch(ctx, "sim_classes", n, &d_cls));
  HIP_TRY(ctx, launch_simulate(ctx->dm, seed, g0, n, d_aln, ld, d_cls, d_st, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_simulate(cmx_ctx* ctx, uint64_t seed, uint64_t g0, size_t n, uint8_t* aln_out, int32_t* classes_out) {
  CMX_TRY(need_model(ctx));
  if (!aln_out || n == 0) return fail(ctx, CMX_ERR_INVALID, "cmx_simulate: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HostModel& h = ctx->hm;
  TmpDev tmp;
  uint8_t* d_aln = nullptr;
  int32_t* d_cls = nullptr;
  CMX_TRY(tmp.alloc(ctx, &d_aln, (size_t)h.T * n));
  CMX_TRY(tmp.alloc(ctx, &d_cls, n));
  CMX_TRY(cmx_simulate_dev(ctx, seed, g0, n, d_aln, n, d_cls, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, aln_out, d_aln, (size_t)h.T * n));
  return download(ctx, classes_out, d_cls, n);
}

cmx_status cmx_simulate_continuous_dev(cmx_ctx* ctx, uint64_t seed, uint64_t g0, size_t n, double gamma_alpha, double p_invariant,
                                       uint8_t* d_aln, size_t ld, double* d_rates, void* stream) {
  CMX_TRY(need_model(ctx));
  if (!d_aln || n == 0 || ld < n || !(gamma_alpha > 0.0) || !(p_invariant >= 0.0 && p_invariant < 1.0))
    return fail(ctx, CMX_ERR_INVALID, "cmx_simulate_continuous: bad arguments (alpha > 0, 0 <= p_invariant < 1)");
  CMX_TRY(rng_range(ctx, g0 + n, "cmx_simulate_continuous"));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint8_t* d_st;
  CMX_TRY(scratch(ctx, "sim_states", (size_t)ctx->hm.nn * ld, &d_st));
  HIP_TRY(ctx, launch_simulate_continuous(ctx->dm, seed, g0, n, gamma_alpha, p_invariant, d_aln, ld, d_rates, d_st, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_simulate_continuous(cmx_ctx* ctx, uint64_t seed, uint64_t g0, size_t n, double gamma_alpha, double p_invariant,
                                   uint8_t* aln_out, double* rates_out) {
  CMX_TRY(need_model(ctx));
  if (!aln_out || n == 0) return fail(ctx, CMX_ERR_INVALID, "cmx_simulate_continuous: bad arguments (alpha > 0, 0 <= p_invariant < 1)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HostModel& h = ctx->hm;
  TmpDev tmp;
  uint8_t* d_aln = nullptr;
  double* d_r = nullptr;
  CMX_TRY(tmp.alloc(ctx, &d_aln, (size_t)h.T * n));
  CMX_TRY(tmp.alloc(ctx, &d_r, n));
  CMX_TRY(cmx_simulate_continuous_dev(ctx, seed, g0, n, gamma_alpha, p_invariant, d_aln, n, d_r, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, aln_out, d_aln, (size_t)h.T * n));
  return download(ctx, rates_out, d_r, n);
}

