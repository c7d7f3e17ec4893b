// C-ABI, null stage: the simulated null distributions of one data set (fused into the mapping waves, or by distinct
// site patterns), of two data sets (simulate -> map -> score), and their host-pointer wrappers.
#include "cmx_ctx.h"

// pass budgets in bytes; CMX_NULL_PASS_BYTES replaces them where tests exercise the multi-pass paths with small nulls
constexpr size_t kNullAlnPassBytes = (size_t)4 << 30;   // the simulated alignments of a pass
static size_t null_pass_bytes(size_t dflt) {
  static const size_t env = [] {
    const char* e = getenv("CMX_NULL_PASS_BYTES");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)0;
  }();
  return env ? env : dflt;
}

// The null's alignments, [replicate][batch][taxon][rep_ram] bytes (what cmx_null_intra_dev takes as `supplied`):
// NonHomogeneousSequenceSimulator::simulate(repRAM) twice per replicate (AnalysisTools.cpp:591, 612), simulated-site index
// g = ((rep * 2 + batch) * rep_ram + j) as everywhere.
cmx_status cmx_null_simulate_dev(cmx_ctx* ctx, uint64_t seed, size_t rep_begin, size_t rep_end, size_t rep_ram, uint8_t* d_aln,
                                 void* stream) {
  CMX_TRY(need_model(ctx));
  if (rep_end <= rep_begin || rep_ram == 0 || !d_aln) return fail(ctx, CMX_ERR_INVALID, "cmx_null_simulate: bad arguments");
  CMX_TRY(rng_range(ctx, (uint64_t)rep_end * 2 * rep_ram, "cmx_null_simulate"));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nsites = (rep_end - rep_begin) * 2 * rep_ram;
  // node states of a pass: nn bytes per site, up to 4 GiB -- one pass for the 2 * 10^7 sites of the target's null (nine
  // passes of 2^21 sites left nine tails of half-empty CUs)
  const size_t chunk = std::min<size_t>(nsites, std::max<size_t>((size_t)1 << 21, (((size_t)4 << 30) / (size_t)ctx->hm.nn) & ~(size_t)1023));
  uint8_t* d_states;
  CMX_TRY(scratch(ctx, "null_states", (size_t)ctx->hm.nn * chunk, &d_states));
  const SimChoice choice{ctx->d_simtab, g_sim_min_sites.load(), g_sim_four_batch_sites.load()};
  HIP_TRY(ctx, launch_simulate_blocked(ctx->dm, seed, (uint64_t)rep_begin * 2 * rep_ram, nsites, rep_ram, d_aln, d_states, chunk,
                                       (hipStream_t)stream, choice));
  return CMX_OK;
}

// ------------------------------------------------------------------------------------------------ inter-gene null
// AnalysisTools::getNullDistributionInterDR (AnalysisTools.cpp:662-735): per replicate simulate + map rep_ram sites
// under data set 1 and rep_ram sites under data set 2, then score site j of the one against site j of the other.
// Not fused (a "next" row of SURVEY 8f): simulate -> map -> diagonal-pair kernel, everything resident in HBM.
// Simulated-site indices follow the intra scheme: g = ((rep*2 + h)*rep_ram + j), h = 0 for ctx1 and 1 for ctx2.
// d_supplied (intra use only: both contexts the same): [nrep][2][T][rep_ram] alignments to map instead of simulating
static cmx_status null_unfused_dev(cmx_ctx* ctx1, cmx_ctx* ctx2, int kind, const double* params, uint64_t seed,
                                   size_t rep_begin, size_t rep_end, size_t rep_ram, const uint8_t* d_supplied, double* d_stat,
                                   int32_t* d_rcmin, double* d_prmin, double* d_nmin, void* stream) {
  CMX_TRY(need_model(ctx1));
  if (!ctx2 || !ctx2->has_model) return fail(ctx1, CMX_ERR_INVALID, "cmx_null_inter: second context has no model");
  CMX_TRY(check_kind(ctx1, kind));
  if (rep_end <= rep_begin || rep_ram == 0 || !d_stat) return fail(ctx1, CMX_ERR_INVALID, "cmx_null_inter: bad arguments");
  CMX_TRY(rng_range(ctx1, (uint64_t)rep_end * 2 * rep_ram, "cmx_null_inter"));
  CMX_TRY(rng_range(ctx2, (uint64_t)rep_end * 2 * rep_ram, "cmx_null_inter"));
  if (ctx1->device != ctx2->device) return fail(ctx1, CMX_ERR_INVALID, "cmx_null_inter: contexts live on different devices");
  if (ctx1->hm.B != ctx2->hm.B || ctx1->hm.K != ctx2->hm.K)
    return fail(ctx1, CMX_ERR_INVALID, "cmx_null_inter: the two data sets must have the same branches and substitution types "
                                       "(Statistic::getValueForPair throws DimensionException otherwise)");
  HIP_TRY(ctx1, hipSetDevice(ctx1->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t nrep = rep_end - rep_begin, n = nrep * rep_ram;
  const size_t BK = (size_t)ctx1->hm.B * ctx1->hm.K;
  double *cnt[2], *pr[2], *nm[2];
  int32_t* rc[2];
  cmx_ctx* cx[2] = {ctx1, ctx2};
  for (int h = 0; h < 2; ++h) {
    cmx_ctx* c = cx[h];
    const std::string tag = std::string("inter") + char('0' + h);
    uint8_t *d_aln, *d_st;
    CMX_TRY(scratch(ctx1, (tag + "_aln").c_str(), (size_t)c->hm.T * n, &d_aln));
    // (node states share the alignment's row stride n in simulate_kernel: [nn][n], not [nn][rep_ram] -- sized for rep_ram
    // this overflowed as soon as a call held more than one replicate)
    CMX_TRY(scratch(ctx1, (tag + "_st").c_str(), (size_t)c->hm.nn * n, &d_st));
    CMX_TRY(scratch(ctx1, (tag + "_cnt").c_str(), BK * n, &cnt[h]));
    CMX_TRY(scratch(ctx1, (tag + "_pr").c_str(), n, &pr[h]));
    CMX_TRY(scratch(ctx1, (tag + "_nm").c_str(), n, &nm[h]));
    CMX_TRY(scratch(ctx1, (tag + "_rc").c_str(), n, &rc[h]));
    if (d_supplied) {
      for (size_t r = 0; r < nrep; ++r)   // batch h of replicate r: [T][rep_ram] -> columns r * rep_ram .. of the [T][n] alignment
        HIP_TRY(ctx1, hipMemcpy2DAsync(d_aln + r * rep_ram, n, d_supplied + ((r * 2 + h) * (size_t)c->hm.T) * rep_ram, rep_ram, rep_ram,
                                       (size_t)c->hm.T, hipMemcpyDeviceToDevice, st));
    } else {
      // ONE launch for all replicates of this side (round 3: one per replicate and side -- 2 000 tiny launches for
      // nb_rep_CPU = 1000): block r of rep_ram columns holds the global sites ((rep_begin + r) * 2 + h) * rep_ram ..
      const uint64_t g0 = ((uint64_t)rep_begin * 2 + h) * (uint64_t)rep_ram;
      HIP_TRY(ctx1, launch_simulate(c->dm, seed, g0, n, d_aln, n, nullptr, d_st, st, rep_ram, 2 * (uint64_t)rep_ram));
    }
    const cmx_status s = map_sites_impl(c, d_aln, n, n, nullptr, cnt[h], n, nullptr, pr[h], rc[h], nm[h], stream, true);
    if (s != CMX_OK) { if (c != ctx1) ctx1->err = c->err; return s; }
  }
  Stat sk;
  CMX_TRY(resolve_stat(ctx1, kind, params, stream, &sk));
  const SiteCols cols[2] = {{rc[0], pr[0], nm[0]}, {rc[1], pr[1], nm[1]}};
  const PairOut out{d_stat, d_rcmin, d_prmin, d_nmin};
  if (sk.mi()) {   // the statistic from the class words; the diagonal kernel writes the minima only
    PairOperand a, b;
    CMX_TRY(pair_operand(ctx1, sk, cnt[0], n, n, "n1", st, &a));
    CMX_TRY(pair_operand(ctx1, sk, cnt[1], n, n, "n2", st, &b));
    HIP_TRY(ctx1, launch_mi_pairs_diag(sk.B, a, b, n, d_stat, st));
    HIP_TRY(ctx1, launch_pair_diag(sk, cnt[0], n, cols[0], cnt[1], n, cols[1], n, PairOut{nullptr, d_rcmin, d_prmin, d_nmin}, st));
    return CMX_OK;
  }
  // branch weights: ctx1's (the reference scores both data sets with one Statistic object, AnalysisTools.cpp:728)
  HIP_TRY(ctx1, launch_pair_diag(sk, cnt[0], n, cols[0], cnt[1], n, cols[1], n, out, st));
  return CMX_OK;
}

// The fused null's distinct columns (cmx_null_patterns.hip).  Per site of a pass the pattern path holds, at
// worst (every site its own pattern), B*K doubles of counts, the packed column and 84 bytes of keys, indices and per-pattern
// scalars (mean and squared deviations among them); a pass is as many whole replicates as fit kNullPatternPassBytes
// (CMX_NULL_PASS_BYTES in tests).  One pass at the target (2 * 10^7 sites x 1 148 bytes): the deduplication is done over
// the whole launch, with a single mapping tail.  The count table is rounded up to whole tiles of one mapping wave's
// patterns (under 64 KB a pass): that rounding is no part of the replicates-per-pass arithmetic.
constexpr size_t kNullPatternPassBytes = (size_t)24 << 30;

static size_t null_pattern_site_bytes(const cmx_ctx* ctx) {
  return (size_t)ctx->hm.B * ctx->hm.K * sizeof(double) + null_pattern_row_bytes(ctx->hm.T) + 84;
}

// replicates per pattern pass, or 0: map every site of every pair (patterns off, or one replicate exceeds the budget)
static size_t null_pattern_reps(const cmx_ctx* ctx, size_t rep_ram) {
  const bool on = ctx->null_patterns < 0 ? (ctx->hm.S == 20 && ctx->hm.fuse == 1) : ctx->null_patterns == 1;
  if (!on) return 0;
  const size_t budget = null_pass_bytes(kNullPatternPassBytes);
  const size_t per_rep = 2 * rep_ram * null_pattern_site_bytes(ctx);
  if (per_rep > budget || 2 * rep_ram > ((size_t)1 << 31)) return 0;
  return std::min(budget / per_rep, ((size_t)1 << 31) / (2 * rep_ram));   // (32-bit site indices)
}

// a.supplied / a.rep_ram / a.null_* describe the whole null, sk its statistic; passes of whole replicates, sized evenly
static cmx_status null_patterns_dev(cmx_ctx* ctx, const Stat& sk, MapArgs a, size_t nrep, size_t reps_max, void* stream) {
  const HostModel& h = ctx->hm;
  const size_t rep_ram = a.rep_ram, T = (size_t)h.T, BK = (size_t)h.B * h.K, rowb = null_pattern_row_bytes(h.T);
  const size_t npass = (nrep + reps_max - 1) / reps_max, reps = (nrep + npass - 1) / npass;
  const size_t cap = reps * 2 * rep_ram;   // sites of the largest pass
  NullPatternBufs b{};
  double *cnt, *pr, *nm;
  int32_t* rc;
  CMX_TRY(scratch(ctx, "pat_key", cap, &b.key));
  CMX_TRY(scratch(ctx, "pat_key_s", cap, &b.key_s));
  CMX_TRY(scratch(ctx, "pat_g", cap, &b.g));
  CMX_TRY(scratch(ctx, "pat_g_s", cap, &b.g_s));
  CMX_TRY(scratch(ctx, "pat_col", rowb * cap, &b.col));
  CMX_TRY(scratch(ctx, "pat_head", cap, &b.head));
  CMX_TRY(scratch(ctx, "pat_incl", cap, &b.incl));
  CMX_TRY(scratch(ctx, "pat_of", cap, &b.pat_of));
  CMX_TRY(scratch(ctx, "pat_site", cap, &b.rep_site));
  // tile-major: a mapping wave's ks patterns are one [B*K][ks] block, the last tile whole (its spare columns are written)
  const size_t ks = (size_t)map_sites_per_wave(h.dS), ntiles = (cap + ks - 1) / ks;
  CMX_TRY(scratch(ctx, "pat_cnt", BK * ks * ntiles, &cnt));
  // Correlation / Covariance: the pairs are scored in one pass from per-pattern moments (pair_stat_moments)
  const bool moments = sk.kind == CMX_STAT_CORRELATION || sk.kind == CMX_STAT_COVARIANCE;
  double *pmean = nullptr, *pss = nullptr;
  if (moments) {
    CMX_TRY(scratch(ctx, "pat_mean", cap, &pmean));
    CMX_TRY(scratch(ctx, "pat_ss", cap, &pss));
  }
  CMX_TRY(scratch(ctx, "pat_pr", cap, &pr));
  CMX_TRY(scratch(ctx, "pat_nm", cap, &nm));
  CMX_TRY(scratch(ctx, "pat_rc", cap, &rc));
  CMX_TRY(scratch(ctx, "pat_total", 1, &b.total));
  const int hash_bits = g_pat_hash_bits.load();
  HIP_TRY(ctx, null_pattern_tmp_bytes(cap, hash_bits, &b.tmp_bytes));
  CMX_TRY(scratch(ctx, "pat_tmp", b.tmp_bytes ? b.tmp_bytes : 16, &b.tmp));
  if (!ctx->null_mapped_dev) {
    HIP_TRY(ctx, hipMemsetAsync(b.total, 0, sizeof(unsigned long long), (hipStream_t)stream));
    ctx->null_mapped_dev = true;
  }
  const uint8_t* sup = a.supplied;
  const PairOut out{a.null_stat, a.null_rcmin, a.null_prmin, a.null_nmin};
  a.counts = cnt; a.ldc = 0; a.post_rate = pr; a.rate_class = rc; a.norm = nm;
  a.rep_site = b.rep_site;
  for (size_t r0 = 0; r0 < nrep; r0 += reps) {
    const size_t r1 = std::min(nrep, r0 + reps), n = (r1 - r0) * 2 * rep_ram;
    a.supplied = sup + r0 * 2 * T * rep_ram;
    HIP_TRY(ctx, launch_null_patterns(a.supplied, h.T, rep_ram, n, hash_bits, b, (hipStream_t)stream));
    // the pattern count stays on the device: the grid is sized for every site its own pattern, the waves read the count
    a.nsites = n;
    a.npat = b.incl + (n - 1);
    const size_t blocks_needed = ((n + ks - 1) / ks + kWavesPerBlock - 1) / kWavesPerBlock;
    const int grid = (int)std::min<size_t>(blocks_needed, (size_t)ctx->grid_blocks);
    CMX_TRY(map_queue_take(ctx, (n + ks - 1) / ks, grid, (hipStream_t)stream, &a.queue));
    HIP_TRY(ctx, launch_map(a, a.cherry_msg ? kModeNullPatternsMsg : kModeNullPatterns, grid, (hipStream_t)stream));
    if (moments)
      HIP_TRY(ctx, launch_null_pattern_moments(h.B, h.K, cnt, (int)ks, (int)ks, a.npat, n, pmean, pss, (hipStream_t)stream));
    HIP_TRY(ctx, launch_null_pattern_pairs(sk, cnt, (int)ks, (int)ks, pmean, pss, SiteCols{rc, pr, nm}, b.pat_of, rep_ram, n / 2, out.at(r0 * rep_ram),
                                           (hipStream_t)stream));
  }
  return CMX_OK;
}

cmx_status cmx_null_intra_dev(cmx_ctx* ctx, int kind, const double* params, uint64_t seed, size_t rep_begin,
                              size_t rep_end, size_t rep_ram, const uint8_t* d_supplied, double* d_stat,
                              int32_t* d_rcmin, double* d_prmin, double* d_nmin, void* stream) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_kind(ctx, kind));
  if (rep_end <= rep_begin || rep_ram == 0 || !d_stat) return fail(ctx, CMX_ERR_INVALID, "cmx_null_intra: bad arguments");
  CMX_TRY(rng_range(ctx, (uint64_t)rep_end * 2 * rep_ram, "cmx_null_intra"));
  if (!ctx->map_average || !ctx->map_joint || kind == CMX_STAT_DISCRETE_MI_BOUNDS || ctx->hm.plain || stat_weights(ctx, kind) || ctx->scaling) {
    // nijt.average = no (AnalysisTools.cpp:598-610): the fused kernel only knows the averaged mapping; and a statistic that
    // needs a joint table per pair cannot be evaluated per lane inside the mapping wave.  The same simulate -> map ->
    // score sequence then runs unfused, which is what the two-data-set null does with both sides equal.  So does a
    // statistic with branch weights (map_kernel's lanes score unweighted only), and a context with likelihood scaling (the
    // fused kernel is the unscaled walk).
    if (ctx->null_depth == 0) { ctx->null_mapped_host = 2 * (rep_end - rep_begin) * rep_ram; ctx->null_mapped_dev = false; }
    return null_unfused_dev(ctx, ctx, kind, params, seed, rep_begin, rep_end, rep_ram, d_supplied, d_stat, d_rcmin, d_prmin, d_nmin, stream);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->null_depth == 0) { ctx->null_mapped_host = 0; ctx->null_mapped_dev = false; }
  const PairOut out{d_stat, d_rcmin, d_prmin, d_nmin};
  if (!d_supplied) {
    // simulate first, at full occupancy, then map the alignments as "supplied" ones: the same draws, the same results
    // as a simulator inside the mapping waves (round 1; 7.8 % of the launch there, latency nobody could hide).  The
    // alignments of a pass stay under 4 GiB: a larger null runs as several passes over replicate ranges.
    const size_t per_rep = 2 * (size_t)ctx->hm.T * rep_ram;
    const size_t reps_per_pass = std::max<size_t>(1, null_pass_bytes(kNullAlnPassBytes) / per_rep);
    if (rep_end - rep_begin > reps_per_pass) {
      cmx_status s = CMX_OK;
      ++ctx->null_depth;
      for (size_t r0 = rep_begin; r0 < rep_end && s == CMX_OK; r0 += reps_per_pass) {
        const PairOut o = out.at((r0 - rep_begin) * rep_ram);
        s = cmx_null_intra_dev(ctx, kind, params, seed, r0, std::min(rep_end, r0 + reps_per_pass), rep_ram, nullptr, o.stat, o.rcmin, o.prmin,
                               o.nmin, stream);
      }
      --ctx->null_depth;
      return s;
    }
    uint8_t* d_aln;
    CMX_TRY(scratch(ctx, "null_aln", (rep_end - rep_begin) * per_rep, &d_aln));
    CMX_TRY(cmx_null_simulate_dev(ctx, seed, rep_begin, rep_end, rep_ram, d_aln, stream));
    d_supplied = d_aln;
  }
  MapArgs a{};
  a.m = ctx->dm; a.ws = ctx->ws;
  a.nsites = (rep_end - rep_begin) * rep_ram;
  Stat sk;
  CMX_TRY(resolve_stat(ctx, kind, params, stream, &sk));
  a.stat_kind = kind; a.stat_param = sk.param; a.stat_mean = sk.d_mean;
  a.rep_ram = rep_ram; a.supplied = d_supplied;
  a.null_stat = d_stat; a.null_rcmin = d_rcmin; a.null_prmin = d_prmin; a.null_nmin = d_nmin;
  a.plan_r = ctx->d_plan_r; a.cherry_msg = ctx->d_cherry_msg;   // (a model with a cherry message table: the walk gathers the cherries' messages)
  const size_t reps_per_pass = null_pattern_reps(ctx, rep_ram);
  if (reps_per_pass) return null_patterns_dev(ctx, sk, a, rep_end - rep_begin, reps_per_pass, stream);
  const size_t ks = (size_t)map_sites_per_wave(ctx->hm.dS);
  const size_t blocks_needed = ((a.nsites + ks - 1) / ks + kWavesPerBlock - 1) / kWavesPerBlock;
  const int grid = (int)std::min<size_t>(blocks_needed, (size_t)ctx->grid_blocks);
  CMX_TRY(map_queue_take(ctx, (a.nsites + ks - 1) / ks, grid, (hipStream_t)stream, &a.queue));
  HIP_TRY(ctx, launch_map(a, a.cherry_msg ? kModeNullMsg : kModeNull, grid, (hipStream_t)stream));
  ctx->null_mapped_host += 2 * a.nsites;
  return CMX_OK;
}

// simulations.continuous = yes (CoMap.cpp:146, 213): the replicates' alignments come from the continuous-rate simulator,
// straight into the device buffer cmx_null_intra_dev maps as "supplied" alignments -- nothing crosses PCIe
cmx_status cmx_null_intra_continuous_dev(cmx_ctx* ctx, int kind, const double* params, uint64_t seed, size_t rep_begin, size_t rep_end,
                                         size_t rep_ram, double gamma_alpha, double p_invariant, double* d_stat, int32_t* d_rcmin,
                                         double* d_prmin, double* d_nmin, void* stream) {
  CMX_TRY(need_model(ctx));
  if (rep_end <= rep_begin || rep_ram == 0 || !d_stat) return fail(ctx, CMX_ERR_INVALID, "cmx_null_intra_continuous: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t T = (size_t)ctx->hm.T, per_rep = 2 * T * rep_ram;
  const size_t reps_per_pass = std::max<size_t>(1, kNullAlnPassBytes / per_rep);   // (not the tests' override)
  const PairOut out{d_stat, d_rcmin, d_prmin, d_nmin};
  uint8_t* d_aln;
  CMX_TRY(scratch(ctx, "null_aln", std::min(reps_per_pass, rep_end - rep_begin) * per_rep, &d_aln));
  for (size_t r0 = rep_begin; r0 < rep_end; r0 += reps_per_pass) {
    const size_t r1 = std::min(rep_end, r0 + reps_per_pass);
    const PairOut o = out.at((r0 - rep_begin) * rep_ram);
    for (size_t r = r0; r < r1; ++r)
      for (int h = 0; h < 2; ++h)   // [replicate][batch][taxon][rep_ram]; simulated-site index g = (rep * 2 + batch) * rep_ram + j
        CMX_TRY(cmx_simulate_continuous_dev(ctx, seed, ((uint64_t)r * 2 + h) * rep_ram, rep_ram, gamma_alpha, p_invariant,
                                            d_aln + ((r - r0) * 2 + h) * T * rep_ram, rep_ram, nullptr, stream));
    CMX_TRY(cmx_null_intra_dev(ctx, kind, params, seed, r0, r1, rep_ram, d_aln, o.stat, o.rcmin, o.prmin, o.nmin, stream));
  }
  return CMX_OK;
}

cmx_status cmx_null_intra_continuous(cmx_ctx* ctx, int kind, const double* params, uint64_t seed, size_t rep_begin, size_t rep_end,
                                     size_t rep_ram, double gamma_alpha, double p_invariant, double* stat, int32_t* rcmin,
                                     double* prmin, double* nmin) {
  CMX_TRY(need_model(ctx));
  if (rep_end <= rep_begin || rep_ram == 0 || !stat) return fail(ctx, CMX_ERR_INVALID, "cmx_null_intra_continuous: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (rep_end - rep_begin) * rep_ram;
  TmpDev tmp;
  PairOut d;
  CMX_TRY(alloc_out(ctx, tmp, n, &d));
  CMX_TRY(cmx_null_intra_continuous_dev(ctx, kind, params, seed, rep_begin, rep_end, rep_ram, gamma_alpha, p_invariant, d.stat, d.rcmin, d.prmin,
                                        d.nmin, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  return fetch_out(ctx, n, d, {stat, rcmin, prmin, nmin});
}

cmx_status cmx_null_intra(cmx_ctx* ctx, int kind, const double* params, uint64_t seed, size_t rep_begin, size_t rep_end,
                          size_t rep_ram, const uint8_t* supplied, double* stat, int32_t* rcmin, double* prmin,
                          double* nmin) {
  CMX_TRY(need_model(ctx));
  if (rep_end <= rep_begin || rep_ram == 0 || !stat) return fail(ctx, CMX_ERR_INVALID, "cmx_null_intra: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (rep_end - rep_begin) * rep_ram;
  TmpDev tmp;
  uint8_t* d_sup = nullptr;
  PairOut d;
  if (supplied) {
    const size_t bytes = (rep_end - rep_begin) * 2 * (size_t)ctx->hm.T * rep_ram;
    for (size_t i = 0; i < bytes; ++i)
      if (supplied[i] >= (unsigned)ctx->hm.S) return fail(ctx, CMX_ERR_INVALID, "cmx_null_intra: supplied alignments must be fully resolved");
    CMX_TRY(tmp.upload(ctx, &d_sup, supplied, bytes));
  }
  CMX_TRY(alloc_out(ctx, tmp, n, &d));
  CMX_TRY(cmx_null_intra_dev(ctx, kind, params, seed, rep_begin, rep_end, rep_ram, d_sup, d.stat, d.rcmin, d.prmin, d.nmin, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  return fetch_out(ctx, n, d, {stat, rcmin, prmin, nmin});
}

cmx_status cmx_null_inter_dev(cmx_ctx* ctx1, cmx_ctx* ctx2, int kind, const double* params, uint64_t seed,
                              size_t rep_begin, size_t rep_end, size_t rep_ram, double* d_stat, int32_t* d_rcmin,
                              double* d_prmin, double* d_nmin, void* stream) {
  return null_unfused_dev(ctx1, ctx2, kind, params, seed, rep_begin, rep_end, rep_ram, nullptr, d_stat, d_rcmin, d_prmin, d_nmin, stream);
}

cmx_status cmx_null_inter(cmx_ctx* ctx1, cmx_ctx* ctx2, int kind, const double* params, uint64_t seed, size_t rep_begin,
                          size_t rep_end, size_t rep_ram, double* stat, int32_t* rcmin, double* prmin, double* nmin) {
  CMX_TRY(need_model(ctx1));
  if (rep_end <= rep_begin || rep_ram == 0 || !stat) return fail(ctx1, CMX_ERR_INVALID, "cmx_null_inter: bad arguments");
  HIP_TRY(ctx1, hipSetDevice(ctx1->device));
  const size_t n = (rep_end - rep_begin) * rep_ram;
  TmpDev tmp;
  PairOut d;
  CMX_TRY(alloc_out(ctx1, tmp, n, &d));
  CMX_TRY(cmx_null_inter_dev(ctx1, ctx2, kind, params, seed, rep_begin, rep_end, rep_ram, d.stat, d.rcmin, d.prmin, d.nmin, nullptr));
  HIP_TRY(ctx1, hipDeviceSynchronize());
  return fetch_out(ctx1, n, d, {stat, rcmin, prmin, nmin});
}

cmx_status cmx_null_pattern_count(cmx_ctx* ctx, unsigned long long* count) {
  CMX_TRY(need_model(ctx));
  if (!count) return fail(ctx, CMX_ERR_INVALID, "cmx_null_pattern_count: count is NULL");
  unsigned long long n = ctx->null_mapped_host;
  if (ctx->null_mapped_dev) {
    void* p = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    CMX_TRY(scratch(ctx, "pat_total", sizeof(unsigned long long), &p));
    unsigned long long d = 0;
    HIP_TRY(ctx, hipMemcpy(&d, p, sizeof d, hipMemcpyDeviceToHost));
    n += d;
  }
  *count = n;
  return CMX_OK;
}

