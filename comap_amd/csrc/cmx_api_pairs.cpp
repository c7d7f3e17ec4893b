// C-ABI, pair stage: the pair statistics and their parameters, p-values against a null, the pair loop (filtered rows,
// compact records, kept Gram blocks) of one and of two data sets, groups of sites and candidate groups.
#include <thread>

#include "cmx_ctx.h"

// A parameter block of an asynchronous call on the device: copied on the CALLER's stream (a blocking copy on the null
// stream does not order against torch's non-blocking streams) into one of eight rotating buffers, so that a later call
// cannot overwrite values a kernel still in flight is reading.  The host copy outlives the asynchronous upload.
static cmx_status upload_params(cmx_ctx* ctx, const char* what, const double* v, size_t count, void* stream, const double** d) {
  double* p = nullptr;
  const unsigned turn = ctx->stat_mean_turn++ & 7;
  CMX_TRY(scratch(ctx, (what + std::to_string(turn)).c_str(), count, &p));
  ctx->param_host[turn].assign(v, v + count);
  HIP_TRY(ctx, hipMemcpyAsync(p, ctx->param_host[turn].data(), sizeof(double) * count, hipMemcpyHostToDevice, (hipStream_t)stream));
  *d = p;
  return CMX_OK;
}

// params: CorrectedCorrelation = the two mean vectors [2][B]; DiscreteMI = [threshold] (optional); DiscreteMI with bounds
// (DiscreteMutualInformationStatistic with a bounds vector, cmx_stat_mi.hip) = [nbounds, b_0 .. b_{nbounds-1}]
cmx_status resolve_stat(cmx_ctx* ctx, int kind, const double* params, void* stream, Stat* out) {
  Stat sk;
  sk.kind = kind; sk.B = ctx->hm.B; sk.K = ctx->hm.K;
  sk.gk = kind == CMX_STAT_CORRECTED_CORRELATION ? CMX_STAT_CORRELATION : kind;
  sk.d_w = stat_weights(ctx, kind);
  if (kind == CMX_STAT_DISCRETE_MI) sk.param = params ? params[0] : 0.99;
  if (kind == CMX_STAT_CORRECTED_CORRELATION) {
    if (!params) return fail(ctx, CMX_ERR_INVALID, "CorrectedCorrelation needs its mean vectors: params = [2][nbranches]");
    CMX_TRY(upload_params(ctx, "stat_mean", params, 2 * (size_t)sk.B, stream, &sk.d_mean));
  }
  if (sk.mi()) {
    if (!params) return fail(ctx, CMX_ERR_INVALID, "DiscreteMI with bounds: params = [nbounds, b_0 .. b_{nbounds-1}] is required");
    const double nbd = params[0];
    if (!(nbd >= 2.0) || nbd > 65535.0 || nbd != std::floor(nbd))
      return fail(ctx, CMX_ERR_INVALID, "DiscreteMI with bounds: the number of bounds must be an integer in 2 .. 65535");
    sk.nb = (int)nbd;
    for (int i = 0; i < sk.nb; ++i) {
      if (params[1 + i] != params[1 + i]) return fail(ctx, CMX_ERR_INVALID, "DiscreteMI with bounds: a bound is NaN");
      if (i && params[1 + i] < params[i])   // Domain::Domain(const Vdouble&) throws for decreasing bounds (Domain.cpp:62-72)
        return fail(ctx, CMX_ERR_INVALID, "DiscreteMI with bounds: bound " + std::to_string(i) + " is < to bound " + std::to_string(i - 1));
    }
    if (sk.B > 4096) return fail(ctx, CMX_ERR_UNSUPPORTED, "DiscreteMI with bounds: at most 4096 branches (the joint table of a pair lives in LDS)");
    CMX_TRY(upload_params(ctx, "mi_bounds", params + 1, (size_t)sk.nb, stream, &sk.d_bounds));
  }
  *out = sk;
  return CMX_OK;
}

cmx_status pair_operand(cmx_ctx* ctx, const Stat& sk, const double* d_counts, size_t n, size_t ldc, const char* slot, hipStream_t st,
                        PairOperand* out, size_t block) {
  PairOperand o;
  o.n = n;
  o.ldx = ((block ? block : n) + 15) / 16 * 16;
  if (sk.mi()) {
    CMX_TRY(scratch(ctx, (std::string("mi_cls_") + slot).c_str(), (size_t)sk.B * o.ldx, &o.cls));
    CMX_TRY(scratch(ctx, (std::string("mi_bad_") + slot).c_str(), n, &o.bad));
    HIP_TRY(ctx, launch_mi_classify(sk, d_counts, n, ldc, o, st));
  } else {
    const bool own = std::strcmp(slot, "gram") == 0, second = std::strcmp(slot, "2") == 0;
    const std::string pre = own ? "gram_" : "pair_", suf = own ? "1" : slot;
    CMX_TRY(scratch(ctx, (pre + "X" + suf).c_str(), pair_Bp(sk.B) * o.ldx * (block ? n / block : 1), &o.X));
    CMX_TRY(scratch(ctx, (pre + "s" + suf).c_str(), n, &o.s));
    CMX_TRY(scratch(ctx, (pre + "r" + suf).c_str(), n, &o.r));
    HIP_TRY(ctx, launch_pair_prep(sk, d_counts, n, ldc, sk.d_mean && second ? sk.d_mean + sk.B : sk.d_mean, block, o, st));
  }
  *out = o;
  return CMX_OK;
}

cmx_status pair_block(cmx_ctx* ctx, const Stat& sk, const PairOperand& a, size_t i0, size_t rb, const PairOperand& b, PairMode mode,
                      double* out, size_t ldo, hipStream_t st) {
  if (sk.mi()) HIP_TRY(ctx, launch_mi_pairs_block(sk.B, a.rows(i0, rb), b, mode, out, ldo, i0, st));
  else HIP_TRY(ctx, launch_pair_gram(sk, a.rows(i0, rb), b, mode, out, ldo, GramBatch{1, 0, 0, 0} /* one block of sites: no grid.z strides */,
                                     mode == kPairUpperRows ? i0 : 0, st));
  return CMX_OK;
}

cmx_status cmx_pair_stats_dev(cmx_ctx* ctx, int kind, const double* params, const double* d_counts1, size_t n1,
                              size_t ld1, const double* d_counts2, size_t n2, size_t ld2, double* d_out, size_t ldo,
                              void* stream) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_kind(ctx, kind));
  const bool intra = d_counts2 == nullptr;
  if (intra) { n2 = n1; ld2 = ld1; }
  if (!d_counts1 || !d_out || n1 == 0 || n2 == 0 || ld1 < n1 || ld2 < n2 || ldo < n2)
    return fail(ctx, CMX_ERR_INVALID, "cmx_pair_stats: bad arguments");
  if (ctx->hm.B < 2) return fail(ctx, CMX_ERR_INVALID, "cmx_pair_stats: need at least two branches");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  Stat sk;
  PairOperand a, b;
  CMX_TRY(resolve_stat(ctx, kind, params, stream, &sk));
  CMX_TRY(pair_operand(ctx, sk, d_counts1, n1, ld1, "1", st, &a));
  if (intra) b = a;
  else CMX_TRY(pair_operand(ctx, sk, d_counts2, n2, ld2, "2", st, &b));
  return pair_block(ctx, sk, a, 0, n1, b, intra ? kPairOneSet : kPairRectangle, d_out, ldo, st);
}

// AnalysisTools::compute*Matrix (AnalysisTools.cpp:102-339): the same operand preparation, Gram kernel and epilogues as
// the pair statistics, with the vector length as the "number of branches" and one "substitution type"
cmx_status cmx_vector_matrix(cmx_ctx* ctx, int kind, size_t dim, const double* v1, size_t n1, const double* v2, size_t n2,
                             int independent, double* out) {
  if (!ctx) return CMX_ERR_INVALID;
  if (kind != CMX_STAT_SCALAR_PRODUCT && kind != CMX_STAT_COSINUS && kind != CMX_STAT_CORRELATION && kind != CMX_STAT_COVARIANCE)
    return fail(ctx, CMX_ERR_INVALID, "cmx_vector_matrix: kind must be scalar product, cosinus, correlation or covariance");
  const bool one = v2 == nullptr;
  if (one) n2 = n1;
  if (!v1 || !out || n1 == 0 || n2 == 0 || dim == 0 || dim > 0x7fffffffull) return fail(ctx, CMX_ERR_INVALID, "cmx_vector_matrix: bad arguments");
  if (independent && (one || n1 != n2))
    return fail(ctx, CMX_ERR_INVALID, "cmx_vector_matrix: when performing independant comparisons, the two datasets must have the same length");
  if ((kind == CMX_STAT_CORRELATION || kind == CMX_STAT_COVARIANCE) && dim < 2)
    return fail(ctx, CMX_ERR_INVALID, "cmx_vector_matrix: correlation / covariance need vectors of at least two elements");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Stat sk;   // no parameters, no weights
  sk.kind = sk.gk = kind; sk.B = (int)dim; sk.K = 1;
  TmpDev tmp;
  double *d1 = nullptr, *d2 = nullptr, *d_out = nullptr;
  CMX_TRY(tmp.upload_branch_major(ctx, &d1, v1, n1, dim));
  if (!one) CMX_TRY(tmp.upload_branch_major(ctx, &d2, v2, n2, dim));
  else d2 = d1;
  if (independent) {   // AnalysisTools.cpp:150-157: j runs over i alone
    CMX_TRY(tmp.alloc(ctx, &d_out, n1));
    const PairOut diag{d_out};   // the statistic alone: no columns, no minima
    HIP_TRY(ctx, launch_pair_diag(sk, d1, n1, SiteCols{}, d2, n2, SiteCols{}, n1, diag, nullptr));
    std::vector<double> dg(n1);
    CMX_TRY(download(ctx, dg.data(), d_out, n1));
    std::fill(out, out + n1 * n2, 0.0);
    for (size_t i = 0; i < n1; ++i) out[i * n2 + i] = dg[i];
    return CMX_OK;
  }
  PairOperand a, b;
  CMX_TRY(pair_operand(ctx, sk, d1, n1, n1, "1", nullptr, &a));
  if (one) b = a;
  else CMX_TRY(pair_operand(ctx, sk, d2, n2, n2, "2", nullptr, &b));
  CMX_TRY(tmp.alloc(ctx, &d_out, n1 * n2));
  // the full rectangle (one-set form too: the reference fills both triangles and the diagonal)
  CMX_TRY(pair_block(ctx, sk, a, 0, n1, b, kPairRectangle, d_out, n2, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, out, d_out, n1 * n2));
  if (one) {
    // matrix[i][i] = 1 for cosinus / correlation (AnalysisTools.cpp:178, 236); the lower triangle mirrors the upper one
    // (matrix[i][j] = matrix[j][i] = f(v_i, v_j), j > i)
    for (size_t i = 0; i < n1; ++i) {
      if (kind == CMX_STAT_COSINUS || kind == CMX_STAT_CORRELATION) out[i * n1 + i] = 1.0;
      for (size_t j = 0; j < i; ++j) out[i * n1 + j] = out[j * n1 + i];
    }
  }
  return CMX_OK;
}

cmx_status cmx_pair_stats(cmx_ctx* ctx, int kind, const double* params, const double* counts1, size_t n1,
                          const double* counts2, size_t n2, double* out) {
  CMX_TRY(need_model(ctx));
  if (!counts1 || !out || n1 == 0 || (counts2 && n2 == 0)) return fail(ctx, CMX_ERR_INVALID, "cmx_pair_stats: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t BK = (size_t)ctx->hm.B * ctx->hm.K;
  if (!counts2) n2 = n1;
  TmpDev tmp;
  double *d1 = nullptr, *d2 = nullptr, *d_out = nullptr;
  CMX_TRY(tmp.upload_branch_major(ctx, &d1, counts1, n1, BK));
  if (counts2) CMX_TRY(tmp.upload_branch_major(ctx, &d2, counts2, n2, BK));
  CMX_TRY(tmp.alloc(ctx, &d_out, n1 * n2));
  CMX_TRY(cmx_pair_stats_dev(ctx, kind, params, d1, n1, n1, d2, n2, n2, d_out, n2, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  return download(ctx, out, d_out, n1 * n2);
}

// ------------------------------------------------------------------------------------------------ p-values
// The null distribution as the p-value kernel wants it (CoETools.cpp:636-652): Domain(0, max norm, nclasses) classes of
// the null pairs' min norms, every class sorted ascending, classes laid out one after the other; hist = class sizes.
static cmx_status prepare_null(cmx_ctx* ctx, const double* d_norms, size_t n, int nclasses, const double* d_null_stat,
                               const double* d_null_nmin, size_t nnull, hipStream_t st, NullTable* out) {
  double *maxnorm, *sa, *sb;
  uint32_t *ca, *cb, *hist, *bins;
  NullClass* cls;
  const size_t nn = nnull ? nnull : 1;
  CMX_TRY(scratch(ctx, "pv_max", 1, &maxnorm));
  CMX_TRY(scratch(ctx, "pv_sa", nn, &sa));
  CMX_TRY(scratch(ctx, "pv_sb", nn, &sb));
  CMX_TRY(scratch(ctx, "pv_ca", nn, &ca));
  CMX_TRY(scratch(ctx, "pv_cb", nn, &cb));
  CMX_TRY(scratch(ctx, "pv_hist", 66, &hist));
  CMX_TRY(scratch(ctx, "pv_cls", 66, &cls));
  CMX_TRY(scratch(ctx, "pv_bins", ((nn >> kNullBinShift) + 2 * 66), &bins));
  HIP_TRY(ctx, launch_max_reduce(d_norms, n, maxnorm, st));
  HIP_TRY(ctx, launch_null_classify(d_null_stat, d_null_nmin, nnull, maxnorm, nclasses, ca, hist, st));
  if (nnull > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(sa, d_null_stat, sizeof(double) * nnull, hipMemcpyDeviceToDevice, st));
    size_t tmp_bytes = 0;
    HIP_TRY(ctx, sort_null_by_class(nullptr, tmp_bytes, sa, sb, ca, cb, nnull, st));
    void* tmp;
    CMX_TRY(scratch(ctx, "pv_sorttmp", tmp_bytes, &tmp));
    HIP_TRY(ctx, sort_null_by_class(tmp, tmp_bytes, sa, sb, ca, cb, nnull, st));
  }
  HIP_TRY(ctx, launch_null_index(sa, hist, nclasses, nnull, cls, bins, st));
  *out = NullTable{sa, cls, bins, maxnorm, nclasses};
  return CMX_OK;
}

cmx_status cmx_intra_pvalues_dev(cmx_ctx* ctx, const double* d_stat, size_t ldo, const double* d_norms, size_t n,
                                 int nclasses, const double* d_null_stat, const double* d_null_nmin, size_t nnull,
                                 double* d_pvalue, int32_t* d_nsim, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!d_stat || !d_norms || !d_pvalue || !d_nsim || n == 0 || ldo < n || nclasses < 1 || nclasses > 64 ||
      (nnull > 0 && (!d_null_stat || !d_null_nmin)) || nnull > 0xfffffff0ull)
    return fail(ctx, CMX_ERR_INVALID, "cmx_intra_pvalues: bad arguments (nclasses must be in 1..64)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  NullTable nt;
  CMX_TRY(prepare_null(ctx, d_norms, n, nclasses, d_null_stat, d_null_nmin, nnull, st, &nt));
  HIP_TRY(ctx, launch_pvalues(d_stat, ldo, d_norms, n, nt, d_pvalue, d_nsim, 0, n, st));
  return CMX_OK;
}

cmx_status cmx_intra_pvalues(cmx_ctx* ctx, const double* stat, const double* norms, size_t n, int nclasses,
                             const double* null_stat, const double* null_nmin, size_t nnull, double* pvalue,
                             int32_t* nsim) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!stat || !norms || !pvalue || !nsim || n == 0) return fail(ctx, CMX_ERR_INVALID, "cmx_intra_pvalues: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  double *d_stat, *d_norms, *d_ns = nullptr, *d_nm = nullptr, *d_pv;
  int32_t* d_nsim;
  CMX_TRY(tmp.upload(ctx, &d_stat, stat, n * n));
  CMX_TRY(tmp.upload(ctx, &d_norms, norms, n));
  CMX_TRY(tmp.alloc(ctx, &d_pv, n * n));
  CMX_TRY(tmp.alloc(ctx, &d_nsim, n * n));
  if (nnull) {
    CMX_TRY(tmp.upload(ctx, &d_ns, null_stat, nnull));
    CMX_TRY(tmp.upload(ctx, &d_nm, null_nmin, nnull));
  }
  CMX_TRY(cmx_intra_pvalues_dev(ctx, d_stat, n, d_norms, n, nclasses, d_ns, d_nm, nnull, d_pv, d_nsim, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, pvalue, d_pv, n * n));
  return download(ctx, nsim, d_nsim, n * n);
}

// ------------------------------------------------------------------------------------------------ compacted rows
// The compaction of statistics into rows runs in two phases: without a temporary a row launcher only reports the size of the
// scan's.  rows(scan, i0, rb): an entry point's call of its launcher for the rows [i0, i0 + rb).  open() acquires "rows_count",
// makes the sizing call (rows [0, rb_max)) and acquires "rows_scan"; after that every call of the pass compacts a block.
template <class Launch>
struct RowPass {
  Launch rows;
  RowScan scan;
  cmx_status open(cmx_ctx* ctx, size_t count_words, size_t rb_max) {
    CMX_TRY(scratch(ctx, "rows_count", count_words, &scan.rowcount));
    HIP_TRY(ctx, rows(scan, 0, rb_max));
    return scratch(ctx, "rows_scan", scan.tmp_bytes ? scan.tmp_bytes : 16, &scan.tmp);
  }
  hipError_t operator()(size_t i0, size_t rb) { return rows(scan, i0, rb); }
};
template <class Launch>
static RowPass<Launch> row_pass(Launch rows) { return {rows, {}}; }

cmx_status cmx_intra_rows_dev(cmx_ctx* ctx, const double* d_stat, size_t ldo, const double* d_pvalue, const int32_t* d_nsim,
                              size_t n, const int32_t* d_rate_class, const double* d_post_rate, const double* d_norm,
                              const cmx_pair_filters* filters, cmx_pair_row* d_rows, size_t capacity, uint64_t* d_count,
                              void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!d_stat || n == 0 || ldo < n || !d_rate_class || !d_post_rate || !d_norm || !d_count || (capacity && !d_rows) ||
      n > 0x7fffffffull)
    return fail(ctx, CMX_ERR_INVALID, "cmx_intra_rows: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  cmx_pair_filters f{0, -1, 0.0, -1.0, 0.0};
  if (filters) f = *filters;
  const SiteCols cols{d_rate_class, d_post_rate, d_norm};
  auto rows = row_pass([&](RowScan& scan, size_t i0, size_t rb) {   // the whole matrix, the p-values given, nothing before its rows
    return launch_pair_rows(d_stat, ldo, d_pvalue, d_nsim, n, cols, f, scan, d_rows, capacity, reinterpret_cast<unsigned long long*>(d_count), i0,
                            rb, nullptr, nullptr, (hipStream_t)stream);
  });
  CMX_TRY(rows.open(ctx, n * kPairRowSegs + 1, n));
  HIP_TRY(ctx, rows(0, n));
  return CMX_OK;
}

// What cmx_intra_rows_range_dev and cmx_intra_compact_range_dev are given alike, in the order of their own parameter lists, and
// what both make of it before their row loops: the statistic, the operand of the Gram kernel for all n sites (both sides of
// every pair), the null index, the row block.
struct RowRange {
  int kind;
  const double *params, *d_counts;
  size_t n, ldc;
  const double *d_norm, *d_null_stat, *d_null_nmin;
  size_t nnull;
  int nclasses;
  size_t row_begin, row_end;
  Stat sk;
  PairOperand x;
  NullTable nt{};   // sorted == nullptr: no null given, as the row launchers read it
  size_t RB = 0;
};
// the checks of entry point `who`, in its order; outputs_ok: its own pointers
static cmx_status row_range_check(cmx_ctx* ctx, const std::string& who, const RowRange& r, bool outputs_ok) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_kind(ctx, r.kind));
  if (!r.d_counts || r.n == 0 || r.ldc < r.n || !r.d_norm || !outputs_ok || r.n > 0x7fffffffull || r.row_begin > r.row_end || r.row_end > r.n ||
      (r.d_null_stat && (!r.d_null_nmin || r.nclasses < 1 || r.nclasses > 64)) || r.nnull > 0xfffffff0ull)
    return fail(ctx, CMX_ERR_INVALID, who + ": bad arguments");
  if (ctx->hm.B < 2) return fail(ctx, CMX_ERR_INVALID, who + ": need at least two branches");
  if (r.kind == CMX_STAT_EUCLIDIAN_DISTANCE) return fail(ctx, CMX_ERR_UNSUPPORTED, who + ": EuclidianDistance is a distance, not a statistic");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return CMX_OK;
}
// kept: the Gram blocks are there already, no operand is prepared
static cmx_status row_range_prepare(cmx_ctx* ctx, RowRange& r, const double* kept, hipStream_t st) {
  CMX_TRY(resolve_stat(ctx, r.kind, r.params, st, &r.sk));
  if (!kept) CMX_TRY(pair_operand(ctx, r.sk, r.d_counts, r.n, r.ldc, "1", st, &r.x));
  if (r.d_null_stat) CMX_TRY(prepare_null(ctx, r.d_norm, r.n, r.nclasses, r.d_null_stat, r.d_null_nmin, r.nnull, st, &r.nt));
  r.RB = pair_row_block(r.n, r.row_end - r.row_begin);
  return CMX_OK;
}

// CoETools::computeIntraStats' pair loop (CoETools.cpp:672-724) for the rows [row_begin, row_end) of the upper triangle,
// a block of rows at a time: Gram block on the matrix cores -> p-values -> filters -> compaction.  No N x N matrix exists;
// the dense scratch is one row block (<= 256 MiB).  Ranks of a multi-GPU job call it with disjoint row ranges: rows come
// out in the reference's (i, j) order, so the ranks' outputs concatenate to the single-GPU output.
cmx_status cmx_intra_rows_range_dev(cmx_ctx* ctx, int kind, const double* params, const double* d_counts, size_t n, size_t ldc,
                                    const int32_t* d_rate_class, const double* d_post_rate, const double* d_norm,
                                    const double* d_null_stat, const double* d_null_nmin, size_t nnull, int nclasses,
                                    const cmx_pair_filters* filters, size_t row_begin, size_t row_end, cmx_pair_row* d_rows,
                                    size_t capacity, uint64_t* d_count, void* stream) {
  RowRange r{kind, params, d_counts, n, ldc, d_norm, d_null_stat, d_null_nmin, nnull, nclasses, row_begin, row_end};
  CMX_TRY(row_range_check(ctx, "cmx_intra_rows_range", r, d_rate_class && d_post_rate && d_count && !(capacity && !d_rows)));
  hipStream_t st = (hipStream_t)stream;
  cmx_pair_filters f{0, -1, 0.0, -1.0, 0.0};
  if (filters) f = *filters;
  HIP_TRY(ctx, hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
  if (row_begin == row_end) return CMX_OK;
  CMX_TRY(row_range_prepare(ctx, r, nullptr, st));
  // row blocks: dense scratch = the f64 statistic; the p-values are looked up by the pass that writes the rows, for the
  // pairs it writes, and every block's rows go behind those already counted
  double* blk_stat;
  unsigned long long* count = reinterpret_cast<unsigned long long*>(d_count);
  CMX_TRY(scratch(ctx, "blk_stat", r.RB * n, &blk_stat));
  const SiteCols cols{d_rate_class, d_post_rate, d_norm};
  auto rows = row_pass([&](RowScan& scan, size_t i0, size_t rb) {
    return launch_pair_rows(blk_stat, n, nullptr, nullptr, n, cols, f, scan, d_rows, capacity, count, i0, rb, scan.tmp ? count : nullptr,
                            &r.nt, st);
  });
  CMX_TRY(rows.open(ctx, r.RB * kPairRowSegs + 1, r.RB));
  for (size_t i0 = row_begin; i0 < row_end; i0 += r.RB) {
    const size_t rb = std::min(r.RB, row_end - i0);
    CMX_TRY(pair_block(ctx, r.sk, r.x, i0, rb, r.x, kPairUpperRows, blk_stat, n, st));
    HIP_TRY(ctx, rows(i0, rb));
  }
  return CMX_OK;
}

cmx_status cmx_intra_gram_prefetch_dev(cmx_ctx* ctx, int kind, const double* d_counts, size_t n, size_t ldc, size_t row_begin,
                                       size_t row_end, void* stream) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_kind(ctx, kind));
  if (!d_counts || n == 0 || ldc < n || n > 0x7fffffffull || row_begin > row_end || row_end > n)
    return fail(ctx, CMX_ERR_INVALID, "cmx_intra_gram_prefetch: bad arguments");
  ctx->gram_kept.valid = false;
  const HostModel& h = ctx->hm;
  const size_t rows = row_end - row_begin;
  // statistics with parameters (mean vectors, thresholds, bounds) and distances: left to the later call
  if (rows == 0 || h.B < 2 || kind == CMX_STAT_CORRECTED_CORRELATION || kind == CMX_STAT_DISCRETE_MI || kind == CMX_STAT_DISCRETE_MI_BOUNDS ||
      kind == CMX_STAT_EUCLIDIAN_DISTANCE)
    return CMX_OK;
  const size_t RB = pair_row_block(n, rows), nblk = (rows + RB - 1) / RB;
  if (nblk * RB * n * sizeof(double) > ((size_t)2 << 30)) return CMX_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  // (scratch of its own: the null's scoring may be using the pair loop's on another stream)
  Stat sk;
  PairOperand x;
  double* kept = nullptr;
  CMX_TRY(resolve_stat(ctx, kind, nullptr, stream, &sk));
  CMX_TRY(pair_operand(ctx, sk, d_counts, n, ldc, "gram", st, &x));
  CMX_TRY(scratch(ctx, "gram_kept", nblk * RB * n, &kept));
  for (size_t i0 = row_begin; i0 < row_end; i0 += RB)
    CMX_TRY(pair_block(ctx, sk, x, i0, std::min(RB, row_end - i0), x, kPairUpperRows, kept + (i0 - row_begin) * n, n, st));
  ctx->gram_kept = {true, kind, d_counts, n, ldc, row_begin, row_end, kept};
  return CMX_OK;
}

cmx_status cmx_intra_compact_range_dev(cmx_ctx* ctx, int kind, const double* params, const double* d_counts, size_t n, size_t ldc,
                                       const double* d_norm, const double* d_null_stat, const double* d_null_nmin, size_t nnull,
                                       int nclasses, size_t row_begin, size_t row_end, cmx_pair_compact* d_out, size_t capacity,
                                       void* stream) {
  // the pass after each Gram block writes the records at their arithmetic position (no filters: no counting pass, no scan);
  // the Gram blocks may be there already (cmx_intra_gram_prefetch_dev with these arguments): then only the record pass runs
  RowRange r{kind, params, d_counts, n, ldc, d_norm, d_null_stat, d_null_nmin, nnull, nclasses, row_begin, row_end};
  CMX_TRY(row_range_check(ctx, "cmx_intra_compact_range", r, !(capacity && !d_out)));
  hipStream_t st = (hipStream_t)stream;
  if (row_begin == row_end) return CMX_OK;
  const cmx_ctx::GramKept gk0 = ctx->gram_kept;
  ctx->gram_kept.valid = false;
  const double* kept = gk0.valid && gk0.kind == kind && gk0.counts == d_counts && gk0.n == n && gk0.ldc == ldc && gk0.row_begin == row_begin &&
                               gk0.row_end == row_end ? gk0.stat : nullptr;
  CMX_TRY(row_range_prepare(ctx, r, kept, st));
  double* blk_stat = nullptr;
  if (!kept) CMX_TRY(scratch(ctx, "blk_stat", r.RB * n, &blk_stat));
  for (size_t i0 = row_begin; i0 < row_end; i0 += r.RB) {
    const size_t rb = std::min(r.RB, row_end - i0);
    if (!kept) CMX_TRY(pair_block(ctx, r.sk, r.x, i0, rb, r.x, kPairUpperRows, blk_stat, n, st));
    HIP_TRY(ctx, launch_pair_compact(kept ? kept + (i0 - row_begin) * n : blk_stat, n, n, d_norm, &r.nt, d_out, capacity, st, i0, rb,
                                     row_begin));
  }
  return CMX_OK;
}

// cmx_intra_compact_range_dev with the window index of the context (cmx_window_null_dev) in the place of the class table: the
// same row blocks, Gram blocks (kept ones too) and positions; the record pass counts in the window of min(norm_i, norm_j)
cmx_status cmx_intra_window_range_dev(cmx_ctx* ctx, int kind, const double* params, const double* d_counts, size_t n, size_t ldc,
                                      const double* d_norm, int lower, size_t row_begin, size_t row_end, cmx_pair_window* d_out,
                                      size_t capacity, void* stream) {
  RowRange r{kind, params, d_counts, n, ldc, d_norm, nullptr, nullptr, 0, 0, row_begin, row_end};
  CMX_TRY(row_range_check(ctx, "cmx_intra_window_range", r, !(capacity && !d_out)));
  CMX_TRY(need_window(ctx, "cmx_intra_window_range"));
  hipStream_t st = (hipStream_t)stream;
  if (row_begin == row_end) return CMX_OK;
  const cmx_ctx::GramKept gk0 = ctx->gram_kept;
  ctx->gram_kept.valid = false;
  const double* kept = gk0.valid && gk0.kind == kind && gk0.counts == d_counts && gk0.n == n && gk0.ldc == ldc && gk0.row_begin == row_begin &&
                               gk0.row_end == row_end ? gk0.stat : nullptr;
  CMX_TRY(row_range_prepare(ctx, r, kept, st));
  uint32_t *lo, *hi;
  CMX_TRY(scratch(ctx, "win_site_lo", n, &lo));
  CMX_TRY(scratch(ctx, "win_site_hi", n, &hi));
  HIP_TRY(ctx, launch_window_site_bounds(ctx->window.ix, d_norm, n, lo, hi, st));
  double* blk_stat = nullptr;
  if (!kept) CMX_TRY(scratch(ctx, "blk_stat", r.RB * n, &blk_stat));
  for (size_t i0 = row_begin; i0 < row_end; i0 += r.RB) {
    const size_t rb = std::min(r.RB, row_end - i0);
    if (!kept) CMX_TRY(pair_block(ctx, r.sk, r.x, i0, rb, r.x, kPairUpperRows, blk_stat, n, st));
    HIP_TRY(ctx, launch_pair_window(kept ? kept + (i0 - row_begin) * n : blk_stat, n, n, d_norm, ctx->window.ix, lo, hi, lower, d_out, capacity, st,
                                    i0, rb, row_begin));
  }
  return CMX_OK;
}

cmx_status cmx_window_pvalues_from_records(size_t n, size_t row_begin, size_t row_end, const double* norm, const cmx_pair_window* records,
                                           size_t npairs, const cmx_window_params* params, double* pvalue) {
  if (!norm || !params || row_begin > row_end || row_end > n || n > 0x7fffffffull || (npairs && (!records || !pvalue))) return CMX_ERR_INVALID;
  if (npairs != (row_end - row_begin) * (n - 1) - (row_end * (row_end - 1) - row_begin * (row_begin - 1)) / 2) return CMX_ERR_INVALID;
  const cmx_pair_window* c = records;
  double* p = pvalue;
  for (size_t i = row_begin; i < row_end; ++i)
    for (size_t j = i + 1; j < n; ++j, ++c, ++p) {
      // the same rule and the same one IEEE division as window_test_kernel on the device
      const double m = norm[i] < norm[j] ? norm[i] : norm[j];
      *p = __builtin_nan("");
      if (m < params->conserved_nmin) *p = 1.0;
      else if (m == m && c->nobs >= params->min_nobs && c->count != 0xffffffffu) *p = (double)(c->count + 1u) / (double)(c->nobs + 1u);
    }
  return CMX_OK;
}

cmx_status cmx_expand_compact_rows(size_t n, size_t row_begin, size_t row_end, const int32_t* rate_class, const double* post_rate,
                                   const double* norm, const cmx_pair_compact* compact, size_t npairs, cmx_pair_row* rows, int nthreads) {
  if (!rate_class || !post_rate || !norm || row_begin > row_end || row_end > n || n > 0x7fffffffull || (npairs && (!compact || !rows)))
    return CMX_ERR_INVALID;
  auto prefix = [n, row_begin](size_t i) { return (i - row_begin) * (n - 1) - (i * (i - 1) - row_begin * (row_begin - 1)) / 2; };
  if (npairs != prefix(row_end)) return CMX_ERR_INVALID;
  auto expand = [&](size_t i_begin, size_t i_end) {
    for (size_t i = i_begin; i < i_end; ++i) {
      const cmx_pair_compact* c = compact + prefix(i);
      cmx_pair_row* r = rows + prefix(i);
      const int32_t ci = rate_class[i];
      const double ri = post_rate[i], ni = norm[i];
      for (size_t j = i + 1; j < n; ++j, ++c, ++r) {
        // the same expressions as pair_rows_kernel / null_pvalue on the device (one IEEE division: bit-identical)
        r->i = (int32_t)i; r->j = (int32_t)j; r->stat = c->stat;
        r->rc_min = ci < rate_class[j] ? ci : rate_class[j];
        r->pr_min = ri < post_rate[j] ? ri : post_rate[j];
        r->n_min = ni < norm[j] ? ni : norm[j];
        if (c->below == 0xffffffffu) { r->pvalue = __builtin_nan(""); r->nsim = 0; }
        else { r->pvalue = (double)(c->nsim - c->below + 1) / (double)(c->nsim + 1); r->nsim = (int32_t)c->nsim; }
      }
    }
  };
  const size_t nrow = row_end - row_begin;
  if (nthreads <= 1 || nrow < 2) { expand(row_begin, row_end); return CMX_OK; }
  // rows cut by pair count: thread t takes the rows whose prefix lies in [t, t + 1) * npairs / nthreads
  std::vector<std::thread> pool;
  size_t i0 = row_begin;
  for (int t = 0; t < nthreads; ++t) {
    const size_t target = (size_t)((unsigned long long)npairs * (t + 1) / nthreads);
    size_t i1 = i0;
    while (i1 < row_end && (t + 1 == nthreads || prefix(i1) < target)) ++i1;
    if (t + 1 == nthreads) i1 = row_end;
    if (i1 > i0) pool.emplace_back(expand, i0, i1);
    i0 = i1;
  }
  for (auto& th : pool) th.join();
  return CMX_OK;
}

cmx_status cmx_intra_rows(cmx_ctx* ctx, int kind, const double* params, const double* counts, size_t n,
                          const int32_t* rate_class, const double* post_rate, const double* norm, const double* null_stat,
                          const double* null_nmin, size_t nnull, int nclasses, const cmx_pair_filters* filters,
                          cmx_pair_row* rows, size_t capacity, uint64_t* count) {
  CMX_TRY(need_model(ctx));
  if (!counts || n == 0 || !rate_class || !post_rate || !norm || !count || (capacity && !rows) ||
      (null_stat && (!null_nmin || nclasses < 1)))
    return fail(ctx, CMX_ERR_INVALID, "cmx_intra_rows: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t BK = (size_t)ctx->hm.B * ctx->hm.K;
  TmpDev tmp;
  double *d_cnt, *d_stat, *d_pr, *d_nm, *d_pv = nullptr, *d_ns = nullptr, *d_nn = nullptr;
  int32_t *d_rc, *d_nsim = nullptr;
  cmx_pair_row* d_rows = nullptr;
  uint64_t* d_count;
  CMX_TRY(tmp.upload_branch_major(ctx, &d_cnt, counts, n, BK));
  CMX_TRY(tmp.alloc(ctx, &d_stat, n * n));
  CMX_TRY(tmp.upload(ctx, &d_pr, post_rate, n));
  CMX_TRY(tmp.upload(ctx, &d_nm, norm, n));
  CMX_TRY(tmp.upload(ctx, &d_rc, rate_class, n));
  CMX_TRY(tmp.alloc(ctx, &d_count, 1));
  if (capacity) CMX_TRY(tmp.alloc(ctx, &d_rows, capacity));
  CMX_TRY(cmx_pair_stats_dev(ctx, kind, params, d_cnt, n, n, nullptr, 0, 0, d_stat, n, nullptr));
  if (null_stat) {
    CMX_TRY(tmp.alloc(ctx, &d_pv, n * n));
    CMX_TRY(tmp.alloc(ctx, &d_nsim, n * n));
    if (nnull) {
      CMX_TRY(tmp.upload(ctx, &d_ns, null_stat, nnull));
      CMX_TRY(tmp.upload(ctx, &d_nn, null_nmin, nnull));
    }
    CMX_TRY(cmx_intra_pvalues_dev(ctx, d_stat, n, d_nm, n, nclasses, d_ns, d_nn, nnull, d_pv, d_nsim, nullptr));
  }
  CMX_TRY(cmx_intra_rows_dev(ctx, d_stat, n, d_pv, d_nsim, n, d_rc, d_pr, d_nm, filters, d_rows, capacity, d_count, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, count, d_count, 1));
  const size_t nw = std::min<size_t>((size_t)*count, capacity);
  if (nw) CMX_TRY(download(ctx, rows, d_rows, nw));
  return CMX_OK;
}

// ------------------------------------------------------------------------------------------------ inter-gene rows
cmx_status cmx_inter_rows_dev(cmx_ctx* ctx, int kind, const double* params, const double* d_counts1, size_t n1, size_t ld1,
                              const int32_t* d_rc1, const double* d_pr1, const double* d_nm1, const double* d_counts2, size_t n2,
                              size_t ld2, const int32_t* d_rc2, const double* d_pr2, const double* d_nm2,
                              const cmx_inter_filters* filters, cmx_pair_row* d_rows, size_t capacity, uint64_t* d_count, void* stream) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_kind(ctx, kind));
  if (!d_counts1 || !d_counts2 || n1 == 0 || n2 == 0 || ld1 < n1 || ld2 < n2 || !d_rc1 || !d_pr1 || !d_nm1 || !d_rc2 || !d_pr2 ||
      !d_nm2 || !d_count || (capacity && !d_rows) || n1 > 0x7fffffffull || n2 > 0x7fffffffull)
    return fail(ctx, CMX_ERR_INVALID, "cmx_inter_rows: bad arguments");
  if (kind == CMX_STAT_EUCLIDIAN_DISTANCE) return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_inter_rows: EuclidianDistance is a distance, not a statistic");
  cmx_inter_filters f{0, 0, -1, 0, 0.0, 0.0, -1.0, 0.0, 0, 0};
  if (filters) f = *filters;
  if (f.independent_comparisons && n1 != n2)   // CoETools.cpp:745-749
    return fail(ctx, CMX_ERR_INVALID, "When performing independant comparisons, the two datasets must have the same length.");
  const HostModel& h = ctx->hm;
  if (h.B < 2) return fail(ctx, CMX_ERR_INVALID, "cmx_inter_rows: need at least two branches");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(ctx, hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
  // the compaction of a block of statistics: [nrows][ldo], every block's rows behind those at *base
  unsigned long long* count = reinterpret_cast<unsigned long long*>(d_count);
  const SiteCols cols1{d_rc1, d_pr1, d_nm1}, cols2{d_rc2, d_pr2, d_nm2};
  auto inter_pass = [&](const double* stat, size_t ldo, const unsigned long long* base) {
    return row_pass([=, &f](RowScan& scan, size_t i0, size_t nrows) {
      return launch_inter_rows(stat, ldo, n2, cols1, cols2, f, scan, d_rows, capacity, count, i0, nrows, scan.tmp ? base : nullptr, st);
    });
  };
  double* dstat = nullptr;
  if (f.independent_comparisons) CMX_TRY(scratch(ctx, "inter_diag", n1, &dstat));
  Stat sk;
  PairOperand a, b;
  CMX_TRY(resolve_stat(ctx, kind, params, stream, &sk));
  if (f.independent_comparisons) {
    // the n1 pairs (i, i): statistic of the diagonal, then the same filters and compaction
    if (sk.mi()) {
      CMX_TRY(pair_operand(ctx, sk, d_counts1, n1, ld1, "1", st, &a));
      CMX_TRY(pair_operand(ctx, sk, d_counts2, n2, ld2, "2", st, &b));
      HIP_TRY(ctx, launch_mi_pairs_diag(h.B, a, b, n1, dstat, st));
    } else {
      const PairOut diag{dstat};   // the statistic alone: no columns, no minima
      HIP_TRY(ctx, launch_pair_diag(sk, d_counts1, ld1, SiteCols{}, d_counts2, ld2, SiteCols{}, n1, diag, st));
    }
    auto rows = inter_pass(dstat, 1, nullptr);
    CMX_TRY(rows.open(ctx, n1 + 1, n1));
    HIP_TRY(ctx, rows(0, n1));
    return CMX_OK;
  }
  // operands of both data sets once, then row blocks of data set 1 (dense scratch <= 256 MiB)
  CMX_TRY(pair_operand(ctx, sk, d_counts1, n1, ld1, "1", st, &a));
  CMX_TRY(pair_operand(ctx, sk, d_counts2, n2, ld2, "2", st, &b));
  const size_t RB = pair_row_block(n2, n1);
  double* blk;
  CMX_TRY(scratch(ctx, "blk_stat", RB * n2, &blk));
  auto rows = inter_pass(blk, n2, count);
  CMX_TRY(rows.open(ctx, RB + 1, RB));
  for (size_t i0 = 0; i0 < n1; i0 += RB) {
    const size_t rb = std::min(RB, n1 - i0);
    CMX_TRY(pair_block(ctx, sk, a, i0, rb, b, kPairRectangle, blk, n2, st));
    HIP_TRY(ctx, rows(i0, rb));
  }
  return CMX_OK;
}

cmx_status cmx_inter_rows(cmx_ctx* ctx, int kind, const double* params, const double* counts1, size_t n1, const int32_t* rate_class1,
                          const double* post_rate1, const double* norm1, const double* counts2, size_t n2, const int32_t* rate_class2,
                          const double* post_rate2, const double* norm2, const cmx_inter_filters* filters, cmx_pair_row* rows,
                          size_t capacity, uint64_t* count) {
  CMX_TRY(need_model(ctx));
  if (!counts1 || !counts2 || n1 == 0 || n2 == 0 || !rate_class1 || !post_rate1 || !norm1 || !rate_class2 || !post_rate2 || !norm2 ||
      !count || (capacity && !rows))
    return fail(ctx, CMX_ERR_INVALID, "cmx_inter_rows: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t BK = (size_t)ctx->hm.B * ctx->hm.K;
  TmpDev tmp;
  double *d_c[2], *d_pr[2], *d_nm[2];
  int32_t* d_rc[2];
  const double* cs[2] = {counts1, counts2};
  const size_t ns[2] = {n1, n2};
  const int32_t* rcs[2] = {rate_class1, rate_class2};
  const double *prs[2] = {post_rate1, post_rate2}, *nms[2] = {norm1, norm2};
  for (int q = 0; q < 2; ++q) {
    CMX_TRY(tmp.upload_branch_major(ctx, &d_c[q], cs[q], ns[q], BK));
    CMX_TRY(tmp.upload(ctx, &d_pr[q], prs[q], ns[q]));
    CMX_TRY(tmp.upload(ctx, &d_nm[q], nms[q], ns[q]));
    CMX_TRY(tmp.upload(ctx, &d_rc[q], rcs[q], ns[q]));
  }
  cmx_pair_row* d_rows = nullptr;
  uint64_t* d_count;
  CMX_TRY(tmp.alloc(ctx, &d_count, 1));
  if (capacity) CMX_TRY(tmp.alloc(ctx, &d_rows, capacity));
  CMX_TRY(cmx_inter_rows_dev(ctx, kind, params, d_c[0], n1, n1, d_rc[0], d_pr[0], d_nm[0], d_c[1], n2, n2, d_rc[1], d_pr[1], d_nm[1], filters, d_rows,
                             capacity, d_count, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, count, d_count, 1));
  const size_t nw = std::min<size_t>((size_t)*count, capacity);
  if (nw) CMX_TRY(download(ctx, rows, d_rows, nw));
  return CMX_OK;
}

// ------------------------------------------------------------------------------------------------ groups of sites
cmx_status cmx_group_stats_dev(cmx_ctx* ctx, int kind, const double* params, const double* d_counts, size_t n, size_t ldc,
                               const int64_t* d_offsets, const int32_t* d_sites, size_t ngroups, double* d_out, void* stream) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_kind(ctx, kind));
  if (!d_counts || n == 0 || ldc < n || !d_offsets || !d_sites || !d_out) return fail(ctx, CMX_ERR_INVALID, "cmx_group_stats: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Stat sk;
  CMX_TRY(resolve_stat(ctx, kind, params, stream, &sk));
  if (sk.mi()) {
    PairOperand g;
    CMX_TRY(pair_operand(ctx, sk, d_counts, n, ldc, "g", (hipStream_t)stream, &g));
    HIP_TRY(ctx, launch_mi_group(sk.B, g, d_offsets, d_sites, ngroups, d_out, (hipStream_t)stream));
    return CMX_OK;
  }
  HIP_TRY(ctx, launch_group_stats(sk, d_counts, ldc, d_offsets, d_sites, ngroups, d_out, (hipStream_t)stream));
  return CMX_OK;
}

static cmx_status check_groups(cmx_ctx* ctx, const int64_t* offsets, const int32_t* sites, size_t ngroups, size_t n) {
  if (offsets[0] != 0) return fail(ctx, CMX_ERR_INVALID, "groups: offsets[0] must be 0");
  for (size_t g = 0; g < ngroups; ++g)
    if (offsets[g + 1] < offsets[g]) return fail(ctx, CMX_ERR_INVALID, "groups: offsets must not decrease");
  if (sites)
    for (int64_t q = 0; q < offsets[ngroups]; ++q)
      if (sites[q] < 0 || (size_t)sites[q] >= n) return fail(ctx, CMX_ERR_INVALID, "groups: site index out of range");
  return CMX_OK;
}

cmx_status cmx_group_stats(cmx_ctx* ctx, int kind, const double* params, const double* counts, size_t n, const int64_t* offsets,
                           const int32_t* sites, size_t ngroups, double* out) {
  CMX_TRY(need_model(ctx));
  if (!counts || n == 0 || !offsets || !sites || !out) return fail(ctx, CMX_ERR_INVALID, "cmx_group_stats: bad arguments");
  if (ngroups == 0) return CMX_OK;
  CMX_TRY(check_groups(ctx, offsets, sites, ngroups, n));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t BK = (size_t)ctx->hm.B * ctx->hm.K;
  TmpDev tmp;
  double *d_c, *d_out;
  int64_t* d_off;
  int32_t* d_sites;
  CMX_TRY(tmp.upload_branch_major(ctx, &d_c, counts, n, BK));
  CMX_TRY(tmp.alloc(ctx, &d_out, ngroups));
  CMX_TRY(tmp.upload(ctx, &d_off, offsets, ngroups + 1));
  CMX_TRY(tmp.upload(ctx, &d_sites, sites, (size_t)offsets[ngroups]));
  CMX_TRY(cmx_group_stats_dev(ctx, kind, params, d_c, n, n, d_off, d_sites, ngroups, d_out, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  return download(ctx, out, d_out, ngroups);
}

namespace {
// The bookkeeping of CandidateGroupSet (CoMap/CoETools.h:139-300, CoETools.cpp:900-1038) on norms alone: which
// simulated site goes to which candidate site, and which pseudo-groups are thereby completed.  Whether a completed
// pseudo-group also counts for n1 needs its statistic -- evaluated afterwards for the whole batch on the device.
struct CandidateCursor {
  size_t G = 0;
  const int64_t* off = nullptr;
  const double *lo = nullptr, *hi = nullptr;
  const uint8_t* usable = nullptr;
  uint32_t min_sim = 0, completed = 0, n_usable = 0, trials = 0;
  size_t gpos = 0, spos = 0;                       // the reference's groupPos_ / sitePos_ (kept across batches)
  std::vector<uint32_t> n2;
  std::vector<std::vector<int32_t>> waiting;       // per candidate site: simulated sites not yet used, oldest first
  std::vector<size_t> head;                        // per candidate site: first unused entry of `waiting`
  std::vector<int64_t> pg_off;                     // completed pseudo-groups of the current batch
  std::vector<int32_t> pg_sites, pg_group;

  size_t gsize(size_t g) const { return (size_t)(off[g + 1] - off[g]); }
  // 0, or what is wrong with the groups: 1 an analysable group is empty, 2 no analysable group
  int init(size_t ngroups, const int64_t* offsets, const double* norm_lo, const double* norm_hi, const uint8_t* analysable, uint32_t min) {
    G = ngroups; off = offsets; lo = norm_lo; hi = norm_hi; usable = analysable; min_sim = min;
    n2.assign(ngroups, 0);
    waiting.resize((size_t)offsets[ngroups]);
    head.assign((size_t)offsets[ngroups], 0);
    for (size_t g = 0; g < ngroups; ++g)
      if (analysable[g]) { if (gsize(g) == 0) return 1; ++n_usable; }
    return n_usable == 0 ? 2 : 0;
  }
  bool open(size_t g) const { return n2[g] < min_sim && usable[g]; }
  // nextCandidateSite: step to the next site of the current group (or the next group), then skip groups that are
  // complete or not analysable.  false: no group is left (the reference throws)
  bool advance() {
    if (n2[gpos] < min_sim && ++spos >= gsize(gpos)) { gpos = (gpos + 1) % G; spos = 0; }
    if (!open(gpos)) {
      const size_t start = gpos;
      do {
        gpos = (gpos + 1) % G;
        if (gpos == start) return false;
      } while (!open(gpos));
      spos = 0;
    }
    return true;
  }
  // addSimulatedSite: true if the group now has one simulated site for each of its members
  bool give(size_t g, size_t sidx, int32_t sim) {
    waiting[off[g] + sidx].push_back(sim);
    for (size_t q = off[g]; q < (size_t)off[g + 1]; ++q)
      if (head[q] >= waiting[q].size()) return false;
    for (size_t q = off[g]; q < (size_t)off[g + 1]; ++q) pg_sites.push_back(waiting[q][head[q]++]);
    pg_off.push_back((int64_t)pg_sites.size());
    pg_group.push_back((int32_t)g);
    if (++n2[g] == min_sim) ++completed;
    return true;
  }
  // analyseSimulations: 1 more batches needed, 0 done, -1 cursor error
  int batch(const double* norms, size_t nsim) {
    pg_off.assign(1, 0); pg_sites.clear(); pg_group.clear();
    bool more = true, nothing = true;
    for (size_t i = 0; more && i < nsim; ++i) {
      bool first = true, hit = false;
      size_t g0 = 0, s0 = 0;
      while (more && !hit) {
        if (!advance()) return -1;
        if (first) { g0 = gpos; s0 = spos; first = false; }
        else if (gpos == g0 && spos == s0) break;              // went round the whole set: this site fits nowhere
        const size_t q = off[gpos] + spos;
        hit = norms[i] >= lo[q] && norms[i] <= hi[q];
        if (hit) {
          if (give(gpos, spos, (int32_t)i)) nothing = false;
          if (completed == n_usable) more = false;
        }
      }
    }
    if (nothing) ++trials;
    for (size_t q = 0; q < waiting.size(); ++q) { waiting[q].clear(); head[q] = 0; }   // resetSimulations
    return more ? 1 : 0;
  }
};
}  // namespace

// host-side only (no GPU): run the candidate cursor over caller-supplied norms, batch by batch, and list the
// pseudo-groups it assembles.  For tests of the bookkeeping.
cmx_status cmx_debug_candidate_cursor(size_t ngroups, const int64_t* offsets, const double* norm_lo, const double* norm_hi,
                                      const uint8_t* analysable, uint32_t min_sim, const double* norms, size_t rep_ram,
                                      size_t nbatches, uint32_t max_trials, uint32_t* n2, uint32_t* trials,
                                      uint64_t* batches_used, int32_t* pg_group, int32_t* pg_batch, int64_t* pg_offsets,
                                      int32_t* pg_sites, size_t cap_groups, size_t cap_sites, size_t* npg) {
  if (ngroups == 0 || !offsets || !norm_lo || !norm_hi || !analysable || min_sim == 0 || !norms || rep_ram == 0 || !n2 || !npg)
    return CMX_ERR_INVALID;
  CandidateCursor cur;
  if (cur.init(ngroups, offsets, norm_lo, norm_hi, analysable, min_sim)) return CMX_ERR_INVALID;
  size_t ng = 0, ns = 0;
  uint64_t nb = 0;
  int more = 1;
  if (pg_offsets && cap_groups) pg_offsets[0] = 0;
  while (more == 1 && cur.trials < max_trials && nb < nbatches) {
    more = cur.batch(norms + nb * rep_ram, rep_ram);
    if (more < 0) return CMX_ERR_INVALID;
    for (size_t q = 0; q < cur.pg_group.size(); ++q, ++ng) {
      const size_t m = (size_t)(cur.pg_off[q + 1] - cur.pg_off[q]);
      if (ng < cap_groups && ns + m <= cap_sites) {
        pg_group[ng] = cur.pg_group[q];
        pg_batch[ng] = (int32_t)nb;
        for (size_t e = 0; e < m; ++e) pg_sites[ns + e] = cur.pg_sites[cur.pg_off[q] + e];
        pg_offsets[ng + 1] = (int64_t)(ns + m);
      }
      ns += m;
    }
    ++nb;
  }
  std::copy(cur.n2.begin(), cur.n2.end(), n2);
  if (trials) *trials = cur.trials;
  if (batches_used) *batches_used = nb;
  *npg = ng;
  return CMX_OK;
}

cmx_status cmx_candidate_groups(cmx_ctx* ctx, int kind, const double* params, size_t ngroups, const int64_t* offsets,
                                const double* norm_lo, const double* norm_hi, const uint8_t* analysable,
                                const double* observed, uint32_t min_sim, size_t rep_ram, uint32_t max_trials,
                                uint64_t max_batches, uint64_t seed, uint32_t* n1, uint32_t* n2, uint32_t* trials,
                                uint64_t* batches) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_kind(ctx, kind));
  if (ngroups == 0 || !offsets || !norm_lo || !norm_hi || !analysable || !observed || min_sim == 0 || rep_ram == 0 || !n1 || !n2)
    return fail(ctx, CMX_ERR_INVALID, "cmx_candidate_groups: bad arguments");
  CMX_TRY(check_groups(ctx, offsets, nullptr, ngroups, 0));
  CandidateCursor cur;
  if (const int bad = cur.init(ngroups, offsets, norm_lo, norm_hi, analysable, min_sim))
    return fail(ctx, CMX_ERR_INVALID, bad == 1 ? "cmx_candidate_groups: an analysable group is empty" : "cmx_candidate_groups: no analysable group");
  std::fill(n1, n1 + ngroups, 0u);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HostModel& h = ctx->hm;
  // The device works ahead of the cursor: a round simulates and maps several batches in one launch, the cursor then
  // consumes them batch by batch exactly as the reference would (batches it does not get to are discarded), and the
  // statistics of all pseudo-groups of the round are evaluated in one launch.
  const size_t BK = (size_t)h.B * h.K;
  const size_t round_batches = std::max<size_t>(1, std::min<size_t>(32, 32768 / rep_ram));
  const size_t N = round_batches * rep_ram;
  uint8_t *d_aln, *d_states;
  int32_t *d_cls, *d_pgs;
  int64_t* d_pgo;
  double *d_cnt, *d_norm, *d_st;
  CMX_TRY(scratch(ctx, "cg_aln", (size_t)h.T * N, &d_aln));
  CMX_TRY(scratch(ctx, "cg_states", (size_t)h.nn * N, &d_states));
  CMX_TRY(scratch(ctx, "cg_cls", N, &d_cls));
  CMX_TRY(scratch(ctx, "cg_cnt", BK * N, &d_cnt));
  CMX_TRY(scratch(ctx, "cg_norm", N, &d_norm));
  CMX_TRY(scratch(ctx, "cg_pgs", N, &d_pgs));
  CMX_TRY(scratch(ctx, "cg_pgo", (N + 1), &d_pgo));
  CMX_TRY(scratch(ctx, "cg_stat", N, &d_st));
  std::vector<double> norms(N), stats(N);
  std::vector<int64_t> r_off;
  std::vector<int32_t> r_sites, r_group;
  uint64_t nb = 0;
  int more = 1;
  auto go_on = [&]() { return more == 1 && cur.trials < max_trials && (max_batches == 0 || nb < max_batches); };
  while (go_on()) {
    HIP_TRY(ctx, launch_simulate(ctx->dm, seed, nb * (uint64_t)rep_ram, N, d_aln, N, d_cls, d_states, nullptr));
    CMX_TRY(map_sites_impl(ctx, d_aln, N, N, nullptr, d_cnt, N, nullptr, nullptr, nullptr, d_norm, nullptr, true));
    CMX_TRY(download(ctx, norms.data(), d_norm, N));
    r_off.assign(1, 0); r_sites.clear(); r_group.clear();
    for (size_t t = 0; t < round_batches && go_on(); ++t) {
      ++nb;
      more = cur.batch(norms.data() + t * rep_ram, rep_ram);
      if (more < 0) return fail(ctx, CMX_ERR_INVALID, "cmx_candidate_groups: candidate cursor found no open group");
      for (size_t q = 0; q < cur.pg_group.size(); ++q) {
        for (int64_t e = cur.pg_off[q]; e < cur.pg_off[q + 1]; ++e) r_sites.push_back((int32_t)(t * rep_ram) + cur.pg_sites[e]);
        r_off.push_back((int64_t)r_sites.size());
        r_group.push_back(cur.pg_group[q]);
      }
    }
    const size_t npg = r_group.size();
    if (npg) {
      HIP_TRY(ctx, hipMemcpy(d_pgo, r_off.data(), sizeof(int64_t) * (npg + 1), hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(d_pgs, r_sites.data(), sizeof(int32_t) * r_sites.size(), hipMemcpyHostToDevice));
      CMX_TRY(cmx_group_stats_dev(ctx, kind, params, d_cnt, N, N, d_pgo, d_pgs, npg, d_st, nullptr));
      CMX_TRY(download(ctx, stats.data(), d_st, npg));
      for (size_t q = 0; q < npg; ++q)
        if (stats[q] >= observed[r_group[q]]) ++n1[r_group[q]];
    }
  }
  std::copy(cur.n2.begin(), cur.n2.end(), n2);
  if (trials) *trials = cur.trials;
  if (batches) *batches = nb;
  return CMX_OK;
}

