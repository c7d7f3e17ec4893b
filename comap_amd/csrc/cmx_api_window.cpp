// C-ABI, sliding-window conditional p-values (R/CoMapFunctions.R:168-215): the index of a null, kept in the context,
// and the array form of its queries.  The pair loop against the index (cmx_intra_window_range_dev) and the host-side p-values
// of its records stand beside their siblings in cmx_api_pairs.cpp.
#include "cmx_ctx.h"

cmx_status cmx_window_null_dev(cmx_ctx* ctx, const double* d_null_stat, const double* d_null_nmin, size_t nnull, double window, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!(window > 0.0) || std::isinf(window))
    return fail(ctx, CMX_ERR_INVALID, "cmx_window_null: the window must be a fraction in (0, +inf)");
  if ((nnull > 0 && (!d_null_stat || !d_null_nmin)) || nnull > 0xfffffffeull) return fail(ctx, CMX_ERR_INVALID, "cmx_window_null: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  ctx->window.built = false;
  const size_t n = nnull, nn = n ? n : 1, units = window_units(n);
  const int L = window_levels(n);
  double *nmin, *stat;
  uint2* levels;
  uint32_t* zeros;
  WindowHead* head;
  CMX_TRY(scratch(ctx, "win_nmin", nn, &nmin));
  CMX_TRY(scratch(ctx, "win_stat", nn, &stat));
  CMX_TRY(scratch(ctx, "win_levels", (size_t)L * units, &levels));
  CMX_TRY(scratch(ctx, "win_zeros", (size_t)L, &zeros));
  CMX_TRY(scratch(ctx, "win_head", 1, &head));
  if (n == 0) {   // nothing to index: nkept = 0, every query gets nobs = 0
    const WindowHead empty{0, 0, 0.0, __builtin_nan(""), __builtin_nan("")};
    static_assert(sizeof(WindowHead) == 32, "uploaded as four words");
    HIP_TRY(ctx, hipMemcpyAsync(head, &empty, sizeof empty, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));   // (the source is on this frame)
  } else {
    WindowBuild b{};
    CMX_TRY(scratch(ctx, "win_key_a", n, &b.key_a));
    CMX_TRY(scratch(ctx, "win_key_b", n, &b.key_b));
    CMX_TRY(scratch(ctx, "win_val_a", n, &b.val_a));
    CMX_TRY(scratch(ctx, "win_val_b", n, &b.val_b));
    CMX_TRY(scratch(ctx, "win_seq_a", n, &b.seq_a));
    CMX_TRY(scratch(ctx, "win_seq_b", n, &b.seq_b));
    CMX_TRY(scratch(ctx, "win_cnt", units, &b.cnt));
    CMX_TRY(scratch(ctx, "win_ones", units, &b.ones));
    HIP_TRY(ctx, launch_window_build(d_null_stat, d_null_nmin, n, window, b, nmin, stat, levels, zeros, head, st));   // sizes rocPRIM's temporary
    CMX_TRY(scratch(ctx, "win_tmp", b.tmp_bytes ? b.tmp_bytes : 16, &b.tmp));
    HIP_TRY(ctx, launch_window_build(d_null_stat, d_null_nmin, n, window, b, nmin, stat, levels, zeros, head, st));
  }
  ctx->window.ix = WindowIndex{nmin, stat, levels, zeros, head, (uint32_t)n, (uint32_t)units, L};
  ctx->window.built = true;
  return CMX_OK;
}

cmx_status cmx_window_null_info(cmx_ctx* ctx, size_t* nkept, double* ws, double* nmin_min, double* nmin_max) {
  CMX_TRY(need_window(ctx, "cmx_window_null_info"));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  WindowHead h;
  CMX_TRY(download(ctx, &h, ctx->window.ix.head, 1));
  if (nkept) *nkept = h.nkept;
  if (ws) *ws = h.ws;
  if (nmin_min) *nmin_min = h.nmin_min;
  if (nmin_max) *nmin_max = h.nmin_max;
  return CMX_OK;
}

cmx_status cmx_window_test_dev(cmx_ctx* ctx, const double* d_stat, const double* d_nmin, size_t nq, const cmx_window_params* params,
                               double* d_pvalue, uint32_t* d_count, uint32_t* d_nobs, void* stream) {
  CMX_TRY(need_window(ctx, "cmx_window_test"));
  if (!params || (nq > 0 && (!d_stat || !d_nmin))) return fail(ctx, CMX_ERR_INVALID, "cmx_window_test: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, launch_window_test(ctx->window.ix, d_stat, d_nmin, nq, *params, d_pvalue, d_count, d_nobs, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_window_test(cmx_ctx* ctx, const double* null_stat, const double* null_nmin, size_t nnull, const double* stat, const double* nmin,
                           size_t nq, const cmx_window_params* params, double* pvalue, uint32_t* count, uint32_t* nobs) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!params || (nnull > 0 && (!null_stat || !null_nmin)) || (nq > 0 && (!stat || !nmin))) return fail(ctx, CMX_ERR_INVALID, "cmx_window_test: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  double *d_ns = nullptr, *d_nm = nullptr, *d_s = nullptr, *d_m = nullptr, *d_pv = nullptr;
  uint32_t *d_c = nullptr, *d_no = nullptr;
  if (nnull) {
    CMX_TRY(tmp.upload(ctx, &d_ns, null_stat, nnull));
    CMX_TRY(tmp.upload(ctx, &d_nm, null_nmin, nnull));
  }
  CMX_TRY(cmx_window_null_dev(ctx, d_ns, d_nm, nnull, params->window, nullptr));
  if (nq) {
    CMX_TRY(tmp.upload(ctx, &d_s, stat, nq));
    CMX_TRY(tmp.upload(ctx, &d_m, nmin, nq));
    CMX_TRY(tmp.alloc(ctx, &d_pv, nq));
    CMX_TRY(tmp.alloc(ctx, &d_c, nq));
    CMX_TRY(tmp.alloc(ctx, &d_no, nq));
  }
  CMX_TRY(cmx_window_test_dev(ctx, d_s, d_m, nq, params, d_pv, d_c, d_no, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (nq == 0) return CMX_OK;
  CMX_TRY(download(ctx, pvalue, d_pv, nq));
  CMX_TRY(download(ctx, count, d_c, nq));
  return download(ctx, nobs, d_no, nq);
}
