// C-ABI, clustering stage: agglomeration of a distance matrix, clustering of mapped sites, the clustering null.
#include "cmx_ctx.h"

extern "C" {

static cmx_status check_cluster(cmx_ctx* ctx, int dist_kind, int linkage, size_t n) {
  if (dist_kind < CMX_DIST_CORRELATION || dist_kind > CMX_DIST_EUCLIDIAN) return fail(ctx, CMX_ERR_INVALID, "unknown clustering distance");
  if (linkage < CMX_LINK_COMPLETE || linkage > CMX_LINK_AVERAGE) return fail(ctx, CMX_ERR_INVALID, "unknown clustering method");
  if (n < 2) return fail(ctx, CMX_ERR_INVALID, "clustering needs at least two sites");
  if (n > CMX_CLUSTER_MAX_SITES)
    return fail(ctx, CMX_ERR_UNSUPPORTED, "clustering is limited to " + std::to_string(CMX_CLUSTER_MAX_SITES) + " sites per matrix");
  return CMX_OK;
}

cmx_status cmx_hclust_dev(cmx_ctx* ctx, int linkage, double* d_dist, size_t n, size_t ld, size_t batch, int32_t* d_merge,
                          double* d_dmax, int32_t* d_size, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  CMX_TRY(check_cluster(ctx, CMX_DIST_CORRELATION, linkage, n));
  if (!d_dist || ld < n || batch == 0 || !d_merge || !d_dmax || !d_size) return fail(ctx, CMX_ERR_INVALID, "cmx_hclust: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  double* rmin;
  int* nn;
  CMX_TRY(scratch(ctx, "hc_rmin", batch * n, &rmin));
  CMX_TRY(scratch(ctx, "hc_nn", batch * n, &nn));
  HIP_TRY(ctx, launch_hclust(linkage, d_dist, n, ld, n * ld, batch, rmin, nn, d_merge, d_dmax, d_size, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_hclust(cmx_ctx* ctx, int linkage, const double* dist, size_t n, size_t batch, int32_t* merge, double* dmax,
                      int32_t* size) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!dist || !merge || !dmax || !size || batch == 0) return fail(ctx, CMX_ERR_INVALID, "cmx_hclust: bad arguments");
  CMX_TRY(check_cluster(ctx, CMX_DIST_CORRELATION, linkage, n));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  double *d_D, *d_dm;
  int32_t *d_mg, *d_sz;
  const size_t nm = batch * (n - 1);
  CMX_TRY(tmp.upload(ctx, &d_D, dist, batch * n * n));
  CMX_TRY(tmp.alloc(ctx, &d_dm, nm));
  CMX_TRY(tmp.alloc(ctx, &d_mg, 2 * nm));
  CMX_TRY(tmp.alloc(ctx, &d_sz, nm));
  CMX_TRY(cmx_hclust_dev(ctx, linkage, d_D, n, n, batch, d_mg, d_dm, d_sz, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, merge, d_mg, 2 * nm));
  CMX_TRY(download(ctx, dmax, d_dm, nm));
  return download(ctx, size, d_sz, nm);
}

// `batch` replicates of n sites each in consecutive column blocks of d_counts / d_norm: statistic (upper triangles) ->
// distances -> agglomeration -> group properties.  d_dist_out (batch == 1 only): copy of the distance matrix.
static cmx_status cluster_batch_dev(cmx_ctx* ctx, int dist_kind, int linkage, const double* d_counts, size_t ldc, size_t n,
                                    size_t batch, const double* d_norm, double* d_dist_out, int32_t* d_merge, double* d_dmax,
                                    int32_t* d_size, double* d_stat, double* d_nmin, hipStream_t st) {
  const HostModel& h = ctx->hm;
  double *D, *sigma = nullptr;
  CMX_TRY(scratch(ctx, "cl_D", batch * n * n, &D));
  const int stat_kind = dist_kind == CMX_DIST_CORRELATION ? CMX_STAT_CORRELATION
                        : dist_kind == CMX_DIST_COMPENSATION ? CMX_STAT_COMPENSATION : CMX_STAT_EUCLIDIAN_DISTANCE;
  // one operand preparation over all batch * n sites (an operand block per replicate), one Gram launch with a replicate per
  // grid.z slice.  (The tree's "Stat" property below stays unweighted, Distance.h:403-421.)
  Stat sk;
  PairOperand x;
  CMX_TRY(resolve_stat(ctx, stat_kind, nullptr, st, &sk));
  CMX_TRY(pair_operand(ctx, sk, d_counts, batch * n, ldc, "1", st, &x, n));
  const PairOperand rep = x.rows(0, n);   // the first replicate; the others follow at the batch's strides
  HIP_TRY(ctx, launch_pair_gram(sk, rep, rep, kPairUpperRows, D, n, GramBatch{batch, n, n * n, (size_t)pair_Bp(h.B) * x.ldx}, 0, st));
  HIP_TRY(ctx, launch_dist_finish(dist_kind, D, n, n, n * n, batch, st));
  if (d_dist_out) HIP_TRY(ctx, hipMemcpyAsync(d_dist_out, D, sizeof(double) * n * n, hipMemcpyDeviceToDevice, st));
  CMX_TRY(cmx_hclust_dev(ctx, linkage, D, n, n, batch, d_merge, d_dmax, d_size, st));
  if (dist_kind == CMX_DIST_COMPENSATION) CMX_TRY(scratch(ctx, "cl_sigma", batch * (2 * n - 1) * h.B, &sigma));
  HIP_TRY(ctx, launch_cluster_props(dist_kind, (int)n, h.B, h.K, batch, d_merge, d_dmax, d_norm, d_counts, ldc, n, sigma, d_stat,
                                    d_nmin, st));
  return CMX_OK;
}

cmx_status cmx_cluster_sites_dev(cmx_ctx* ctx, int dist_kind, int linkage, const double* d_counts, size_t n, size_t ldc,
                                 const double* d_norm, double* d_dist_out, int32_t* d_merge, double* d_dmax, int32_t* d_size,
                                 double* d_stat, double* d_nmin, void* stream) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_cluster(ctx, dist_kind, linkage, n));
  if (!d_counts || ldc < n || !d_norm || !d_merge || !d_dmax || !d_size || !d_stat || !d_nmin)
    return fail(ctx, CMX_ERR_INVALID, "cmx_cluster_sites: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cluster_batch_dev(ctx, dist_kind, linkage, d_counts, ldc, n, 1, d_norm, d_dist_out, d_merge, d_dmax, d_size, d_stat,
                           d_nmin, (hipStream_t)stream);
}

cmx_status cmx_cluster_sites(cmx_ctx* ctx, int dist_kind, int linkage, const double* counts, size_t n, double* dist_out,
                             int32_t* merge, double* dmax, int32_t* size, double* stat, double* nmin) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_cluster(ctx, dist_kind, linkage, n));
  if (!counts || !merge || !dmax || !size || !stat || !nmin) return fail(ctx, CMX_ERR_INVALID, "cmx_cluster_sites: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HostModel& h = ctx->hm;
  const size_t BK = (size_t)h.B * h.K, nm = n - 1;
  std::vector<double> norm(n);
  for (size_t i = 0; i < n; ++i) {       // computeNormForSite: sqrt(sum_b (sum_k n_bk)^2)
    double q = 0.0;
    for (int b = 0; b < h.B; ++b) {
      double t = 0.0;
      for (int k = 0; k < h.K; ++k) t += counts[i * BK + (size_t)b * h.K + k];
      q += t * t;
    }
    norm[i] = std::sqrt(q);
  }
  TmpDev tmp;
  double *d_c, *d_norm, *d_dist = nullptr, *d_dm, *d_st, *d_nmn;
  int32_t *d_mg, *d_sz;
  CMX_TRY(tmp.upload_branch_major(ctx, &d_c, counts, n, BK));
  CMX_TRY(tmp.upload(ctx, &d_norm, norm.data(), n));
  if (dist_out) CMX_TRY(tmp.alloc(ctx, &d_dist, n * n));
  CMX_TRY(tmp.alloc(ctx, &d_dm, nm));
  CMX_TRY(tmp.alloc(ctx, &d_st, nm));
  CMX_TRY(tmp.alloc(ctx, &d_nmn, nm));
  CMX_TRY(tmp.alloc(ctx, &d_mg, 2 * nm));
  CMX_TRY(tmp.alloc(ctx, &d_sz, nm));
  CMX_TRY(cmx_cluster_sites_dev(ctx, dist_kind, linkage, d_c, n, n, d_norm, d_dist, d_mg, d_dm, d_sz, d_st, d_nmn, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, dist_out, d_dist, n * n));
  CMX_TRY(download(ctx, merge, d_mg, 2 * nm));
  CMX_TRY(download(ctx, dmax, d_dm, nm));
  CMX_TRY(download(ctx, size, d_sz, nm));
  CMX_TRY(download(ctx, stat, d_st, nm));
  return download(ctx, nmin, d_nmn, nm);
}

cmx_status cmx_cluster_null(cmx_ctx* ctx, int dist_kind, int linkage, uint64_t seed, size_t rep_begin, size_t rep_end,
                            size_t nsites, int32_t* merge, double* dmax, int32_t* size, double* stat, double* nmin) {
  CMX_TRY(need_model(ctx));
  CMX_TRY(check_cluster(ctx, dist_kind, linkage, nsites));
  if (rep_end <= rep_begin || !merge || !dmax || !size || !stat || !nmin) return fail(ctx, CMX_ERR_INVALID, "cmx_cluster_null: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HostModel& h = ctx->hm;
  const size_t n = nsites, nm = n - 1, nrep = rep_end - rep_begin, BK = (size_t)h.B * h.K;
  // replicates per batch: every replicate keeps its own n x n matrix in HBM; 16 GiB of them at most
  const size_t per_rep = sizeof(double) * (n * n + BK * n) + (size_t)(h.T + h.nn) * n;
  const size_t R = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(nrep, 1024), ((size_t)16 << 30) / per_rep));
  const size_t N = R * n;
  uint8_t *d_aln, *d_states;
  int32_t *d_cls, *d_mg, *d_sz;
  double *d_cnt, *d_norm, *d_dm, *d_st, *d_nmn;
  CMX_TRY(scratch(ctx, "cl_aln", (size_t)h.T * N, &d_aln));
  CMX_TRY(scratch(ctx, "cl_states", (size_t)h.nn * N, &d_states));
  CMX_TRY(scratch(ctx, "cl_cls", N, &d_cls));
  CMX_TRY(scratch(ctx, "cl_cnt", BK * N, &d_cnt));
  CMX_TRY(scratch(ctx, "cl_norm", N, &d_norm));
  CMX_TRY(scratch(ctx, "cl_merge", 2 * R * nm, &d_mg));
  CMX_TRY(scratch(ctx, "cl_size", R * nm, &d_sz));
  CMX_TRY(scratch(ctx, "cl_dmax", R * nm, &d_dm));
  CMX_TRY(scratch(ctx, "cl_stat", R * nm, &d_st));
  CMX_TRY(scratch(ctx, "cl_nmin", R * nm, &d_nmn));
  for (size_t r0 = 0; r0 < nrep; r0 += R) {
    const size_t rb = std::min(R, nrep - r0), nb = rb * n;
    HIP_TRY(ctx, launch_simulate(ctx->dm, seed, (uint64_t)(rep_begin + r0) * n, nb, d_aln, nb, d_cls, d_states, nullptr));
    CMX_TRY(map_sites_impl(ctx, d_aln, nb, nb, nullptr, d_cnt, nb, nullptr, nullptr, nullptr, d_norm, nullptr, true));
    CMX_TRY(cluster_batch_dev(ctx, dist_kind, linkage, d_cnt, nb, n, rb, d_norm, nullptr, d_mg, d_dm, d_sz, d_st, d_nmn, nullptr));
    HIP_TRY(ctx, hipDeviceSynchronize());
    CMX_TRY(download(ctx, merge + 2 * r0 * nm, d_mg, 2 * rb * nm));
    CMX_TRY(download(ctx, size + r0 * nm, d_sz, rb * nm));
    CMX_TRY(download(ctx, dmax + r0 * nm, d_dm, rb * nm));
    CMX_TRY(download(ctx, stat + r0 * nm, d_st, rb * nm));
    CMX_TRY(download(ctx, nmin + r0 * nm, d_nmn, rb * nm));
  }
  return CMX_OK;
}

}  // extern "C"
