// C-ABI, Mica stage: mutual information of alignment columns, the bootstrap nulls, averages / z-scores, the permutation test.
#include "cmx_ctx.h"
#include "cmx_mica_perm.h"
#include "cmx_philox.h"

// the 256 compatibility masks of an alphabet: a state is itself, every other code "unknown" (compatible with all states)
// unless the caller's table says otherwise (an empty mask there is an unknown too)
static std::vector<uint32_t> mi_mask_table(int nalpha, const uint32_t* masks = nullptr, size_t nmasks = 0) {
  std::vector<uint32_t> mk(256, (1u << nalpha) - 1u);
  for (int i = 0; i < nalpha; ++i) mk[i] = 1u << i;
  if (masks) for (size_t i = 0; i < nmasks && i < 256; ++i) mk[i] = masks[i];
  for (size_t i = 0; i < 256; ++i) if (mk[i] == 0) mk[i] = (1u << nalpha) - 1u;
  return mk;
}
// a _dev call without a table: the default one, in scratch
static cmx_status default_mi_masks(cmx_ctx* ctx, int nalpha, const uint32_t** d_masks) {
  if (*d_masks) return CMX_OK;
  uint32_t* p = nullptr;
  CMX_TRY(scratch(ctx, "mi_masks", 256, &p));
  HIP_TRY(ctx, hipMemcpy(p, mi_mask_table(nalpha).data(), 256 * sizeof(uint32_t), hipMemcpyHostToDevice));
  *d_masks = p;
  return CMX_OK;
}

// the scratch of alignment k = 1, 2 that `path` reads (or writes: the classification kernels fill C, flag, gap and S on every path)
static cmx_status mica_side_scratch(cmx_ctx* ctx, MicaPath path, int Tp, int k, MicaSide* s) {
  const std::string t = std::to_string(k);
  const size_t n = s->n, codes = (size_t)Tp * (n + kMicaCodePad);
  if (path == kMicaDna1) CMX_TRY(scratch(ctx, ("mica_H" + t).c_str(), 32 * (size_t)Tp * n, &s->H));
  CMX_TRY(scratch(ctx, ("mica_C" + t).c_str(), codes, &s->C));
  CMX_TRY(scratch(ctx, ("mica_f" + t).c_str(), n, &s->flag));
  CMX_TRY(scratch(ctx, ("mica_g" + t).c_str(), n, &s->gap));
  CMX_TRY(scratch(ctx, ("mica_S" + t).c_str(), n, &s->S));
  if (path != kMicaProtein4) return CMX_OK;
  CMX_TRY(scratch(ctx, ("mica_info" + t).c_str(), mica4_info_words(n), &s->info));
  CMX_TRY(scratch(ctx, ("mica_order" + t).c_str(), n, &s->order));
  CMX_TRY(scratch(ctx, ("mica_Cs" + t).c_str(), codes, &s->Cs));
  return scratch(ctx, ("mica_Ss" + t).c_str(), n, &s->Ss);
}

// Alphabets other than 4 / 20 states (2 .. 64, cmx_mica_wide.hip): every code >= nalpha is an unknown, a mask table is refused
static bool mica_wide(int nalpha) { return nalpha != 4 && nalpha != 20; }
static cmx_status mica_alphabet(cmx_ctx* ctx, const char* who, int nalpha, const void* masks) {
  if (nalpha < 2 || nalpha > 64) return fail(ctx, CMX_ERR_INVALID, std::string(who) + ": 2 <= alphabet size <= 64");
  if (mica_wide(nalpha) && masks)
    return fail(ctx, CMX_ERR_UNSUPPORTED, std::string(who) + ": no ambiguity table for alphabets other than 4 / 20 states (codes >= nstates are unknowns)");
  return CMX_OK;
}
// their scratch, under names of its own: the symbol bytes and column sums of the matrix-core kernel, the counts of both kernels
static cmx_status mica_wide_side_scratch(cmx_ctx* ctx, MicaPath path, int nalpha, int Tp, int k, MicaSide* s) {
  const std::string t = std::to_string(k);
  const size_t n = s->n;
  CMX_TRY(scratch(ctx, ("micaw_cnt" + t).c_str(), n * (size_t)nalpha, &s->cnt));
  CMX_TRY(scratch(ctx, ("micaw_unk" + t).c_str(), n, &s->unk));
  if (path != kMicaWide) return CMX_OK;
  CMX_TRY(scratch(ctx, ("micaw_C" + t).c_str(), n * (size_t)Tp, &s->C));
  CMX_TRY(scratch(ctx, ("micaw_g" + t).c_str(), n, &s->gap));
  return scratch(ctx, ("micaw_S" + t).c_str(), n, &s->S);
}

cmx_status cmx_mi_columns_dev(cmx_ctx* ctx, int nalpha, int ntaxa, const uint32_t* d_masks, const uint8_t* d_aln1,
                              size_t n1, size_t ld1, const uint8_t* d_aln2, size_t n2, size_t ld2, double* d_mi,
                              double* d_hjoint, size_t ldo, double* d_h1, double* d_h2, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  CMX_TRY(mica_alphabet(ctx, "cmx_mi_columns", nalpha, d_masks));
  const bool intra = d_aln2 == nullptr;
  if (intra) { d_aln2 = d_aln1; n2 = n1; ld2 = ld1; }
  if (!mica_wide(nalpha)) CMX_TRY(default_mi_masks(ctx, nalpha, &d_masks));
  if (!d_aln1 || !d_mi || !d_hjoint || ntaxa < 1 || n1 == 0 || n2 == 0 || ld1 < n1 || ld2 < n2 || ldo < n2)
    return fail(ctx, CMX_ERR_INVALID, "cmx_mi_columns: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the MFMA paths (one-hot Gram) serve the columns without partial ambiguity codes, the LDS-table kernel the pairs of the
  // others
  MicaWork w{{{n1}, {n2}}};   // the column counts; every pointer null
  w.Tp = mica_padded_taxa(ntaxa);
  const MicaPath path = mica_path(nalpha, ntaxa, n1, n2);
  if (mica_wide(nalpha) && path == kMicaRefused)
    return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_mi_columns: more column tiles than one launch of the matrix-core kernel takes (2^31 - 1); split the call");
  if (path == kMicaWide || path == kMicaWidePlain) {
    CMX_TRY(mica_wide_side_scratch(ctx, path, nalpha, w.Tp, 1, &w.s[0]));
    if (intra) w.s[1] = w.s[0];
    else CMX_TRY(mica_wide_side_scratch(ctx, path, nalpha, w.Tp, 2, &w.s[1]));
    if (path == kMicaWide) CMX_TRY(scratch(ctx, "micaw_ftab", micaw_ftab_entries(nalpha, ntaxa), &w.ftab));
  } else if (path != kMicaTables && path != kMicaRefused) {
    CMX_TRY(mica_side_scratch(ctx, path, w.Tp, 1, &w.s[0]));
    if (intra) w.s[1] = w.s[0];
    else CMX_TRY(mica_side_scratch(ctx, path, w.Tp, 2, &w.s[1]));
    CMX_TRY(scratch(ctx, "mica_ftab", mica_ftab_entries(nalpha, ntaxa), &w.ftab));
    CMX_TRY(scratch(ctx, "mica_any", 1, &w.anyflag));
    if (path == kMicaProtein4) CMX_TRY(scratch(ctx, "mica_img2", mica4_image_bytes(w.Tp, n2), &w.img2));
  }
  HIP_TRY(ctx, launch_mi_columns(nalpha, ntaxa, d_masks, d_aln1, ld1, d_aln2, ld2, intra ? 1 : 0, d_mi, d_hjoint, ldo, d_h1,
                                 intra ? nullptr : d_h2, w, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_mi_columns(cmx_ctx* ctx, int nalpha, int ntaxa, const uint32_t* masks, size_t nmasks, const uint8_t* aln1,
                          size_t n1, const uint8_t* aln2, size_t n2, double* mi, double* hjoint, double* h1, double* h2) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!aln1 || !mi || !hjoint || n1 == 0 || ntaxa < 1 || nalpha < 2 || nalpha > 64) return fail(ctx, CMX_ERR_INVALID, "cmx_mi_columns: bad arguments");
  CMX_TRY(mica_alphabet(ctx, "cmx_mi_columns", nalpha, masks));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!aln2) n2 = n1;
  TmpDev tmp;
  uint32_t* d_masks = nullptr;
  uint8_t *d1, *d2 = nullptr;
  double *d_mi, *d_hj, *d_h1, *d_h2 = nullptr;
  if (!mica_wide(nalpha)) CMX_TRY(tmp.upload(ctx, &d_masks, mi_mask_table(nalpha, masks, nmasks).data(), 256));
  CMX_TRY(tmp.upload(ctx, &d1, aln1, (size_t)ntaxa * n1));
  if (aln2) {
    CMX_TRY(tmp.upload(ctx, &d2, aln2, (size_t)ntaxa * n2));
    CMX_TRY(tmp.alloc(ctx, &d_h2, n2));
  }
  CMX_TRY(tmp.alloc(ctx, &d_mi, n1 * n2));
  CMX_TRY(tmp.alloc(ctx, &d_hj, n1 * n2));
  CMX_TRY(tmp.alloc(ctx, &d_h1, n1));
  CMX_TRY(cmx_mi_columns_dev(ctx, nalpha, ntaxa, d_masks, d1, n1, n1, d2, n2, n2, d_mi, d_hj, n2, d_h1, d_h2, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, mi, d_mi, n1 * n2));
  CMX_TRY(download(ctx, hjoint, d_hj, n1 * n2));
  CMX_TRY(download(ctx, h1, d_h1, n1));
  return download(ctx, h2, aln2 ? d_h2 : d_h1, n2);
}

// d_masks: device table of 256 compatibility masks (NULL: codes >= nalpha are unknowns); column indices are validated by
// the caller (the host entry point checks them)
cmx_status cmx_mi_pairs_dev(cmx_ctx* ctx, int nalpha, int ntaxa, const uint32_t* d_masks, const uint8_t* d_aln1, size_t n1, size_t ld1,
                            const uint8_t* d_aln2, size_t n2, size_t ld2, const int64_t* d_idx1, const int64_t* d_idx2, size_t npairs,
                            double* d_mi, double* d_hjoint, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  CMX_TRY(mica_alphabet(ctx, "cmx_mi_pairs", nalpha, d_masks));
  if (!d_aln2) { d_aln2 = d_aln1; n2 = n1; ld2 = ld1; }
  if (!d_aln1 || !d_idx1 || !d_idx2 || !d_mi || !d_hjoint || n1 == 0 || n2 == 0 || ld1 < n1 || ld2 < n2 || ntaxa < 1 || npairs == 0)
    return fail(ctx, CMX_ERR_INVALID, "cmx_mi_pairs: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!mica_wide(nalpha)) CMX_TRY(default_mi_masks(ctx, nalpha, &d_masks));
  HIP_TRY(ctx, launch_mi_pairs(nalpha, ntaxa, d_masks, d_aln1, ld1, d_aln2, ld2, d_idx1, d_idx2, npairs, d_mi, d_hjoint, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_mi_pairs(cmx_ctx* ctx, int nalpha, int ntaxa, const uint32_t* masks, size_t nmasks, const uint8_t* aln1,
                        size_t n1, const uint8_t* aln2, size_t n2, const int64_t* idx1, const int64_t* idx2, size_t npairs,
                        double* mi, double* hjoint) {
  if (!ctx) return CMX_ERR_INVALID;
  CMX_TRY(mica_alphabet(ctx, "cmx_mi_pairs", nalpha, masks));
  if (!aln1 || !idx1 || !idx2 || !mi || !hjoint || n1 == 0 || ntaxa < 1 || npairs == 0)
    return fail(ctx, CMX_ERR_INVALID, "cmx_mi_pairs: bad arguments");
  if (!aln2) n2 = n1;
  for (size_t p = 0; p < npairs; ++p)
    if (idx1[p] < 0 || (size_t)idx1[p] >= n1 || idx2[p] < 0 || (size_t)idx2[p] >= n2)
      return fail(ctx, CMX_ERR_INVALID, "cmx_mi_pairs: column index out of range");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  uint32_t* d_masks = nullptr;
  uint8_t *d1, *d2 = nullptr;
  int64_t *di1, *di2;
  double *d_mi, *d_hj;
  if (!mica_wide(nalpha)) CMX_TRY(tmp.upload(ctx, &d_masks, mi_mask_table(nalpha, masks, nmasks).data(), 256));
  CMX_TRY(tmp.upload(ctx, &d1, aln1, (size_t)ntaxa * n1));
  if (aln2) CMX_TRY(tmp.upload(ctx, &d2, aln2, (size_t)ntaxa * n2));
  CMX_TRY(tmp.upload(ctx, &di1, idx1, npairs));
  CMX_TRY(tmp.upload(ctx, &di2, idx2, npairs));
  CMX_TRY(tmp.alloc(ctx, &d_mi, npairs));
  CMX_TRY(tmp.alloc(ctx, &d_hj, npairs));
  CMX_TRY(cmx_mi_pairs_dev(ctx, nalpha, ntaxa, d_masks, d1, n1, n1, d2, n2, n2, di1, di2, npairs, d_mi, d_hj, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, mi, d_mi, npairs));
  return download(ctx, hjoint, d_hj, npairs);
}

// ---- Mica's bootstrap nulls.  Site indices of the non-parametric bootstrap (SiteContainerTools::sampleSites,
// CoMap/Mica.cpp:426-430) come from the engine's counter RNG (cmx_philox.h philox_uniform: Philox2x32-10, key from the
// seed, counter = (g, draw)), so that every binding -- this library's C++ adapter, the Python mirror, a Mica.cpp linked
// against the C-ABI -- draws the same pairs: idx_h[r * rep_ram + j] = floor(u(seed, g = (r * 2 + h) * rep_ram + j, draw 0) * nsites).
cmx_status cmx_mica_bootstrap_indices(uint64_t seed, size_t nsites, size_t nrep_cpu, size_t nrep_ram, int64_t* idx1, int64_t* idx2) {
  if (nsites == 0 || !idx1 || !idx2 || (uint64_t)nrep_cpu * 2 * nrep_ram > (1ull << 47)) return CMX_ERR_INVALID;
  for (size_t r = 0; r < nrep_cpu; ++r)
    for (size_t j = 0; j < nrep_ram; ++j)
      for (int h = 0; h < 2; ++h) {
        size_t v = (size_t)(philox_uniform(seed, ((uint64_t)r * 2 + h) * nrep_ram + j, 0) * (double)nsites);
        if (v >= nsites) v = nsites - 1;
        (h ? idx2 : idx1)[r * nrep_ram + j] = (int64_t)v;
      }
  return CMX_OK;
}

// null.method = parametric-bootstrap (CoMap/Mica.cpp:469-548): per replicate two alignments of nrep_ram sites are simulated
// under the context's model, column j of the one is scored against column j of the other (MI, joint entropy), and -- Mica's
// `use_model` case -- both are mapped for their norms.  One simulation, one MI launch and one mapping over all replicates,
// none of it leaving the device; only the null's columns come back.
cmx_status cmx_mica_parametric_null(cmx_ctx* ctx, int nalpha, uint64_t seed, size_t nrep_cpu, size_t nrep_ram, double gamma_alpha,
                                    double p_invariant, double* mi, double* hjoint, double* nmin) {
  CMX_TRY(need_model(ctx));
  if (nrep_cpu == 0 || nrep_ram == 0 || !mi || !hjoint) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_parametric_null: bad arguments");
  if (nalpha != ctx->hm.S) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_parametric_null: the alphabet is the model's");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = nrep_cpu * nrep_ram, T = (size_t)ctx->hm.T;
  TmpDev tmp;
  uint8_t* d_aln;
  int64_t *d_i1, *d_i2;
  double *d_mi, *d_hj, *d_norm = nullptr;
  CMX_TRY(tmp.alloc(ctx, &d_aln, T * 2 * n));
  CMX_TRY(tmp.alloc(ctx, &d_i1, n));
  CMX_TRY(tmp.alloc(ctx, &d_i2, n));
  CMX_TRY(tmp.alloc(ctx, &d_mi, n));
  CMX_TRY(tmp.alloc(ctx, &d_hj, n));
  // simulated-site index g = (rep * 2 + batch) * nrep_ram + j = its column in the [T][2 n] alignment
  if (gamma_alpha > 0.0) CMX_TRY(cmx_simulate_continuous_dev(ctx, seed, 0, 2 * n, gamma_alpha, p_invariant, d_aln, 2 * n, nullptr, nullptr));
  else CMX_TRY(cmx_simulate_dev(ctx, seed, 0, 2 * n, d_aln, 2 * n, nullptr, nullptr));
  std::vector<int64_t> i1(n), i2(n);
  for (size_t q = 0; q < n; ++q) {
    const size_t rep = q / nrep_ram, j = q % nrep_ram;
    i1[q] = (int64_t)((rep * 2) * nrep_ram + j);
    i2[q] = (int64_t)((rep * 2 + 1) * nrep_ram + j);
  }
  HIP_TRY(ctx, hipMemcpy(d_i1, i1.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(d_i2, i2.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
  CMX_TRY(cmx_mi_pairs_dev(ctx, nalpha, (int)T, nullptr, d_aln, 2 * n, 2 * n, nullptr, 0, 0, d_i1, d_i2, n, d_mi, d_hj, nullptr));
  if (nmin) {
    CMX_TRY(tmp.alloc(ctx, &d_norm, 2 * n));
    CMX_TRY(map_sites_impl(ctx, d_aln, 2 * n, 2 * n, nullptr, nullptr, 0, nullptr, nullptr, nullptr, d_norm, nullptr, true));
  }
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, mi, d_mi, n));
  CMX_TRY(download(ctx, hjoint, d_hj, n));
  if (nmin) {
    std::vector<double> norm(2 * n);
    CMX_TRY(download(ctx, norm.data(), d_norm, 2 * n));
    for (size_t q = 0; q < n; ++q) nmin[q] = std::min(norm[(size_t)i1[q]], norm[(size_t)i2[q]]);
  }
  return CMX_OK;
}

int cmx_debug_mica_wide_plain(int on) { return mica_wide_plain(on); }

// ------------------------------------------------------------------------------------------------ Mica post-processing
cmx_status cmx_mica_average_mi_dev(cmx_ctx* ctx, const double* d_mi, size_t n, size_t ldo, double* d_average,
                                   double* d_full_average, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!d_mi || n < 2 || ldo < n || !d_average || !d_full_average) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_average_mi: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, launch_mica_average(d_mi, n, ldo, d_average, d_full_average, (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_mica_average_mi(cmx_ctx* ctx, const double* mi, size_t n, double* average, double* full_average) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!mi || n < 2 || !average || !full_average) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_average_mi: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  double *d_mi, *d_avg, *d_full;
  CMX_TRY(tmp.upload(ctx, &d_mi, mi, n * n));
  CMX_TRY(tmp.alloc(ctx, &d_avg, n));
  CMX_TRY(tmp.alloc(ctx, &d_full, 1));
  CMX_TRY(cmx_mica_average_mi_dev(ctx, d_mi, n, n, d_avg, d_full, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, average, d_avg, n));
  return download(ctx, full_average, d_full, 1);
}

cmx_status cmx_mica_zscore_null_dev(cmx_ctx* ctx, int which, const double* d_mi, size_t n, size_t ldo, const double* d_average,
                                    const double* d_full_average, const double* d_key, double* d_null_stat,
                                    double* d_null_key, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  if (which < CMX_MICA_MI || which > CMX_MICA_MIC) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_zscore_null: unknown statistic");
  if (!d_mi || n < 2 || ldo < n || !d_key || !d_null_stat || !d_null_key || (which != CMX_MICA_MI && (!d_average || !d_full_average)))
    return fail(ctx, CMX_ERR_INVALID, "cmx_mica_zscore_null: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, launch_mica_zscore(which, d_mi, n, ldo, d_average, d_full_average, d_key, d_null_stat, d_null_key,
                                  (hipStream_t)stream));
  return CMX_OK;
}

cmx_status cmx_mica_zscore_null(cmx_ctx* ctx, int which, const double* mi, size_t n, const double* key, double* null_stat,
                                double* null_key) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!mi || n < 2 || !key || !null_stat || !null_key) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_zscore_null: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t np = n * (n - 1) / 2;
  TmpDev tmp;
  double *d_mi, *d_avg, *d_full, *d_key, *d_ns, *d_nk;
  CMX_TRY(tmp.upload(ctx, &d_mi, mi, n * n));
  CMX_TRY(tmp.alloc(ctx, &d_avg, n));
  CMX_TRY(tmp.alloc(ctx, &d_full, 1));
  CMX_TRY(tmp.upload(ctx, &d_key, key, n));
  CMX_TRY(tmp.alloc(ctx, &d_ns, np));
  CMX_TRY(tmp.alloc(ctx, &d_nk, np));
  CMX_TRY(cmx_mica_average_mi_dev(ctx, d_mi, n, n, d_avg, d_full, nullptr));
  CMX_TRY(cmx_mica_zscore_null_dev(ctx, which, d_mi, n, n, d_avg, d_full, d_key, d_ns, d_nk, nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, null_stat, d_ns, np));
  return download(ctx, null_key, d_nk, np);
}

// extended codes of the permutation test: states 0..A-1; a code in [A, min(nmasks, 31)) with a partial mask keeps its
// number; everything else (codes without an entry, gap, X, N: all states) is 31 = unknown.  L = lcm of the state counts.
namespace {
struct PermCodes {
  uint8_t emap[256];
  uint32_t emask[32], ewgt[32];
  uint32_t L;
};
cmx_status perm_codes(cmx_ctx* ctx, int A, const uint32_t* masks, size_t nmasks, int T, PermCodes* pc) {
  const uint32_t all = (1u << A) - 1u;
  unsigned long long L = (unsigned long long)A;
  auto lcm = [](unsigned long long a, unsigned long long b) {
    unsigned long long x = a, y = b;
    while (y) { const unsigned long long r = x % y; x = y; y = r; }
    return a / x * b;
  };
  int k[32];
  for (int e = 0; e < 32; ++e) { pc->emask[e] = e < A ? (1u << e) : all; k[e] = e < A ? 1 : A; }
  for (int c = 0; c < 256; ++c) {
    if (c < A) { pc->emap[c] = (uint8_t)c; continue; }
    if (!masks || (size_t)c >= nmasks) { pc->emap[c] = 31; continue; }
    const uint32_t m = masks[c] & all;
    if (m == 0) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_permutation_test: mask of code " + std::to_string(c) + " has no state");
    if (m == all) { pc->emap[c] = 31; continue; }
    if (c >= 31) return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_mica_permutation_test: partial ambiguity codes must be < 31");
    pc->emap[c] = (uint8_t)c;
    pc->emask[c] = m;
    k[c] = __builtin_popcount(m);
    L = lcm(L, (unsigned long long)k[c]);
  }
  const double M = (double)L * (double)L * (double)T;
  if (M > 67108864.0)
    return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_mica_permutation_test: lcm of the ambiguity codes' state counts too large for the fixed-point table");
  pc->L = (uint32_t)L;
  for (int e = 0; e < 32; ++e) pc->ewgt[e] = (uint32_t)(L / (unsigned long long)k[e]);
  return CMX_OK;
}

// ---- what the entries of both alphabet families share (who: the entry's name in its messages)
cmx_status perm_taxa(cmx_ctx* ctx, const char* who, int ntaxa) {
  if (ntaxa < 2 || ntaxa > mica_perm_max_taxa())
    return fail(ctx, CMX_ERR_UNSUPPORTED, std::string(who) + ": 2 <= ntaxa <= " + std::to_string(mica_perm_max_taxa()));
  return CMX_OK;
}
cmx_status perm_args(cmx_ctx* ctx, const char* who, const uint8_t* aln, size_t n, size_t ld, uint32_t max_perm, size_t pair_begin,
                     size_t pair_end, const double* pvalue, const int32_t* nperm) {
  if (!aln || n < 2 || ld < n || max_perm == 0 || pair_end <= pair_begin || pair_end > n * (n - 1) / 2 || !pvalue || !nperm)
    return fail(ctx, CMX_ERR_INVALID, std::string(who) + ": bad arguments");
  return CMX_OK;
}

// resolved pairs: F[c] = round(c ln c * 2^40); the kernels accumulate F[c+1] - F[c] per increment of a joint count.  Into
// scratch `name` on `st` (the source is owned by the context: a failing call further down must not free memory an upload
// still reads; every caller synchronises `st` before it returns)
cmx_status perm_increments(cmx_ctx* ctx, const char* name, int T, hipStream_t st, long long** d_dF) {
  CMX_TRY(scratch(ctx, name, (size_t)T, d_dF));
  std::vector<long long>& dF = ctx->perm_dF_host;
  dF.assign(T, 0);
  long long prev = 0;
  for (int c = 1; c <= T; ++c) {
    const long long f = std::llround((double)c * std::log((double)c) * 1099511627776.0);
    dF[c - 1] = f - prev;
    prev = f;
  }
  HIP_TRY(ctx, hipMemcpyAsync(*d_dF, dF.data(), sizeof(long long) * T, hipMemcpyHostToDevice, st));
  return CMX_OK;
}

// pairs with non-states: F[m] = round(m ln m 2^sh) for m <= M, resident in scratch `name` on `st`.  Built on the host, with the
// oracle's logarithm, so that the fixed-point sums, and with them every tie, are the oracle's; once per (M, sh) -- a caller that
// shards the pairs over several calls pays for it once.  The device copy is keyed by the buffer's allocation too: scratch
// starts over when it grows, and when the scratch guard is switched on after the context was created.
cmx_status perm_table(cmx_ctx* ctx, PermTable& t, const char* name, size_t M, hipStream_t st, long long** d_F) {
  const int sh = std::min(40, 62 - (int)std::ceil(std::log2((double)M * std::log((double)M))));
  CMX_TRY(scratch(ctx, name, M + 1, d_F));
  if (t.M != M || t.sh != sh || t.host.size() != M + 1) {
    t.sh = -1;
    t.allocs = 0;
    t.host.assign(M + 1, 0);
    const double scale = std::ldexp(1.0, sh);
    for (size_t m = 1; m <= M; ++m) t.host[m] = std::llround((double)m * std::log((double)m) * scale);
    t.M = M; t.sh = sh;
  }
  const size_t allocs = ctx->scratch[name].allocs;
  if (t.allocs != allocs) {
    HIP_TRY(ctx, hipMemcpyAsync(*d_F, t.host.data(), sizeof(long long) * (M + 1), hipMemcpyHostToDevice, st));
    t.allocs = allocs;
  }
  return CMX_OK;
}

// the host-pointer entries: the alignment up, run(d_aln, d_pvalue, d_nperm) for np pairs, both results down
template <class Run>
cmx_status perm_host_call(cmx_ctx* ctx, int ntaxa, const uint8_t* aln, size_t n, size_t np, double* pvalue, int32_t* nperm, Run run) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpDev tmp;
  uint8_t* d_aln;
  double* d_pv;
  int32_t* d_np;
  CMX_TRY(tmp.upload(ctx, &d_aln, aln, (size_t)ntaxa * n));
  CMX_TRY(tmp.alloc(ctx, &d_pv, np));
  CMX_TRY(tmp.alloc(ctx, &d_np, np));
  CMX_TRY(run(d_aln, d_pv, d_np));
  HIP_TRY(ctx, hipDeviceSynchronize());
  CMX_TRY(download(ctx, pvalue, d_pv, np));
  return download(ctx, nperm, d_np, np);
}
}  // namespace

cmx_status cmx_mica_permutation_test_masks_dev(cmx_ctx* ctx, int nalpha, int ntaxa, const uint32_t* masks, size_t nmasks,
                                               const uint8_t* d_aln, size_t n, size_t ld, uint32_t max_perm, uint64_t seed,
                                               size_t pair_begin, size_t pair_end, double* d_pvalue, int32_t* d_nperm, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  if (nalpha != 4 && nalpha != 20) return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_mica_permutation_test: alphabet size must be 4 or 20 (other alphabets: cmx_mica_permutation_test_states)");
  CMX_TRY(perm_taxa(ctx, "cmx_mica_permutation_test", ntaxa));
  CMX_TRY(perm_args(ctx, "cmx_mica_permutation_test", d_aln, n, ld, max_perm, pair_begin, pair_end, d_pvalue, d_nperm));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  PermCodes pc;
  CMX_TRY(perm_codes(ctx, nalpha, masks, nmasks, ntaxa, &pc));
  uint16_t *d_cnt, *d_ext, *d_order = nullptr;
  uint8_t *d_emap, *d_hasamb;
  uint32_t* d_tab;   // emask[32] | ewgt[32]
  int* d_bad;
  long long *d_dF, *d_F = nullptr;
  CMX_TRY(scratch(ctx, "perm_cnt", n * nalpha, &d_cnt));
  CMX_TRY(scratch(ctx, "perm_ext", n * 32, &d_ext));
  CMX_TRY(scratch(ctx, "perm_emap", 256, &d_emap));
  CMX_TRY(scratch(ctx, "perm_hasamb", n, &d_hasamb));
  CMX_TRY(scratch(ctx, "perm_tab", 64, &d_tab));
  CMX_TRY(scratch(ctx, "perm_bad", 2, &d_bad));
  CMX_TRY(perm_increments(ctx, "perm_dF", ntaxa, st, &d_dF));
  ctx->perm_tab_host.assign(256 + 64 * sizeof(uint32_t), 0);
  std::memcpy(ctx->perm_tab_host.data(), pc.emap, 256);
  std::memcpy(ctx->perm_tab_host.data() + 256, pc.emask, 32 * sizeof(uint32_t));
  std::memcpy(ctx->perm_tab_host.data() + 256 + 32 * sizeof(uint32_t), pc.ewgt, 32 * sizeof(uint32_t));
  HIP_TRY(ctx, hipMemcpyAsync(d_emap, ctx->perm_tab_host.data(), 256, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_tab, ctx->perm_tab_host.data() + 256, sizeof(uint32_t) * 64, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(d_bad, 0, 2 * sizeof(int), st));
  HIP_TRY(ctx, launch_mica_colcount(d_aln, ntaxa, n, ld, nalpha, d_emap, d_cnt, d_ext, d_hasamb, d_bad, st));
  int bad[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(bad, d_bad, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));   // the one host decision of this call: are there pairs with unknowns at all
  int cus = 0;
  HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (bad[0]) {
    // pairs with gaps / unknowns / ambiguity codes (SiteTools::*(.., resolveUnknowns = true)): a kernel of their own, with
    // the fixed-point table for m <= L^2 T and column i's visiting order
    if (mica_perm_general_lds(ntaxa, nalpha, bad[1]) == 0)
      return fail(ctx, CMX_ERR_UNSUPPORTED, "cmx_mica_permutation_test: " + std::to_string(ntaxa) + " taxa with " + std::to_string(bad[1]) +
                                            " distinct ambiguity codes in one column do not fit the LDS");
    CMX_TRY(perm_table(ctx, ctx->perm_F, "perm_F", (size_t)pc.L * pc.L * (size_t)ntaxa, st, &d_F));
    CMX_TRY(scratch(ctx, "perm_order", n * (size_t)ntaxa, &d_order));
    HIP_TRY(ctx, launch_mica_colorder(d_aln, ntaxa, n, ld, nalpha, d_emap, d_ext, d_order, st));
  }
  HIP_TRY(ctx, launch_mica_perm(nalpha, ntaxa, d_aln, ld, n, d_cnt, d_hasamb, d_emap, d_ext, d_order, d_tab, d_tab + 32, d_dF, d_F, pc.L,
                                bad[1], max_perm, seed, pair_begin, pair_end, d_pvalue, d_nperm, cus, st));
  return CMX_OK;
}

cmx_status cmx_mica_permutation_test_dev(cmx_ctx* ctx, int nalpha, int ntaxa, const uint8_t* d_aln, size_t n, size_t ld,
                                         uint32_t max_perm, uint64_t seed, size_t pair_begin, size_t pair_end,
                                         double* d_pvalue, int32_t* d_nperm, void* stream) {
  return cmx_mica_permutation_test_masks_dev(ctx, nalpha, ntaxa, nullptr, 0, d_aln, n, ld, max_perm, seed, pair_begin, pair_end,
                                             d_pvalue, d_nperm, stream);
}

cmx_status cmx_mica_permutation_test_masks(cmx_ctx* ctx, int nalpha, int ntaxa, const uint32_t* masks, size_t nmasks,
                                           const uint8_t* aln, size_t n, uint32_t max_perm, uint64_t seed, double* pvalue,
                                           int32_t* nperm) {
  if (!ctx) return CMX_ERR_INVALID;
  if (!aln || n < 2 || ntaxa < 2 || !pvalue || !nperm) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_permutation_test: bad arguments");
  const size_t np = n * (n - 1) / 2;
  return perm_host_call(ctx, ntaxa, aln, n, np, pvalue, nperm, [&](const uint8_t* d_aln, double* d_pv, int32_t* d_np) {
    return cmx_mica_permutation_test_masks_dev(ctx, nalpha, ntaxa, masks, nmasks, d_aln, n, n, max_perm, seed, 0, np, d_pv, d_np, nullptr);
  });
}

cmx_status cmx_mica_permutation_test(cmx_ctx* ctx, int nalpha, int ntaxa, const uint8_t* aln, size_t n, uint32_t max_perm,
                                     uint64_t seed, double* pvalue, int32_t* nperm) {
  return cmx_mica_permutation_test_masks(ctx, nalpha, ntaxa, nullptr, 0, aln, n, max_perm, seed, pvalue, nperm);
}

// ---- the same test for every alphabet of 2 .. 64 states, without a mask table (cmx_mica_perm_wide.hip); 4 / 20 states are
// the entry above with masks = NULL.  The entries above keep refusing the other alphabets: folding the two families into one
// entry is a later change.
static cmx_status permw_shape(cmx_ctx* ctx, int nalpha, int ntaxa) {
  if (nalpha < 2 || nalpha > 64) return fail(ctx, CMX_ERR_INVALID, "cmx_mica_permutation_test_states: 2 <= alphabet size <= 64");
  return perm_taxa(ctx, "cmx_mica_permutation_test_states", ntaxa);
}

cmx_status cmx_mica_permutation_test_states_dev(cmx_ctx* ctx, int nalpha, int ntaxa, const uint8_t* d_aln, size_t n, size_t ld,
                                                uint32_t max_perm, uint64_t seed, size_t pair_begin, size_t pair_end,
                                                double* d_pvalue, int32_t* d_nperm, void* stream) {
  if (!ctx) return CMX_ERR_INVALID;
  CMX_TRY(permw_shape(ctx, nalpha, ntaxa));
  if (!mica_wide(nalpha))
    return cmx_mica_permutation_test_masks_dev(ctx, nalpha, ntaxa, nullptr, 0, d_aln, n, ld, max_perm, seed, pair_begin, pair_end,
                                               d_pvalue, d_nperm, stream);
  CMX_TRY(perm_args(ctx, "cmx_mica_permutation_test_states", d_aln, n, ld, max_perm, pair_begin, pair_end, d_pvalue, d_nperm));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int A = nalpha, T = ntaxa;
  uint16_t *d_end, *d_unk, *d_order;
  uint8_t* d_flag;
  int* d_any;
  long long *d_dF, *d_F = nullptr;
  CMX_TRY(scratch(ctx, "permw_end", n * (size_t)A, &d_end));
  CMX_TRY(scratch(ctx, "permw_unk", n, &d_unk));
  CMX_TRY(scratch(ctx, "permw_flag", n, &d_flag));
  CMX_TRY(scratch(ctx, "permw_order", n * (size_t)T, &d_order));
  CMX_TRY(scratch(ctx, "permw_any", 1, &d_any));
  CMX_TRY(perm_increments(ctx, "permw_dF", T, st, &d_dF));
  HIP_TRY(ctx, hipMemsetAsync(d_any, 0, sizeof(int), st));
  HIP_TRY(ctx, launch_mica_permw_classify(A, T, d_aln, ld, n, d_end, d_unk, d_flag, d_order, d_any, st));
  int any = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&any, d_any, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));   // the one host decision of this call: are there columns with unknowns at all
  // the unknowns' table: m <= A^2 T (8.4 M entries at 64 states x 2 047 taxa)
  if (any) CMX_TRY(perm_table(ctx, ctx->permw_F, "permw_F", (size_t)A * A * (size_t)T, st, &d_F));
  int cus = 0;
  HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  HIP_TRY(ctx, launch_mica_permw(A, T, d_aln, ld, n, d_end, d_unk, d_flag, d_order, d_dF, d_F, max_perm, seed, pair_begin, pair_end,
                                 d_pvalue, d_nperm, cus, st));
  return CMX_OK;
}

cmx_status cmx_mica_permutation_test_states(cmx_ctx* ctx, int nalpha, int ntaxa, const uint8_t* aln, size_t n, uint32_t max_perm,
                                            uint64_t seed, size_t pair_begin, size_t pair_end, double* pvalue, int32_t* nperm) {
  if (!ctx) return CMX_ERR_INVALID;
  CMX_TRY(permw_shape(ctx, nalpha, ntaxa));
  CMX_TRY(perm_args(ctx, "cmx_mica_permutation_test_states", aln, n, n, max_perm, pair_begin, pair_end, pvalue, nperm));
  return perm_host_call(ctx, ntaxa, aln, n, pair_end - pair_begin, pvalue, nperm, [&](const uint8_t* d_aln, double* d_pv, int32_t* d_np) {
    return cmx_mica_permutation_test_states_dev(ctx, nalpha, ntaxa, d_aln, n, n, max_perm, seed, pair_begin, pair_end, d_pv, d_np, nullptr);
  });
}
