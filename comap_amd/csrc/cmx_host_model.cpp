// Host model, the substitution model and the device layouts (see cmx_host_model.h): model validation, generators, branch
// matrices P, P o N^k, N1, NC, the matrices and tables the device reads, and build_host_model itself.  The tree and the walk
// program are in cmx_host_tree.cpp, the self-check in cmx_host_verify.cpp.  Plain C++17, no device code.
#include "cmx_host_parts.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace cmx {
namespace {

using Mat = std::vector<double>;

Mat matmul(int n, const Mat& A, const Mat& B) {
  Mat C((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k) {
      const double a = A[(size_t)i * n + k];
      for (int j = 0; j < n; ++j) C[(size_t)i * n + j] += a * B[(size_t)k * n + j];
    }
  return C;
}

// cyclic Jacobi eigen-solver for a symmetric matrix (n <= 64 here); columns of U are eigenvectors
void jacobi(int n, Mat A, Mat* U, std::vector<double>* lam) {
  U->assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) (*U)[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 200; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i) {
      diag += A[(size_t)i * n + i] * A[(size_t)i * n + i];
      for (int j = i + 1; j < n; ++j) off += A[(size_t)i * n + j] * A[(size_t)i * n + j];
    }
    if (off <= 1e-40 * (diag + 1e-300)) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double theta = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - s * akq;
          A[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - s * aqk;
          A[(size_t)q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double ukp = (*U)[(size_t)k * n + p], ukq = (*U)[(size_t)k * n + q];
          (*U)[(size_t)k * n + p] = c * ukp - s * ukq;
          (*U)[(size_t)k * n + q] = s * ukp + c * ukq;
        }
      }
  }
  lam->resize(n);
  for (int i = 0; i < n; ++i) (*lam)[i] = A[(size_t)i * n + i];
}

// row-major SxS -> 4x4-block packed (tile t = (bi, bj), element k = (k/4, k%4)); layout consumed by matvec_stage.
// diag (class-fused nucleotide models: the operator is block diagonal, one 4-state tile per class): only the NB diagonal
// tiles are stored, tile (q, q) at position q -- the kernel then stages NB * 128 bytes per product instead of the unit
void pack_blocks(int S, const double* M, double* out, bool diag) {
  const int NB = S / 4;
  if (diag) {
    for (int q = 0; q < NB; ++q)
      for (int k = 0; k < 16; ++k) out[q * 16 + k] = M[(size_t)(4 * q + k / 4) * S + 4 * q + k % 4];
    return;
  }
  for (int t = 0; t < NB * NB; ++t)
    for (int k = 0; k < 16; ++k) out[t * 16 + k] = M[(size_t)(4 * (t / NB) + k / 4) * S + 4 * (t % NB) + k % 4];
}

// ------------------------------------------------------------------------------------------------ stages of build_host_model
// A stage that checks returns its error message or an empty string.  No check may move relative to another: the first
// failing one decides the message and the status code of a refused input.
std::string check_arguments(const cmx_model* model, const cmx_tree* tree, HostModel* hm, int* code) {
  if (!model || !tree) return "model and tree are required";
  const int S = model->nstates, C = model->nclasses;
  const int K = (model->nmodels > 0 ? model->Bks : model->Bk) ? model->ntypes : 1;
  if (S < 2 || S > kPlainStates) {
    *code = CMX_ERR_UNSUPPORTED;
    return "nstates must be between 2 and " + std::to_string(kPlainStates) + " (4 and 20 run on the matrix cores, the others on the plain kernels); got " + std::to_string(S);
  }
  if (C < 1 || C > 64) return "nclasses out of range";
  if (K < 1 || K > 64) return "ntypes out of range";
  if (!model->rates || !model->probs) return "rates and probs are required";
  if (model->nmodels <= 0 && (!model->Q || !model->pi)) return "Q, pi, rates and probs are required";
  hm->S = S; hm->C = C; hm->K = K;
  hm->plain = S != 4 && S != 20;
  return std::string();
}

std::string check_model(const cmx_model* model, HostModel* hm) {
  const int S = hm->S, C = hm->C;
  const bool nh = model->nmodels > 0;
  const int NM = nh ? model->nmodels : 1;
  if (nh && (!model->Qs || !model->pis || !model->model_of_branch || !model->root_freqs))
    return "non-homogeneous model: Qs, pis, model_of_branch and root_freqs are required";
  if (!nh && (model->Qs || model->pis || model->Bks || model->model_of_branch || model->root_freqs))
    return "non-homogeneous fields are set but nmodels is 0";
  // frequencies at the root: the stationary ones, or the model set's root frequency set
  const double* rootf = nh ? model->root_freqs : model->pi;
  hm->pi.assign(rootf, rootf + S);
  hm->rates.assign(model->rates, model->rates + C);
  hm->probs.assign(model->probs, model->probs + C);
  double spi = 0, spr = 0;
  for (double v : hm->pi) { if (!(v > 0)) return "pi must be positive"; spi += v; }
  for (double v : hm->probs) { if (!(v >= 0)) return "probs must be >= 0"; spr += v; }
  if (std::fabs(spi - 1.0) > 1e-6 || std::fabs(spr - 1.0) > 1e-6) return "pi and probs must sum to one";
  for (double v : hm->rates) if (!(v >= 0) || !std::isfinite(v)) return "rates must be finite and >= 0";
  hm->model_of.assign(hm->B, 0);
  if (nh)
    for (int b = 0; b < hm->B; ++b) {
      hm->model_of[b] = model->model_of_branch[b];
      if (hm->model_of[b] < 0 || hm->model_of[b] >= NM) return "model_of_branch: generator index out of range";
    }
  return std::string();
}

// eigensystem of a generator through its symmetrised form; W[k] = Vinv B_k V
struct Eig { Mat V, Vi; std::vector<double> lam; std::vector<Mat> W; };

// per generator: checks and eigen-decomposition
std::string build_generators(const cmx_model* model, HostModel* hm, std::vector<Eig>* eigs) {
  const int S = hm->S, K = hm->K;
  const bool nh = model->nmodels > 0;
  const int NM = nh ? model->nmodels : 1;
  const size_t S2 = (size_t)S * S;
  std::vector<Eig>& eig = *eigs;
  eig.resize(NM);
  for (int m = 0; m < NM; ++m) {
    const double* Qp = nh ? model->Qs + (size_t)m * S2 : model->Q;
    const double* pip = nh ? model->pis + (size_t)m * S : model->pi;
    const double* Bp = nh ? (model->Bks ? model->Bks + (size_t)m * K * S2 : nullptr) : model->Bk;
    Mat Q(Qp, Qp + S2);
    double sp = 0;
    for (int x = 0; x < S; ++x) { if (!(pip[x] > 0)) return "pi must be positive"; sp += pip[x]; }
    if (std::fabs(sp - 1.0) > 1e-6) return "pi and probs must sum to one";
    for (int x = 0; x < S; ++x) {
      double rs = 0;
      for (int y = 0; y < S; ++y) {
        rs += Q[(size_t)x * S + y];
        const double a = pip[x] * Q[(size_t)x * S + y], b = pip[y] * Q[(size_t)y * S + x];
        if (std::fabs(a - b) > 1e-9 * (std::fabs(a) + std::fabs(b) + 1e-300) + 1e-14)
          return "Q must be reversible with respect to pi (pi_x Q_xy == pi_y Q_yx)";
      }
      if (std::fabs(rs) > 1e-9) return "rows of Q must sum to zero";
    }
    std::vector<Mat> Bk(K);
    for (int k = 0; k < K; ++k) {
      if (Bp) Bk[k].assign(Bp + k * S2, Bp + (k + 1) * S2);
      else { Bk[k] = Q; for (int x = 0; x < S; ++x) Bk[k][(size_t)x * S + x] = 0.0; }
    }
    Mat A(S2), U;
    for (int x = 0; x < S; ++x)
      for (int y = 0; y < S; ++y) A[(size_t)x * S + y] = std::sqrt(pip[x]) * Q[(size_t)x * S + y] / std::sqrt(pip[y]);
    for (int x = 0; x < S; ++x)
      for (int y = x + 1; y < S; ++y) A[(size_t)x * S + y] = A[(size_t)y * S + x] = 0.5 * (A[(size_t)x * S + y] + A[(size_t)y * S + x]);
    Eig& e = eig[m];
    jacobi(S, A, &U, &e.lam);
    e.V.resize(S2); e.Vi.resize(S2);
    for (int x = 0; x < S; ++x)
      for (int j = 0; j < S; ++j) {
        e.V[(size_t)x * S + j] = U[(size_t)x * S + j] / std::sqrt(pip[x]);
        e.Vi[(size_t)j * S + x] = U[(size_t)x * S + j] * std::sqrt(pip[x]);
      }
    e.W.resize(K);   // Vinv B_k V
    for (int k = 0; k < K; ++k) e.W[k] = matmul(S, matmul(S, e.Vi, Bk[k]), e.V);
  }
  hm->eigV.clear(); hm->eigVi.clear(); hm->eigLam.clear();
  for (int m = 0; m < NM; ++m) {
    hm->eigV.insert(hm->eigV.end(), eig[m].V.begin(), eig[m].V.end());
    hm->eigVi.insert(hm->eigVi.end(), eig[m].Vi.begin(), eig[m].Vi.end());
    hm->eigLam.insert(hm->eigLam.end(), eig[m].lam.begin(), eig[m].lam.end());
  }
  return std::string();
}

// per (class, branch) matrices, each branch with its own generator
void build_branch_matrices(const cmx_model* model, const std::vector<Eig>& eig, HostModel* hm) {
  const int S = hm->S, C = hm->C, K = hm->K, B = hm->B;
  const size_t S2 = (size_t)S * S;
  const std::vector<int>& model_of = hm->model_of;
  hm->P.assign((size_t)C * B * S2, 0.0);
  hm->PN.assign((size_t)C * B * K * S2, 0.0);
  Mat E(S2), Phi(S2);
  // P(t) of branch b and, per substitution type, either P o N^k (the joint count operator of the averaged mapping) or the
  // conditional expectation N^k itself (nijt.average = no picks single entries of it)
  auto branch_mats = [&](int b, double t, double* P, double* outK /*[K][S2]*/, bool conditional, bool rate_zero) {
    const Eig& e = eig[model_of[b]];
    const Mat &V = e.V, &Vi = e.Vi;
    const std::vector<double>& lam = e.lam;
    const std::vector<Mat>& W = e.W;
    if (rate_zero) {
      // a rate-zero class (Invariant + Gamma): P = I exactly, and the rest below runs at t = 0 (J = 0).  V Vinv is I only
      // to rounding, with off-diagonals of either sign; a star of some 40 leaves multiplies them into vectors of mixed
      // signs, which break the rescaling rule of the scaled kernels (largest element of a non-negative vector; DESIGN.md
      // 2).  A zero-length branch under a positive rate keeps the eigen product and its bits.
      std::fill(P, P + S2, 0.0);
      for (int x = 0; x < S; ++x) P[(size_t)x * S + x] = 1.0;
    } else {
      for (int x = 0; x < S; ++x)
        for (int j = 0; j < S; ++j) E[(size_t)x * S + j] = V[(size_t)x * S + j] * std::exp(lam[j] * t);
      Mat Pm = matmul(S, E, Vi);
      std::memcpy(P, Pm.data(), sizeof(double) * S2);
    }
    for (int k = 0; k < K; ++k) {
      double* Ok = outK + (size_t)k * S2;
      if (model->count_method == CMX_COUNT_NAIVE) {
        for (size_t i = 0; i < S2; ++i) {
          const double nxy = (i / S == i % S) ? 0.0 : (model->naive_weights ? model->naive_weights[i] : 1.0);
          Ok[i] = conditional ? nxy : P[i] * nxy;
        }
        continue;
      }
      // J = V [ (Vinv B V) o Phi ] Vinv; Phi through expm1 (accurate O(t^2) diagonal on 1e-6 branches).
      // Saturated branches: e^{lam_j t} expm1(d) is (underflow) x (overflow) once d nears 709.78, and the Bio++ guard below
      // would then zero every count of the branch.  Phi is symmetric in (i, j), so above kPhiSymmetricAbove it is taken from
      // the larger eigenvalue, t e^{max(lam_i, lam_j) t} (-expm1(-|d|)) / |d|, finite for every t >= 0.  The threshold: at
      // d <= 680 expm1(d) is finite, and a term whose e^{lam_j t} has left the normal range (lam_j t < -708) has
      // lam_i t < -28, under 1e-12 of t; it stays above the d of every branch the suite and the benchmark have used so far
      // (t = 120 at rate 2.9 of JTT: d = 653), whose operators keep their bits.
      constexpr double kPhiSymmetricAbove = 680.0;
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) {
          const double d = (lam[i] - lam[j]) * t;
          const double phi = std::fabs(d) < 1e-14 ? t * std::exp(lam[i] * t)
                             : d > kPhiSymmetricAbove ? t * std::exp(lam[i] * t) * -std::expm1(-d) / d
                                                      : t * std::exp(lam[j] * t) * std::expm1(d) / d;
          Phi[(size_t)i * S + j] = W[k][(size_t)i * S + j] * phi;
        }
      Mat J = matmul(S, matmul(S, V, Phi), Vi);
      for (size_t i = 0; i < S2; ++i) {
        double nxy = J[i] / P[i];  // conditional count; Bio++ guards: non-finite -> 0, unweighted negatives -> 0
        if (std::isnan(nxy) || std::isinf(nxy)) nxy = 0.0;
        if (model->clamp_negative && nxy < 0.0) nxy = 0.0;
        Ok[i] = conditional ? nxy : P[i] * nxy;
        // An entry of P below P's own rounding (off-diagonals carry +-1e-17 ... 1e-15: a 1e-100 branch, rates of 1e-5 on
        // a 1e-12 branch) can come out <= 0, and the guards above then drop a positive J(x, y) from the joint operator,
        // which needs no quotient: keep J itself there.  P > 0 gives P (J / P) = J whatever P's error, so no other entry
        // moves.
        if (!conditional && model->clamp_negative && !(P[i] > 0.0) && J[i] > 0.0) Ok[i] = J[i];
        // A signed register keeps every finite quotient (P (J / P) = J for P < 0 too); only an entry of P that is exactly
        // 0 (a 1e-100 branch: the off-diagonals of V Vinv are multiples of 1e-17, now and then 0) has none, and lost
        // J(x, y) of either sign to the non-finite guard.
        if (!conditional && !model->clamp_negative && P[i] == 0.0) Ok[i] = J[i];
      }
    }
  };
  for (int c = 0; c < C; ++c)
    for (int b = 0; b < B; ++b)
      branch_mats(b, hm->blen[b] * hm->rates[c], &hm->P[((size_t)c * B + b) * S2], &hm->PN[((size_t)c * B + b) * K * S2], false, hm->rates[c] == 0.0);
  // N^k(x, y; t_b) at the branch length itself: computeSubstitutionVectorsNoAveraging reads single entries of it; and at
  // r_c t_b per class: computeSubstitutionVectorsMarginal weights it with the two marginal posteriors
  hm->N1.assign((size_t)B * K * S2, 0.0);
  hm->NC.assign((size_t)C * B * K * S2, 0.0);
  {
    Mat P1(S2);
    for (int b = 0; b < B; ++b) branch_mats(b, hm->blen[b], P1.data(), &hm->N1[(size_t)b * K * S2], true, false);
    for (int c = 0; c < C; ++c)
      for (int b = 0; b < B; ++b) branch_mats(b, hm->blen[b] * hm->rates[c], P1.data(), &hm->NC[((size_t)c * B + b) * K * S2], true, hm->rates[c] == 0.0);
  }
}

// MAT: per device class one ClassBlock (cmx_layout.h) of matrices of mat_unit(dS) doubles, the unit the kernel DMAs into
// LDS.  Here the operators of the branches; the cherry tables follow (build_cherry_tables).
void build_device_matrices(HostModel* hm) {
  const int S = hm->S, C = hm->C, K = hm->K, B = hm->B, F = hm->fuse;
  const size_t S2 = (size_t)S * S;
  const ClassBlock mats = hm->block();
  const int MC = hm->plain ? 0 : mats.count();
  hm->MC = MC;
  const int dS = S * F, dC = (C + F - 1) / F;
  hm->dS = dS;
  hm->dC = dC;
  const size_t MU = hm->plain ? 0 : (size_t)mat_unit(dS);   // doubles per device matrix: dS*dS plus max_ambig(dS) extra leaf rows
  const size_t dS2 = (size_t)dS * dS;
  hm->MAT.assign((size_t)dC * MC * MU, 0.0);
  Mat dense(dS2);
  for (int dc = 0; dc < (hm->plain ? 0 : dC); ++dc) {
    double* blk = &hm->MAT[(size_t)dc * MC * MU];
    for (int b = 0; b < B; ++b) {
      // operator of edge b for device class dc: diagonal blocks g = 0..F-1 <-> true class dc*F + g (classes beyond C
      // pad the last group: identity transition, zero weight).  which = -1: P, k >= 0: w_c (P o N^k), w_c = class
      // probability when fused (the kernel then uses weight 1 per pass), else 1.
      auto block = [&](int g, int which) -> const double* {
        const int c = dc * F + g;
        if (c >= C) return nullptr;
        return which < 0 ? &hm->P[((size_t)c * B + b) * S2] : &hm->PN[(((size_t)c * B + b) * K + which) * S2];
      };
      auto weight = [&](int g, int which) { return (which >= 0 && F > 1) ? hm->probs[dc * F + g] : 1.0; };
      if (hm->taxon_of[b] >= 0) {
        const int tx = hm->taxon_of[b];
        for (int which = -1; which < K; ++which) {
          double* lt = blk + (size_t)mats.leaf(tx, which) * MU;
          for (int g = 0; g < F; ++g) {
            const double* M = block(g, which);
            for (int x = 0; x < S; ++x)
              for (int z = 0; z < S; ++z) {  // row = observed state z, column = device state X = (class g, state x): transposed.
                lt[(size_t)z * leaf_row_stride(dS) + leaf_col(g * S + x, dS)] = M ? weight(g, which) * M[(size_t)x * S + z] : (which < 0 && x == z ? 1.0 : 0.0);
              }
          }
        }
      } else {
        const int sl = hm->slot[b];
        for (int which = -1; which < K; ++which) {
          std::fill(dense.begin(), dense.end(), 0.0);
          for (int g = 0; g < F; ++g) {
            const double* M = block(g, which);
            for (int x = 0; x < S; ++x)
              for (int y = 0; y < S; ++y)
                dense[(size_t)(g * S + x) * dS + g * S + y] =
                    M ? weight(g, which) * M[(size_t)x * S + y] : (which < 0 && x == y ? 1.0 : 0.0);
          }
          pack_blocks(dS, dense.data(), blk + (size_t)mats.internal(sl, which) * MU, F > 1);
        }
      }
    }
  }
}

// cherry tables: row 4 s1 + s2 (symbols of the cherry's leaves l1, l2), column X = (class g, state x) stored like a
// leaf row; class weights are folded into the count operators as everywhere in the fused layout
void build_cherry_tables(HostModel* hm) {
  if (hm->plain || hm->ncherry == 0) return;
  const int S = hm->S, C = hm->C, K = hm->K, B = hm->B, F = hm->fuse, nn = hm->nn, dS = hm->dS;
  const size_t S2 = (size_t)S * S, MU = (size_t)mat_unit(dS);
  const ClassBlock mats = hm->block();
  for (int dc = 0; dc < hm->dC; ++dc) {
    double* blk = &hm->MAT[(size_t)dc * hm->MC * MU];
    for (int n = 0; n < nn; ++n) {
      if (hm->cherry_of[n] < 0) continue;
      int l1 = -1, l2 = -1;
      for (int e = hm->first_child[n]; e >= 0; e = hm->next_sib[e]) { if (l1 < 0) l1 = e; else l2 = e; }
      double* tab = blk + (size_t)mats.cherry(hm->cherry_of[n], 0) * MU;
      for (int g = 0; g < F; ++g) {
        const int c = dc * F + g;
        for (int s1 = 0; s1 < S; ++s1)
          for (int s2 = 0; s2 < S; ++s2)
            for (int x = 0; x < S; ++x) {
              const size_t at = (size_t)(4 * s1 + s2) * leaf_row_stride(dS) + leaf_col(g * S + x, dS);
              if (c >= C) {   // padding class: identity transitions, zero weight -- message = [x == s1 == s2], no counts
                tab[at] = (x == s1 && x == s2) ? 1.0 : 0.0;
                for (int q = 1; q <= 3 * K; ++q) tab[(size_t)q * MU + at] = 0.0;
                continue;
              }
              const double w = hm->probs[c];
              const double* Pn = &hm->P[((size_t)c * B + n) * S2];
              const double* P1 = &hm->P[((size_t)c * B + l1) * S2];
              const double* P2 = &hm->P[((size_t)c * B + l2) * S2];
              double m = 0.0;
              for (int y = 0; y < S; ++y) m += Pn[(size_t)x * S + y] * P1[(size_t)y * S + s1] * P2[(size_t)y * S + s2];
              tab[at] = m;
              for (int k = 0; k < K; ++k) {
                const double* Jn = &hm->PN[(((size_t)c * B + n) * K + k) * S2];
                const double* J1 = &hm->PN[(((size_t)c * B + l1) * K + k) * S2];
                const double* J2 = &hm->PN[(((size_t)c * B + l2) * K + k) * S2];
                double tj = 0.0, t1 = 0.0, t2 = 0.0;
                for (int y = 0; y < S; ++y) {
                  tj += Jn[(size_t)x * S + y] * P1[(size_t)y * S + s1] * P2[(size_t)y * S + s2];
                  t1 += Pn[(size_t)x * S + y] * J1[(size_t)y * S + s1] * P2[(size_t)y * S + s2];
                  t2 += Pn[(size_t)x * S + y] * P1[(size_t)y * S + s1] * J2[(size_t)y * S + s2];
                }
                tab[(size_t)(1 + k) * MU + at] = w * tj;
                tab[(size_t)(1 + K + k) * MU + at] = w * t1;
                tab[(size_t)(1 + 2 * K + k) * MU + at] = w * t2;
              }
            }
      }
    }
  }
}

// simulator tables: running row sums of P with their guide table, running sums of pi and probs
void build_sim_tables(HostModel* hm) {
  const int S = hm->S, C = hm->C, B = hm->B, nn = hm->nn;
  const size_t S2 = (size_t)S * S;
  hm->CP.assign((size_t)C * nn * S2 + 4, 0.0);   // + 4: the fused simulator reads four running sums at a time
  for (int c = 0; c < C; ++c)
    for (int b = 0; b < B; ++b) {
      const double* P = &hm->P[((size_t)c * B + b) * S2];
      double* cp = &hm->CP[((size_t)c * nn + b) * S2];
      for (int x = 0; x < S; ++x) {
        double cum = 0.0;
        for (int y = 0; y < S; ++y) { cum += P[(size_t)x * S + y]; cp[(size_t)x * S + y] = cum; }
      }
    }
  // guide table of the simulator's inverse-CDF search: entry k of a row = the number of leading running sums that are
  // <= k/32, i.e. where the linear scan "index = #{j < S-1 : u >= cum[j]}" may start for any u in [k/32, (k+1)/32)
  hm->CPG.assign((size_t)C * nn * S * 32, 0);
  for (size_t r = 0; r < (size_t)C * nn * S; ++r) {
    const double* cum = &hm->CP[r * S];
    for (int k = 0; k < 32; ++k) {
      int st = 0;
      while (st < S - 1 && cum[st] <= k / 32.0) ++st;
      hm->CPG[r * 32 + k] = (uint8_t)st;
    }
  }
  // The chain kernel's copy.  A node draw is u = w / 2^32 of a 32-bit word w, and the search counts the running sums with
  // u >= cum, i.e. w >= cum * 2^32 (exact: a power of two), i.e. w > ceil(cum * 2^32) - 1 for an integer w: the threshold
  // kept here, 2^32 - 1 ("never") from cum >= 1 on and for the row's last sum and the padding, which the search does not
  // count.  A sum <= 0 ("always") has no such threshold and needs none: the guide starts every search behind the sums
  // that are <= k/32, k >= 0.  The thresholds of a row are made non-decreasing (rounding can leave the sums of a
  // zero-length branch out of order by an ulp): the search counts the thresholds below w wherever they stand, and on a
  // non-decreasing row that is where draw_guided's scan stops.
  hm->simtab.clear();
  if (sim_has_tables(S, C)) {
    const int rs = sim_thr_row(S);
    const size_t nodeb = sim_node_bytes(S, C), tabb = (size_t)C * S * rs * 4;
    hm->simtab.assign((size_t)nn * nodeb, 0);
    for (int b = 0; b < B; ++b)
      for (int c = 0; c < C; ++c)
        for (int x = 0; x < S; ++x) {
          const size_t r = ((size_t)c * nn + b) * S + x;
          uint32_t thr[kPlainStates + kSimThrPad + 3];
          for (int y = 0; y < rs; ++y) {
            const double t = y < S - 1 ? std::ceil(std::ldexp(hm->CP[r * S + y], 32)) - 1.0 : 4294967295.0;
            thr[y] = t <= 0.0 ? 0u : t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
            if (y > 0) thr[y] = std::max(thr[y], thr[y - 1]);
          }
          uint8_t* node = &hm->simtab[(size_t)b * nodeb];
          std::memcpy(node + ((size_t)c * S + x) * rs * 4, thr, (size_t)rs * 4);
          std::memcpy(node + tabb + ((size_t)c * S + x) * 32, &hm->CPG[r * 32], 32);
        }
  }
  hm->cum_pi.resize(S);
  hm->cum_probs.resize(C);
  double cum = 0.0;
  for (int x = 0; x < S; ++x) { cum += hm->pi[x]; hm->cum_pi[x] = cum; }
  cum = 0.0;
  for (int c = 0; c < C; ++c) { cum += hm->probs[c]; hm->cum_probs[c] = cum; }
}

}  // namespace

std::string build_host_model(const cmx_model* model, const cmx_tree* tree, HostModel* hm, int* code) {
  *code = CMX_ERR_INVALID;
  std::vector<Eig> eig;
  std::string bad = check_arguments(model, tree, hm, code);
  if (bad.empty()) bad = build_tree(tree, hm);
  if (!bad.empty()) return bad;
  build_walk_program(hm);
  build_sim_groups(hm);
  bad = check_model(model, hm);
  if (bad.empty()) bad = build_generators(model, hm, &eig);
  if (!bad.empty()) return bad;
  build_branch_matrices(model, eig, hm);
  build_device_matrices(hm);
  build_cherry_tables(hm);
  build_sim_tables(hm);
  if (!hm->plain) bad = verify_walk(*hm);
  if (!bad.empty()) return bad;
  *code = CMX_OK;
  return std::string();
}

}  // namespace cmx
