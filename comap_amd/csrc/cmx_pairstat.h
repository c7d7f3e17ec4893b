// Per-lane pair statistics shared by the mapping kernels (null mode), the diagonal-pair and the group kernels
// (CoMap/Statistics.h:164-329).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "cmx_device.h"

namespace cmx {

// per-lane statistic between two count columns (row strides ld1 / ld2), CoMap/Statistics.h
__device__ __forceinline__ double pair_stat_strided(int kind, double param, int B, int K, const double* __restrict__ c1,
                                                    size_t ld1, const double* __restrict__ c2, size_t ld2,
                                                    const double* __restrict__ mv = nullptr /* [2][B], CorrectedCorrelation */) {
  switch (kind) {
    case CMX_STAT_CORRELATION: case CMX_STAT_COVARIANCE: case CMX_STAT_CORRECTED_CORRELATION: {  // VectorTools::cor, two-pass on type 0
      // CorrectedCorrelation (Statistics.h:176-204) first subtracts a per-branch mean vector from either operand
      const double* u1 = kind == CMX_STAT_CORRECTED_CORRELATION ? mv : nullptr;
      const double* u2 = kind == CMX_STAT_CORRECTED_CORRELATION ? mv + B : nullptr;
      double m1 = 0, m2 = 0;
#pragma unroll 8
      for (int b = 0; b < B; ++b) {
        m1 += c1[(size_t)b * K * ld1] - (u1 ? u1[b] : 0.0);
        m2 += c2[(size_t)b * K * ld2] - (u2 ? u2[b] : 0.0);
      }
      m1 /= B; m2 /= B;
      double sxy = 0, sxx = 0, syy = 0;
#pragma unroll 8
      for (int b = 0; b < B; ++b) {
        const double dx = c1[(size_t)b * K * ld1] - (u1 ? u1[b] : 0.0) - m1, dy = c2[(size_t)b * K * ld2] - (u2 ? u2[b] : 0.0) - m2;
        sxy += dx * dy; sxx += dx * dx; syy += dy * dy;
      }
      const double cov = sxy / (B - 1);
      if (kind == CMX_STAT_COVARIANCE) return cov;
      return cov / (sqrt(sxx / (B - 1)) * sqrt(syy / (B - 1)));
    }
    case CMX_STAT_SCALAR_PRODUCT: {  // VectorTools::scalar
      double sxy = 0;
      for (int b = 0; b < B; ++b) sxy += c1[(size_t)b * K * ld1] * c2[(size_t)b * K * ld2];
      return sxy;
    }
    case CMX_STAT_COSINUS: {
      double sxy = 0, sxx = 0, syy = 0;
      for (int b = 0; b < B; ++b) {
        const double x = c1[(size_t)b * K * ld1], y = c2[(size_t)b * K * ld2];
        sxy += x * y; sxx += x * x; syy += y * y;
      }
      return sxy / (sqrt(sxx) * sqrt(syy));
    }
    case CMX_STAT_EUCLIDIAN_DISTANCE: {
      double d = 0;
      for (int b = 0; b < B; ++b) {
        double t1 = 0, t2 = 0;
        for (int k = 0; k < K; ++k) { t1 += c1[((size_t)b * K + k) * ld1]; t2 += c2[((size_t)b * K + k) * ld2]; }
        d = __builtin_fma(t2 - t1, t2 - t1, d);
      }
      return sqrt(d);
    }
    case CMX_STAT_COMPENSATION: case CMX_STAT_COSUBSTITUTION: case CMX_STAT_DISCRETE_MI: {
      double s1 = 0, s2 = 0, s3 = 0, cc = 0, n11 = 0, r1 = 0, r2 = 0;
      bool bad = false;
      for (int b = 0; b < B; ++b) {
        double t1 = 0, t2 = 0;
        for (int k = 0; k < K; ++k) { t1 += c1[((size_t)b * K + k) * ld1]; t2 += c2[((size_t)b * K + k) * ld2]; }
        s1 += t1 * t1; s2 += t2 * t2; s3 += (t1 + t2) * (t1 + t2);
        if (t1 >= 1.0 && t2 >= 1.0) cc += 1.0;
        if (!(t1 >= 0.0 && t1 < 10000.0) || !(t2 >= 0.0 && t2 < 10000.0)) bad = true;
        const double i1 = t1 >= param ? 1.0 : 0.0, i2 = t2 >= param ? 1.0 : 0.0;
        n11 += i1 * i2; r1 += i1; r2 += i2;
      }
      if (kind == CMX_STAT_COMPENSATION) return 1.0 - sqrt(s3) / (sqrt(s1) + sqrt(s2));
      if (kind == CMX_STAT_COSUBSTITUTION) return cc;
      if (bad) return __builtin_nan("");
      const double np = B;
      const double cell[4] = {n11, r1 - n11, r2 - n11, np - r1 - r2 + n11};
      const double ma[4] = {r1, r1, np - r1, np - r1}, mb[4] = {r2, np - r2, r2, np - r2};
      double s = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (cell[q] > 0) s += (cell[q] / np) * log(cell[q] * np / (ma[q] * mb[q]));
      return s / log(2.7182818);
    }
  }
  return __builtin_nan("");
}

// ---- Correlation / Covariance in one pass over the pair (the fused null's pattern table).
// pair_stat_strided's first pass and two of its three second-pass sums depend on one operand alone, so they are taken once
// per pattern (null_pattern_moments_kernel) -- in its order, with its expressions, the squares contracted into v_fma_f64 as the compiler contracts them
// there -- and a pair adds the cross products.  The statistic is the same bytes as pair_stat_strided's.  That rests on the
// build's -ffp-contract=fast (hipcc's default for device code), under which "sxx += dx * dx" in pair_stat_strided becomes one
// v_fma_f64; the explicit fma here pins this side only.  A build that stops contracting splits the two paths, and
// tests/test_gpu_null_patterns.py / test_gpu_null_pattern_tiles.py (bytes against the per-site path) say so.
__device__ __forceinline__ void pattern_moments(int B, int K, const double* __restrict__ c, size_t ld, double& mean, double& ss) {
  double m = 0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) m += c[(size_t)b * K * ld];
  m /= B;
  double sxx = 0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) {
    const double dx = c[(size_t)b * K * ld] - m;
    sxx = __builtin_fma(dx, dx, sxx);
  }
  mean = m;
  ss = sxx;
}

__device__ __forceinline__ double pair_stat_moments(int kind, int B, int K, const double* __restrict__ c1, size_t ld1, double m1,
                                                    double sxx, const double* __restrict__ c2, size_t ld2, double m2, double syy) {
  double sxy = 0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) {
    const double dx = c1[(size_t)b * K * ld1] - m1, dy = c2[(size_t)b * K * ld2] - m2;
    sxy = __builtin_fma(dx, dy, sxy);
  }
  const double cov = sxy / (B - 1);
  if (kind == CMX_STAT_COVARIANCE) return cov;
  return cov / (sqrt(sxx / (B - 1)) * sqrt(syy / (B - 1)));
}

// ---- per-branch weights (Statistic::setWeights, CoMap/Statistics.h:83-104; DESIGN A.7, weighted).  w is normalised
// (sum 1).  Every weighted kind is a plain sum of products of scaled operands X_b = weight_factor(kind, w_b) * value_b,
// on the lanes here and in the Gram operand of pair_prep_kernel alike, so a corrected reading of bpp-core's
// VectorTools changes this one line: Cosinus squares the weights (scalar(x, y, w) = sum w^2 x y and norm(x, w)),
// Correlation / Covariance / Compensation / EuclidianDistance take them once.
__device__ __forceinline__ double weight_factor(int kind, double w) { return kind == CMX_STAT_COSINUS ? w : sqrt(w); }

// weighted per-lane statistic (the kinds below; the others ignore weights as the reference does).  A function of
// its own: pair_stat_strided is inlined into map_kernel's null mode and stays as it is.
//   (Corrected)Correlation: VectorTools::cor(x, y, w, false) = sum w dx dy / sqrt(sum w dx^2 sum w dy^2), m = sum w x (no (B-1) factors)
//   Covariance:        VectorTools::cov(x, y, w, false, false) = sum w dx dy
//   Cosinus:           sum w^2 x y / (sqrt(sum w^2 x^2) sqrt(sum w^2 y^2))
//   Compensation:      1 - sqrt(sum w (t1 + t2)^2) / (sqrt(sum w t1^2) + sqrt(sum w t2^2))   (Statistics.h:255-264)
//   EuclidianDistance: sqrt(sum w (t2 - t1)^2)                                               (Distance.h:160-168)
__device__ inline double pair_stat_weighted(int kind, double param, int B, int K, const double* __restrict__ c1,
                                                  size_t ld1, const double* __restrict__ c2, size_t ld2,
                                                  const double* __restrict__ mv, const double* __restrict__ w) {
  switch (kind) {
    case CMX_STAT_CORRELATION: case CMX_STAT_COVARIANCE: case CMX_STAT_CORRECTED_CORRELATION: {
      const double* u1 = kind == CMX_STAT_CORRECTED_CORRELATION ? mv : nullptr;
      const double* u2 = kind == CMX_STAT_CORRECTED_CORRELATION ? mv + B : nullptr;
      double m1 = 0, m2 = 0;
      for (int b = 0; b < B; ++b) {
        m1 += w[b] * (c1[(size_t)b * K * ld1] - (u1 ? u1[b] : 0.0));
        m2 += w[b] * (c2[(size_t)b * K * ld2] - (u2 ? u2[b] : 0.0));
      }
      double sxy = 0, sxx = 0, syy = 0;
      for (int b = 0; b < B; ++b) {
        const double f = weight_factor(kind, w[b]);
        const double dx = f * (c1[(size_t)b * K * ld1] - (u1 ? u1[b] : 0.0) - m1), dy = f * (c2[(size_t)b * K * ld2] - (u2 ? u2[b] : 0.0) - m2);
        sxy += dx * dy; sxx += dx * dx; syy += dy * dy;
      }
      if (kind == CMX_STAT_COVARIANCE) return sxy;
      return sxy / (sqrt(sxx) * sqrt(syy));
    }
    case CMX_STAT_COSINUS: {
      double sxy = 0, sxx = 0, syy = 0;
      for (int b = 0; b < B; ++b) {
        const double f = weight_factor(kind, w[b]);
        const double x = f * c1[(size_t)b * K * ld1], y = f * c2[(size_t)b * K * ld2];
        sxy += x * y; sxx += x * x; syy += y * y;
      }
      return sxy / (sqrt(sxx) * sqrt(syy));
    }
    case CMX_STAT_COMPENSATION: case CMX_STAT_EUCLIDIAN_DISTANCE: {
      double s1 = 0, s2 = 0, s3 = 0, d = 0;
      for (int b = 0; b < B; ++b) {
        double t1 = 0, t2 = 0;
        for (int k = 0; k < K; ++k) { t1 += c1[((size_t)b * K + k) * ld1]; t2 += c2[((size_t)b * K + k) * ld2]; }
        const double f = weight_factor(kind, w[b]);
        t1 *= f; t2 *= f;
        s1 += t1 * t1; s2 += t2 * t2; s3 += (t1 + t2) * (t1 + t2);
        d = __builtin_fma(t2 - t1, t2 - t1, d);
      }
      if (kind == CMX_STAT_EUCLIDIAN_DISTANCE) return sqrt(d);
      return 1.0 - sqrt(s3) / (sqrt(s1) + sqrt(s2));
    }
  }
  return pair_stat_strided(kind, param, B, K, c1, ld1, c2, ld2, mv);
}

}  // namespace cmx
