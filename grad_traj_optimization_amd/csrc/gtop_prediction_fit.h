// gtop_prediction_fit.h — the arithmetic of the prediction fit (include/gtop_prediction.h) behind the sums: the local
// system, its Cholesky factor, the substitutions, the conversion to a row of the polynomial box list and the centre the
// residuals are taken at.  ONE statement for the kernel (gtop_prediction.hip) and the host form
// (gtop_capi_prediction.cpp): both include it with floating-point contraction off, every step is one rounded fp64
// operation in the order written, and the one fused step is the fma Horner of the consumers' centre.
//
// Every loop has constant bounds and every array index is a constant after unrolling, with the degree applied as a
// mask: on the device the arrays live in registers (no scratch).  Rows beyond the degree hold values nothing reads.
#ifndef GTOP_PREDICTION_FIT_H_
#define GTOP_PREDICTION_FIT_H_

#include <hip/hip_runtime.h>

#include <cmath>

#define GTOP_PRED_HD __host__ __device__ __forceinline__

constexpr int kPredInfo = 12;    // = GTOP_PRED_INFO
constexpr int kPredLocal = 20;   // = GTOP_PRED_LOCAL
constexpr int kPredChunk = 64;   // samples per chunk of the sums: one per lane
constexpr int kPredSums = 29;    // S_0 .. S_10, then M_{j,k} at 11 + 3 j + k
enum { kPredOk = 0, kPredLowered = 1, kPredEmpty = 2, kPredBad = 3 };
enum { kPredPolyfit = 0, kPredConstVel = 1 };

struct GtopPredictArgs {   // gtop_predict_opts as the kernel takes it
  int degree, regularise_horizon;
  double lambda, horizon, inflate;
};

GTOP_PRED_HD bool pred_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

// One sample's 29 terms: the powers s^0 .. s^10 by repeated product, and s^j q_k.
GTOP_PRED_HD void pred_terms(double s, const double q[3], double term[kPredSums]) {
  double pw = 1.0;
#pragma unroll
  for (int j = 0; j <= 10; ++j) {
    term[j] = pw;
    if (j <= 5) {
#pragma unroll
      for (int k = 0; k < 3; ++k) term[11 + 3 * j + k] = pw * q[k];
    }
    pw = pw * s;
  }
}

// The factor of the leading block of A_jk = S_{j+k} + [j, k >= 2] lam_e w_jk (e^p - (-1)^p), p = j + k - 3, row by
// row with left-to-right subtractions.  Returns the degree in force: deg0, or one below the first row whose pivot d is
// not > 2^-40 A_jj (the leading rows of the factor do not depend on the degree, so "lower it and factor again" is
// stopping there).  L: 6 x 6, lower triangle.
GTOP_PRED_HD int pred_factor(const double sums[kPredSums], double lam_e, double e, int deg0, double L[6][6]) {
  double ep[8];
  ep[0] = 1.0;
#pragma unroll
  for (int p = 1; p < 8; ++p) ep[p] = ep[p - 1] * e;
  int deg = deg0;
  bool live = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double ajj = 0.0;
#pragma unroll
    for (int k = 0; k <= j; ++k) {
      double a = sums[j + k];
      if (j >= 2 && k >= 2) {
        const int p = j + k - 3;
        const double w = (double)(j * (j - 1) * k * (k - 1)) / (double)p;
        const double d = ep[p] - ((p & 1) ? -1.0 : 1.0);
        a = a + (lam_e * w) * d;
      }
      if (k == j) ajj = a;
      double acc = a;
#pragma unroll
      for (int p = 0; p < k; ++p) acc = acc - L[j][p] * L[k][p];
      if (k < j) {
        L[j][k] = acc / L[k][k];
      } else {
        if (live && j <= deg && !(acc > 0x1p-40 * ajj)) {
          deg = j - 1;
          live = false;
        }
        L[j][j] = sqrt(acc);
      }
    }
  }
  return deg;
}

// g_0 .. g_deg of one axis from b (higher entries 0): forward, then back; each sum left to right in ascending index.
GTOP_PRED_HD void pred_substitute(const double L[6][6], int deg, const double b[6], double g[6]) {
  double y[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double acc = b[j];
#pragma unroll
    for (int p = 0; p < j; ++p) acc = acc - L[j][p] * y[p];
    y[j] = acc / L[j][j];
  }
#pragma unroll
  for (int j = 5; j >= 0; --j) {
    double acc = y[j];
#pragma unroll
    for (int p = j + 1; p < 6; ++p)
      if (p <= deg) acc = acc - L[p][j] * g[p];
    g[j] = j <= deg ? acc / L[j][j] : 0.0;
  }
}

// a_j = g_j / sigma^j (sigma^j by repeated product), then the Taylor shift to absolute time.
GTOP_PRED_HD void pred_to_row(const double g[6], double sigma, double t_last, double c[6]) {
  double sp = 1.0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    c[j] = g[j] / sp;
    sp = sp * sigma;
  }
  const double x0 = -t_last;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 4; j >= i; --j) c[j] = c[j] + c[j + 1] * x0;
  }
}

// The consumers' centre (gtop_box_poly_centre of gtop_edt_lookup.h) at an unclamped time.
GTOP_PRED_HD double pred_centre(const double c[6], double t) {
  return fma(fma(fma(fma(fma(c[5], t, c[4]), t, c[3]), t, c[2]), t, c[1]), t, c[0]);
}

GTOP_PRED_HD bool pred_all_finite6(const double v[6]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) ok = ok && pred_finite(v[j]);
  return ok;
}

#endif  // GTOP_PREDICTION_FIT_H_
