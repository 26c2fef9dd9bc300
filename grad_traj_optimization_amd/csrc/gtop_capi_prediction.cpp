// gtop_capi_prediction.cpp — the entry points of the companion header include/gtop_prediction.h: predictions fitted
// from observation histories (gtop_prediction.hip) into the caller's buffers or straight into the context's polynomial
// box list (no allocation, no synchronisation: capturable), and the host form with the same bits.
#include <cmath>
#include <cstdint>

#include "gtop_ctx.h"
#include "gtop_prediction.h"

// The host form restates the kernel's sums serially and shares everything behind them (gtop_prediction_fit.h): every
// step ONE rounded fp64 operation, so nothing here may be contracted.
#pragma clang fp contract(off)

#include "gtop_prediction_fit.h"

static_assert(GTOP_PRED_INFO == kPredInfo && GTOP_PRED_LOCAL == kPredLocal, "the public row sizes are the kernel's own");
static_assert(GTOP_PRED_OK == kPredOk && GTOP_PRED_LOWERED == kPredLowered && GTOP_PRED_EMPTY == kPredEmpty &&
              GTOP_PRED_BAD == kPredBad && GTOP_PREDICT_POLYFIT == kPredPolyfit && GTOP_PREDICT_CONST_VEL == kPredConstVel,
              "the public codes are the kernel's own");

namespace {

// the options' rules; NULL = fine
const char *check_predict_opts(const gtop_predict_opts *o) {
  if (!o) return "predictions: options is NULL";
  if (o->reserved != 0) return "predictions: reserved must be 0";
  if (o->mode != GTOP_PREDICT_POLYFIT && o->mode != GTOP_PREDICT_CONST_VEL) return "predictions: mode is neither POLYFIT nor CONST_VEL";
  if (o->degree < 1 || o->degree > 5) return "predictions: need 1 <= degree <= 5";
  if (!(std::isfinite(o->lambda) && o->lambda >= 0.0)) return "predictions: lambda must be finite and >= 0";
  if (!(o->horizon >= 0.0)) return "predictions: horizon must be >= 0 (+inf allowed)";
  if (!(std::isfinite(o->inflate) && o->inflate >= 0.0)) return "predictions: inflate must be finite and >= 0";
  if (o->regularise_horizon != 0 && o->regularise_horizon != 1) return "predictions: regularise_horizon must be 0 or 1";
  if (o->regularise_horizon && std::isinf(o->horizon)) return "predictions: regularise_horizon needs a finite horizon";
  return nullptr;
}

GtopPredictArgs predict_args(const gtop_predict_opts *o) {
  return {o->degree, o->regularise_horizon, o->lambda, o->horizon, o->inflate};
}

// what both device entries ask of their shared arguments
int predictions_ready(gtop_ctx *c, int N, int H, const void *d_hist, const void *d_count, const gtop_predict_opts *o,
                      bool outputs) {
  if (const char *why = check_predict_opts(o)) return fail(c, GTOP_ERR_INVALID, why);
  if (N < 0 || H < 1) return fail(c, GTOP_ERR_INVALID, "predictions: need N >= 0 and H >= 1");
  if (N > 0 && (!d_hist || !d_count || !outputs)) return fail(c, GTOP_ERR_INVALID, "predictions: NULL buffer");
  if (reinterpret_cast<uintptr_t>(d_hist) % 16 != 0)
    return fail(c, GTOP_ERR_INVALID, "predictions: the history buffer must be 16-byte aligned");
  return GTOP_OK;
}

// ---- the host form ----
// One chunk of up to 64 values by the balanced pair tree, missing places +0.0.
double tree_sum(const double *v, int n) {
  double lane[kPredChunk];
  for (int i = 0; i < kPredChunk; ++i) lane[i] = i < n ? v[i] : 0.0;
  for (int width = kPredChunk; width > 1; width /= 2)
    for (int i = 0; i < width / 2; ++i) lane[i] = lane[2 * i] + lane[2 * i + 1];
  return lane[0];
}

struct Sample {
  double v[4];
};

// One object: returns the status; coef [18], t_range [2], local [20] (may be NULL) written only when it was fitted.
int fit_one(int H, const double *hist_n, int raw, int head, int mode, const GtopPredictArgs &o, double *coef,
            double *t_range, double *info, double *local) {
  const int cnt = raw < 0 ? 0 : (raw > H ? H : raw);
  for (int q = 0; q < kPredInfo; ++q) info[q] = 0.0;
  info[1] = (double)cnt;
  const auto give_up = [&](int status) {
    info[0] = (double)status;
    return status;
  };
  if (cnt != raw) return give_up(kPredBad);
  if (cnt == 0) return give_up(kPredEmpty);
  int hm = head % H;
  if (hm < 0) hm += H;
  const auto sample = [&](int i) {
    int slot = hm + i;
    if (slot >= H) slot -= H;
    return hist_n + 4 * (size_t)slot;
  };
  for (int i = 0; i < cnt; ++i)
    for (int a = 0; a < 4; ++a)
      if (!pred_finite(sample(i)[a])) return give_up(kPredBad);
  const double *first = sample(0), *last = sample(cnt - 1);
  const double t_first = first[3], t_last = last[3];
  if (cnt >= 2 && !(t_last - t_first > 0.0)) return give_up(kPredBad);

  int status = kPredOk, deg = 0;
  double g[3][6] = {}, c[3][6] = {}, sigma = 0.0, t_start = t_first;
  if (cnt == 1) {
    status = kPredLowered;
    t_start = t_last;
    for (int k = 0; k < 3; ++k) g[k][0] = c[k][0] = last[k];
  } else if (mode == kPredConstVel) {
    const double *prev = sample(cnt - 2);
    if (!(prev[3] < t_last)) return give_up(kPredBad);
    deg = 1;
    t_start = prev[3];
    sigma = t_last - prev[3];
    for (int k = 0; k < 3; ++k) {
      g[k][0] = last[k];
      g[k][1] = last[k] - prev[k];
      c[k][1] = g[k][1] / sigma;
      c[k][0] = last[k] - c[k][1] * t_last;
    }
  } else {
    sigma = t_last - t_first;
    double sums[kPredSums] = {};
    double term[kPredChunk][kPredSums], col[kPredChunk];
    for (int base = 0; base < cnt; base += kPredChunk) {
      const int nb = cnt - base < kPredChunk ? cnt - base : kPredChunk;
      for (int i = 0; i < nb; ++i) {
        const double *smp = sample(base + i);
        pred_terms((smp[3] - t_last) / sigma, smp, term[i]);
      }
      for (int q = 0; q < kPredSums; ++q) {
        for (int i = 0; i < nb; ++i) col[i] = term[i][q];
        sums[q] = sums[q] + tree_sum(col, nb);
      }
    }
    const double e = o.regularise_horizon ? o.horizon / sigma : 0.0;
    const double lam_e = o.lambda / ((sigma * sigma) * sigma);
    double L[6][6] = {};
    deg = pred_factor(sums, lam_e, e, o.degree < cnt - 1 ? o.degree : cnt - 1, L);
    if (deg < o.degree) status = kPredLowered;
    for (int k = 0; k < 3; ++k) {
      double b[6];
      for (int j = 0; j < 6; ++j) b[j] = sums[11 + 3 * j + k];
      pred_substitute(L, deg, b, g[k]);
    }
    for (int k = 0; k < 3; ++k)
      if (!pred_all_finite6(g[k])) return give_up(kPredBad);
    for (int k = 0; k < 3; ++k) pred_to_row(g[k], sigma, t_last, c[k]);
  }
  for (int k = 0; k < 3; ++k)
    if (!pred_all_finite6(c[k])) return give_up(kPredBad);

  double resmax[3] = {0.0, 0.0, 0.0}, esum = 0.0, sq[kPredChunk];
  for (int base = 0; base < cnt; base += kPredChunk) {
    const int nb = cnt - base < kPredChunk ? cnt - base : kPredChunk;
    for (int i = 0; i < nb; ++i) {
      const double *smp = sample(base + i);
      double r[3];
      for (int k = 0; k < 3; ++k) {
        r[k] = pred_centre(c[k], smp[3]) - smp[k];
        resmax[k] = std::fmax(resmax[k], std::fabs(r[k]));
      }
      sq[i] = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    }
    esum = esum + tree_sum(sq, nb);
  }
  const double t_end = t_last + o.horizon;
  info[0] = (double)status;
  info[2] = (double)deg;
  info[3] = t_start;
  info[4] = t_last;
  info[5] = t_end;
  for (int k = 0; k < 3; ++k) info[6 + k] = resmax[k];
  info[9] = std::sqrt(esum / (double)(3 * (long long)cnt));
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 6; ++j) coef[6 * k + j] = c[k][j];
  t_range[0] = t_start;
  t_range[1] = t_end;
  if (local) {
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 6; ++j) local[6 * k + j] = g[k][j];
    local[18] = t_last;
    local[19] = sigma;
  }
  return status;
}

}  // namespace

extern "C" {

int gtop_pred_abi_version(void) { return GTOP_PRED_ABI_VERSION; }

int gtop_fit_predictions_device(gtop_ctx *c, int N, int H, const void *d_hist, const void *d_count, const void *d_head,
                                const gtop_predict_opts *opts, void *d_coef, void *d_t_range, void *d_info, void *d_local,
                                void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = predictions_ready(c, N, H, d_hist, d_count, opts, d_coef && d_t_range && d_info)) return rc;
  if (N == 0) return GTOP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_fit_predictions(opts->mode, N, H, static_cast<const double *>(d_hist),
                                        static_cast<const int *>(d_count), static_cast<const int *>(d_head),
                                        predict_args(opts), static_cast<double *>(d_coef), static_cast<double *>(d_t_range),
                                        static_cast<double *>(d_info), static_cast<double *>(d_local),
                                        static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_refresh_box_predictions_device(gtop_ctx *c, int N, int H, const void *d_hist, const void *d_count,
                                        const void *d_head, const gtop_predict_opts *opts, const void *d_scale,
                                        void *d_info, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = predictions_ready(c, N, H, d_hist, d_count, opts, d_info != nullptr)) return rc;
  if (c->box_kind != GTOP_BOXES_POLYNOMIAL || c->nbox != N || N == 0)
    return fail(c, GTOP_ERR_STATE, "refresh_box_predictions: needs a polynomial box list (gtop_set_moving_box_polynomials) "
                                   "of exactly N boxes in force");
  HIPCHK(c, hipSetDevice(c->device));
  // the rows the cost bodies read follow when the list fits them (gtop_set_moving_box_polynomials filled them then)
  double *cost_rows = N <= GTOP_MOVING_COST_MAX_BOXES ? c->box_rows.data() : nullptr;
  HIPCHK(c, gtop_launch_refresh_predictions(opts->mode, N, H, static_cast<const double *>(d_hist),
                                            static_cast<const int *>(d_count), static_cast<const int *>(d_head),
                                            predict_args(opts), static_cast<const double *>(d_scale), c->boxes.data(),
                                            cost_rows, static_cast<double *>(d_info),
                                            static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_fit_predictions(int N, int H, const double *hist, const int32_t *count, const int32_t *head,
                         const gtop_predict_opts *opts, double *coef, double *t_range, double *info, double *local) try {
  if (check_predict_opts(opts) || N < 0 || H < 1) return GTOP_ERR_INVALID;
  if (N > 0 && (!hist || !count || !coef || !t_range || !info)) return GTOP_ERR_INVALID;
  const GtopPredictArgs o = predict_args(opts);
  for (int n = 0; n < N; ++n)
    fit_one(H, hist + (size_t)n * H * 4, count[n], head ? head[n] : 0, opts->mode, o, coef + 18 * (size_t)n,
            t_range + 2 * (size_t)n, info + kPredInfo * (size_t)n, local ? local + kPredLocal * (size_t)n : nullptr);
  return GTOP_OK;
} GTOP_CATCH_STATUS(static_cast<gtop_ctx *>(nullptr))

}  // extern "C"
