// gtop_capi_time.cpp — the entry points of the companion header include/gtop_time.h: the derivative of the cost with
// respect to the segment times and the optimizer of the time allocation (gtop_time.hip), each in a device form (no
// allocation, no synchronisation: capturable) and a host form over the problem set.
#include <cmath>

#include "gtop_capi_time.h"

int gtop_time_ready(gtop_ctx *c, const char *who, int B, int m, int time_stride, bool refuse_moving) {
  if (!c->have_params) return fail(c, GTOP_ERR_STATE, "gtop_set_params has not been called");
  if (!c->field.have_grid) return fail(c, GTOP_ERR_STATE, "no distance field set");
  if (refuse_moving && c->moving_cost != 0)
    return fail(c, GTOP_ERR_STATE, std::string(who) + ": the moving-obstacle cost is switched on; under absolute sample "
                                                      "times a segment time moves every later segment's lookups, "
                                                      "which this derivative does not form");
  if (B < 0 || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, std::string(who) + ": need B >= 0, 2 <= m <= 227, time_stride in {0, m}");
  return GTOP_OK;
}

int gtop_check_timeopt(gtop_ctx *c, const gtop_timeopt *o) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "optimize_times: options is NULL");
  if (o->reserved != 0) return fail(c, GTOP_ERR_INVALID, "optimize_times: reserved must be 0");
  if (!(o->rho >= 0.0) || !std::isfinite(o->rho))
    return fail(c, GTOP_ERR_INVALID, "optimize_times: rho must be finite and >= 0");
  if (!(o->t_min >= 0.0301) || !(o->t_min <= o->t_max) || !std::isfinite(o->t_max))
    return fail(c, GTOP_ERR_INVALID, "optimize_times: need 0.0301 <= t_min <= t_max, both finite");
  if (!(o->first_move > 0.0) || !std::isfinite(o->first_move))
    return fail(c, GTOP_ERR_INVALID, "optimize_times: first_move must be finite and > 0");
  if (!(o->ftol_rel >= 0.0) || !(o->xtol_abs >= 0.0))
    return fail(c, GTOP_ERR_INVALID, "optimize_times: ftol_rel and xtol_abs must be >= 0");
  if (o->max_evals < 1) return fail(c, GTOP_ERR_INVALID, "optimize_times: max_evals must be >= 1");
  return GTOP_OK;
}

GtopTimeCost gtop_time_cost(const gtop_ctx *c) {
  const gtop_params &p = c->prm;
  return {p.ws, p.wc, p.alpha, p.r, p.d0, p.alpha_v, p.r_v, p.v0, p.alpha_a, p.r_a, p.a0, p.step, p.enable_dyn};
}

namespace {

int gradient_on_stream(gtop_ctx *c, int B, int m, const void *d_x, const void *d_Df, const void *d_T, int time_stride,
                       void *d_cost, void *d_gT, void *d_parts, void *hip_stream) {
  if (int rc = gtop_time_ready(c, "time_gradient", B, m, time_stride, true)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_cost || !d_gT) return fail(c, GTOP_ERR_INVALID, "time_gradient: NULL buffer");
  if (int rc = c->field.need_records64(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_time_gradient(c->field.grid, c->field.rec64.data(), gtop_time_cost(c), B, m,
                                      static_cast<const double *>(d_x), static_cast<const double *>(d_Df),
                                      static_cast<const double *>(d_T), time_stride, static_cast<double *>(d_cost),
                                      static_cast<double *>(d_gT), static_cast<double *>(d_parts),
                                      static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

int optimize_on_stream(gtop_ctx *c, const gtop_timeopt *o, int B, int m, const void *d_x, const void *d_Df,
                       const void *d_T, int time_stride, const void *d_T_lo, void *d_T_out, void *d_info,
                       void *hip_stream) {
  if (int rc = gtop_check_timeopt(c, o)) return rc;
  if (int rc = gtop_time_ready(c, "optimize_times", B, m, time_stride, true)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_T_out || !d_info) return fail(c, GTOP_ERR_INVALID, "optimize_times: NULL buffer");
  if (d_T_out == d_T) return fail(c, GTOP_ERR_INVALID, "optimize_times: T_out may not alias T");
  if (int rc = c->field.need_records64(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_time_optimize(c->field.grid, c->field.rec64.data(), gtop_time_cost(c), o->rho, o->t_min, o->t_max,
                                      o->first_move, o->ftol_rel, o->xtol_abs, o->max_evals, B, m,
                                      static_cast<const double *>(d_x), static_cast<const double *>(d_Df),
                                      static_cast<const double *>(d_T), time_stride, static_cast<const double *>(d_T_lo),
                                      static_cast<double *>(d_T_out), static_cast<double *>(d_info),
                                      static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_time_abi_version(void) { return GTOP_TIME_ABI_VERSION; }

int gtop_time_gradient_device(gtop_ctx *c, int B, int m, const void *d_x, const void *d_Df, const void *d_T,
                              int time_stride, void *d_cost, void *d_gT, void *d_parts, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return gradient_on_stream(c, B, m, d_x, d_Df, d_T, time_stride, d_cost, d_gT, d_parts, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_time_gradient_batch(gtop_ctx *c, int B, const double *x, double *cost, double *gT, double *parts) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && cost && gT, "time_gradient_batch: 1 <= B <= problem batch; x, cost and gT required")))
    return rc;
  const int m = c->m;
  if ((rc = gtop_time_ready(c, "time_gradient_batch", B, m, c->t_stride, true))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), nT = (size_t)B * m;
  // the segment staging: cost | gT | parts
  HIPCHK(c, c->seg_rep.reserve((size_t)B + nT * (1 + GTOP_TIME_PARTS)));
  double *d_cost = c->seg_rep.data(), *d_gT = d_cost + B, *d_parts = d_gT + nT;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = gradient_on_stream(c, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, d_cost, d_gT,
                               parts ? d_parts : nullptr, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(cost, d_cost, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(gT, d_gT, nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (parts)
    HIPCHK(c, hipMemcpyAsync(parts, d_parts, nT * GTOP_TIME_PARTS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_optimize_times_device(gtop_ctx *c, const gtop_timeopt *opt, int B, int m, const void *d_x, const void *d_Df,
                               const void *d_T, int time_stride, const void *d_T_lo, void *d_T_out, void *d_info,
                               void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return optimize_on_stream(c, opt, B, m, d_x, d_Df, d_T, time_stride, d_T_lo, d_T_out, d_info, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_optimize_times(gtop_ctx *c, const gtop_timeopt *opt, int B, const double *x, const double *T_lo, double *T_out,
                        double *info) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_check_timeopt(c, opt))) return rc;
  if ((rc = gtop_problem_rows(c, B, x && T_out && info, "optimize_times: 1 <= B <= problem batch; x, T_out and info required")))
    return rc;
  const int m = c->m;
  if ((rc = gtop_time_ready(c, "optimize_times", B, m, c->t_stride, true))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), nT = (size_t)B * m, nI = (size_t)B * GTOP_TIMEOPT_INFO;
  // the segment staging: T_lo | T_out | info
  HIPCHK(c, c->seg_rep.reserve(2 * nT + nI));
  double *d_lo = c->seg_rep.data(), *d_Tout = d_lo + nT, *d_info = d_Tout + nT;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (T_lo) HIPCHK(c, hipMemcpyAsync(d_lo, T_lo, nT * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = optimize_on_stream(c, opt, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride,
                               T_lo ? d_lo : nullptr, d_Tout, d_info, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(T_out, d_Tout, nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info, d_info, nI * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
