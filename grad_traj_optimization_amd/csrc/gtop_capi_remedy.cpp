// gtop_capi_remedy.cpp — the two remedies for a row that fails its report or certificate: the segment-time reallocation
// (gtop_retime.hip) and the waypoint insertion (gtop_insert.hip).  Each in a device form (no allocation, no
// synchronisation: capturable) and a host form over the problem set.
#include <cmath>
#include <string>

#include "gtop_ctx.h"

namespace {

// the rules of a gtop_retime, before anything is staged or launched
int check_retime(gtop_ctx *c, const gtop_retime *o) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "reallocate_times: options is NULL");
  if (o->mode == GTOP_RETIME_LENGTH) {
    if (!(o->mean_v > 0.0) || !std::isfinite(o->mean_v) || !(o->init_time >= 0.0) || !std::isfinite(o->init_time))
      return fail(c, GTOP_ERR_INVALID, "reallocate_times: LENGTH needs a finite mean_v > 0 and a finite init_time >= 0");
  } else if (o->mode == GTOP_RETIME_LIMITS) {
    if (!(o->max_ratio >= 1.0) || !std::isfinite(o->max_ratio))
      return fail(c, GTOP_ERR_INVALID, "reallocate_times: LIMITS needs a finite max_ratio >= 1");
  } else {
    return fail(c, GTOP_ERR_INVALID, "reallocate_times: unknown mode");
  }
  return GTOP_OK;
}

// the rules of a gtop_insert and of a call of B rows of m segments, before anything is staged or launched; which of the
// optional buffers are given: bounds (lb and ub), bounds_out (lb_out and ub_out)
int insert_ready(gtop_ctx *c, const gtop_insert *o, int B, int m, int time_stride, int when_stride, bool has_lb,
                 bool has_ub, bool has_lb_out, bool has_ub_out) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "insert_waypoints: options is NULL");
  if (o->mode != GTOP_INSERT_AT_TIME && o->mode != GTOP_INSERT_LONGEST)
    return fail(c, GTOP_ERR_INVALID, "insert_waypoints: unknown mode");
  if (o->reserved != 0) return fail(c, GTOP_ERR_INVALID, "insert_waypoints: reserved must be 0");
  if (!(o->min_fraction > 0.0 && o->min_fraction <= 0.5))
    return fail(c, GTOP_ERR_INVALID, "insert_waypoints: min_fraction must lie in (0, 0.5]");
  if (!std::isfinite(o->push) || !std::isfinite(o->push_below))
    return fail(c, GTOP_ERR_INVALID, "insert_waypoints: push and push_below must be finite");
  if (has_lb != has_ub) return fail(c, GTOP_ERR_INVALID, "insert_waypoints: lb and ub go together");
  if (has_lb_out != has_ub_out || has_lb_out != has_lb)
    return fail(c, GTOP_ERR_INVALID, "insert_waypoints: lb_out and ub_out are required exactly when lb and ub are given");
  if (has_lb)
    for (double v : {o->bos, o->vos, o->aos})
      if (!(std::isfinite(v) && v >= 0.0))
        return fail(c, GTOP_ERR_INVALID, "insert_waypoints: bos, vos and aos must be finite and >= 0");
  if (B < 0 || m < 2 || m > 226 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "insert_waypoints: need B >= 0, 2 <= m <= 226, time_stride in {0, m}");
  if (o->mode == GTOP_INSERT_AT_TIME && when_stride < 1)
    return fail(c, GTOP_ERR_INVALID, "insert_waypoints: AT_TIME needs when_stride >= 1");
  return o->push > 0.0 ? c->field.need_records64(c) : GTOP_OK;
}

}  // namespace

extern "C" {

// ---- segment-time reallocation (gtop_retime.hip) ----
int gtop_reallocate_times_device(gtop_ctx *c, const gtop_retime *opt, int B, int m, void *d_x, const void *d_Df,
                                 const void *d_T, int time_stride, const void *d_seg_report, void *d_T_out,
                                 void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = check_retime(c, opt)) return rc;
  if (B < 0 || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "reallocate_times: need B >= 0, 2 <= m <= 227, time_stride in {0, m}");
  if (B == 0) return GTOP_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  double *T_out = static_cast<double *>(d_T_out);
  if (opt->mode == GTOP_RETIME_LENGTH) {
    if (!d_x || !d_Df || !d_T_out) return fail(c, GTOP_ERR_INVALID, "reallocate_times: NULL buffer (LENGTH: x, Df, T_out)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, gtop_launch_retime_length(B, m, static_cast<const double *>(d_x), static_cast<const double *>(d_Df),
                                        opt->mean_v, opt->init_time, T_out, s));
    return GTOP_OK;
  }
  if (!d_T || !d_seg_report || !d_T_out || (opt->scale_x && !d_x))
    return fail(c, GTOP_ERR_INVALID, "reallocate_times: NULL buffer (LIMITS: T, seg_report, T_out; x with scale_x)");
  if (d_T_out == d_T && time_stride == 0 && B > 1)
    return fail(c, GTOP_ERR_INVALID, "reallocate_times: a shared time vector cannot be its own per-trajectory output");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_retime_limits(B, m, static_cast<double *>(d_x), static_cast<const double *>(d_T), time_stride,
                                      static_cast<const double *>(d_seg_report), opt->max_vel, opt->max_acc,
                                      opt->max_ratio, opt->per_axis != 0, opt->uniform != 0, opt->scale_x != 0, T_out, s));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_reallocate_times(gtop_ctx *c, const gtop_retime *opt, int B, double *x, double dt_sample,
                          const gtop_limits *limits, double *T_out) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_set(c))) return rc;
  if ((rc = check_retime(c, opt))) return rc;
  if ((rc = gtop_problem_rows(c, B, x && T_out, "reallocate_times: 1 <= B <= problem batch, x and T_out required")))
    return rc;
  const int m = c->m;
  const size_t n = 9 * (size_t)(m - 1), nT = (size_t)B * m;
  const bool limits_mode = opt->mode == GTOP_RETIME_LIMITS;
  if (limits_mode && (rc = gtop_validate_ready(c, B, m, c->t_stride, dt_sample, limits, c->B))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (limits_mode) {
    if ((rc = gtop_segments_staged(c, B, x, dt_sample, limits))) return rc;
  } else {
    HIPCHK(c, c->seg_rep.reserve(nT * (GTOP_SEG_REPORT + 1)));
    HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  double *d_seg = c->seg_rep.data(), *d_Tout = d_seg + nT * GTOP_SEG_REPORT;
  if ((rc = gtop_reallocate_times_device(c, opt, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, d_seg,
                                         d_Tout, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(T_out, d_Tout, nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (limits_mode && opt->scale_x)
    HIPCHK(c, hipMemcpyAsync(x, c->d_x.data(), (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- waypoint insertion (gtop_insert.hip) ----
int gtop_insert_waypoints_device(gtop_ctx *c, const gtop_insert *opt, int B, int m, const void *d_x, const void *d_coeff,
                                 const void *d_T, int time_stride, const void *d_when, int when_stride, const void *d_lb,
                                 const void *d_ub, void *d_x_out, void *d_T_out, void *d_lb_out, void *d_ub_out,
                                 void *d_info, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = insert_ready(c, opt, B, m, time_stride, when_stride, d_lb, d_ub, d_lb_out, d_ub_out)) return rc;
  if (B == 0) return GTOP_OK;
  const bool at_time = opt->mode == GTOP_INSERT_AT_TIME;
  if (!d_x || !d_coeff || !d_T || !d_x_out || !d_T_out || (at_time && !d_when))
    return fail(c, GTOP_ERR_INVALID, "insert_waypoints: NULL buffer (x, coeff, T, x_out, T_out; when under AT_TIME)");
  HIPCHK(c, hipSetDevice(c->device));
  const bool push = opt->push > 0.0;
  HIPCHK(c, gtop_launch_insert_waypoints(c->field.grid, push ? c->field.rec64.data() : nullptr, opt->mode,
                                         opt->min_fraction, opt->push, opt->push_below, opt->bos, opt->vos, opt->aos, B, m,
                                         static_cast<const double *>(d_x), static_cast<const double *>(d_coeff),
                                         static_cast<const double *>(d_T), time_stride,
                                         at_time ? static_cast<const double *>(d_when) : nullptr, at_time ? when_stride : 0,
                                         static_cast<const double *>(d_lb), static_cast<const double *>(d_ub),
                                         static_cast<double *>(d_x_out), static_cast<double *>(d_T_out),
                                         static_cast<double *>(d_lb_out), static_cast<double *>(d_ub_out),
                                         static_cast<double *>(d_info), static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_insert_waypoints(gtop_ctx *c, const gtop_insert *opt, int B, const double *x, const double *when,
                          const double *lb, const double *ub, double *x_out, double *T_out, double *lb_out,
                          double *ub_out, double *info) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_set(c))) return rc;
  const int m = c->m;
  if ((rc = insert_ready(c, opt, B, m, c->t_stride, 1, lb, ub, lb_out, ub_out))) return rc;   // (before anything is staged)
  const bool at_time = opt->mode == GTOP_INSERT_AT_TIME;
  if ((rc = gtop_problem_rows(c, B, x && x_out && T_out && (!at_time || when),
                              "insert_waypoints: 1 <= B <= problem batch; x, x_out and T_out required, when under AT_TIME")))
    return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n_old = (size_t)B * 9 * (m - 1), n_new = (size_t)B * 9 * m, n_T = (size_t)B * (m + 1);
  const size_t n_info = (size_t)B * GTOP_INSERT_INFO;
  // when | lb | ub | x_out | T_out | lb_out | ub_out | info
  HIPCHK(c, c->seg_rep.reserve(B + 2 * n_old + n_new + n_T + 2 * n_new + n_info));
  double *d_when = c->seg_rep.data(), *d_lb = d_when + B, *d_ub = d_lb + n_old, *d_x_out = d_ub + n_old;
  double *d_T_out = d_x_out + n_new, *d_lb_out = d_T_out + n_T, *d_ub_out = d_lb_out + n_new, *d_info = d_ub_out + n_new;
  if ((rc = gtop_stage_coefficients(c, B, x))) return rc;
  if (at_time) HIPCHK(c, hipMemcpyAsync(d_when, when, (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (lb) {
    HIPCHK(c, hipMemcpyAsync(d_lb, lb, n_old * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ub, ub, n_old * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = gtop_insert_waypoints_device(c, opt, B, m, c->d_x.data(), c->mma_g.data(), c->d_T.data(), c->t_stride,
                                         at_time ? d_when : nullptr, 1, lb ? d_lb : nullptr, lb ? d_ub : nullptr, d_x_out,
                                         d_T_out, lb ? d_lb_out : nullptr, lb ? d_ub_out : nullptr,
                                         info ? d_info : nullptr, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(x_out, d_x_out, n_new * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(T_out, d_T_out, n_T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (lb) {
    HIPCHK(c, hipMemcpyAsync(lb_out, d_lb_out, n_new * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ub_out, d_ub_out, n_new * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  if (info) HIPCHK(c, hipMemcpyAsync(info, d_info, n_info * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
