// gtop_capi_time_moving.cpp — the entry points of the companion header include/gtop_time_moving.h: the derivative of
// the cost with respect to the segment times and the optimizer of the time allocation under the moving-obstacle cost
// (gtop_time_moving.hip), each in a device form (no allocation, no synchronisation: capturable) and a host form over
// the problem set.  The rules of a call are gtop_capi_time.h's without the moving-cost refusal, plus — with the cost in
// force — those of a moving-mode evaluation (gtop_moving_args).
#include "gtop_capi_time.h"
#include "gtop_time_moving.h"

namespace {

// The boxes and start times of a launch of B rows (problem_B as gtop_start_times_fit's): the context's list when the
// moving cost is in force, an empty one otherwise (the static lookup).
struct MovingLookup {
  GtopBoxList boxes;
  GtopStartTimes st;
};
int moving_lookup(gtop_ctx *c, int B, int problem_B, MovingLookup *out) {
  out->boxes = gtop_box_list(c, 0);
  out->st = {nullptr, 0};
  if (!gtop_moving_active(c)) return GTOP_OK;
  GtopMovingArgs mov{};
  if (int rc = gtop_moving_args(c, B, problem_B, &mov)) return rc;
  out->boxes = gtop_box_list(c, c->nbox);
  out->st = {mov.t0, mov.t0_stride};
  return GTOP_OK;
}

int gradient_on_stream(gtop_ctx *c, int B, int m, const void *d_x, const void *d_Df, const void *d_T, int time_stride,
                       void *d_cost, void *d_gT, void *d_gt0, void *d_parts, int problem_B, void *hip_stream) {
  if (int rc = gtop_time_ready(c, "time_gradient_moving", B, m, time_stride, false)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_cost || !d_gT) return fail(c, GTOP_ERR_INVALID, "time_gradient_moving: NULL buffer");
  MovingLookup look;
  if (int rc = moving_lookup(c, B, problem_B, &look)) return rc;
  if (int rc = c->field.need_records64(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_time_gradient_moving(c->field.grid, c->field.rec64.data(), gtop_time_cost(c), look.boxes,
                                             look.st.t0, look.st.stride, B, m, static_cast<const double *>(d_x),
                                             static_cast<const double *>(d_Df), static_cast<const double *>(d_T),
                                             time_stride, static_cast<double *>(d_cost), static_cast<double *>(d_gT),
                                             static_cast<double *>(d_gt0), static_cast<double *>(d_parts),
                                             static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

int optimize_on_stream(gtop_ctx *c, const gtop_timeopt *o, int B, int m, const void *d_x, const void *d_Df,
                       const void *d_T, int time_stride, const void *d_T_lo, void *d_T_out, void *d_info,
                       int problem_B, void *hip_stream) {
  if (int rc = gtop_check_timeopt(c, o)) return rc;
  if (int rc = gtop_time_ready(c, "optimize_times_moving", B, m, time_stride, false)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_T_out || !d_info)
    return fail(c, GTOP_ERR_INVALID, "optimize_times_moving: NULL buffer");
  if (d_T_out == d_T) return fail(c, GTOP_ERR_INVALID, "optimize_times_moving: T_out may not alias T");
  MovingLookup look;
  if (int rc = moving_lookup(c, B, problem_B, &look)) return rc;
  if (int rc = c->field.need_records64(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const double *x = static_cast<const double *>(d_x), *Df = static_cast<const double *>(d_Df);
  const double *T = static_cast<const double *>(d_T), *T_lo = static_cast<const double *>(d_T_lo);
  double *T_out = static_cast<double *>(d_T_out), *info = static_cast<double *>(d_info);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (look.boxes.count == 0)   // the static optimizer itself: its bits
    HIPCHK(c, gtop_launch_time_optimize(c->field.grid, c->field.rec64.data(), gtop_time_cost(c), o->rho, o->t_min,
                                        o->t_max, o->first_move, o->ftol_rel, o->xtol_abs, o->max_evals, B, m, x, Df, T,
                                        time_stride, T_lo, T_out, info, stream));
  else
    HIPCHK(c, gtop_launch_time_optimize_moving(c->field.grid, c->field.rec64.data(), gtop_time_cost(c), look.boxes,
                                               look.st.t0, look.st.stride, o->rho, o->t_min, o->t_max, o->first_move,
                                               o->ftol_rel, o->xtol_abs, o->max_evals, B, m, x, Df, T, time_stride, T_lo,
                                               T_out, info, stream));
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_time_moving_abi_version(void) { return GTOP_TIME_MOVING_ABI_VERSION; }

int gtop_time_gradient_moving_device(gtop_ctx *c, int B, int m, const void *d_x, const void *d_Df, const void *d_T,
                                     int time_stride, void *d_cost, void *d_gT, void *d_gt0, void *d_parts,
                                     void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return gradient_on_stream(c, B, m, d_x, d_Df, d_T, time_stride, d_cost, d_gT, d_gt0, d_parts, 0, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_time_gradient_moving_batch(gtop_ctx *c, int B, const double *x, double *cost, double *gT, double *gt0,
                                    double *parts) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && cost && gT,
                              "time_gradient_moving_batch: 1 <= B <= problem batch; x, cost and gT required")))
    return rc;
  const int m = c->m;
  // (before anything is staged)
  if ((rc = gtop_time_ready(c, "time_gradient_moving_batch", B, m, c->t_stride, false))) return rc;
  MovingLookup look;
  if ((rc = moving_lookup(c, B, c->B, &look))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), nT = (size_t)B * m;
  // the segment staging: cost | gt0 | gT | parts
  HIPCHK(c, c->seg_rep.reserve(2 * (size_t)B + nT * (1 + GTOP_TIME_MOVING_PARTS)));
  double *d_cost = c->seg_rep.data(), *d_gt0 = d_cost + B, *d_gT = d_gt0 + B, *d_parts = d_gT + nT;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = gradient_on_stream(c, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, d_cost, d_gT,
                               gt0 ? d_gt0 : nullptr, parts ? d_parts : nullptr, c->B, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(cost, d_cost, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(gT, d_gT, nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (gt0) HIPCHK(c, hipMemcpyAsync(gt0, d_gt0, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (parts)
    HIPCHK(c, hipMemcpyAsync(parts, d_parts, nT * GTOP_TIME_MOVING_PARTS * sizeof(double), hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_optimize_times_moving_device(gtop_ctx *c, const gtop_timeopt *opt, int B, int m, const void *d_x,
                                      const void *d_Df, const void *d_T, int time_stride, const void *d_T_lo,
                                      void *d_T_out, void *d_info, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return optimize_on_stream(c, opt, B, m, d_x, d_Df, d_T, time_stride, d_T_lo, d_T_out, d_info, 0, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_optimize_times_moving(gtop_ctx *c, const gtop_timeopt *opt, int B, const double *x, const double *T_lo,
                               double *T_out, double *info) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_check_timeopt(c, opt))) return rc;
  if ((rc = gtop_problem_rows(c, B, x && T_out && info,
                              "optimize_times_moving: 1 <= B <= problem batch; x, T_out and info required")))
    return rc;
  const int m = c->m;
  // (before anything is staged)
  if ((rc = gtop_time_ready(c, "optimize_times_moving", B, m, c->t_stride, false))) return rc;
  MovingLookup look;
  if ((rc = moving_lookup(c, B, c->B, &look))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), nT = (size_t)B * m, nI = (size_t)B * GTOP_TIMEOPT_INFO;
  // the segment staging: T_lo | T_out | info
  HIPCHK(c, c->seg_rep.reserve(2 * nT + nI));
  double *d_lo = c->seg_rep.data(), *d_Tout = d_lo + nT, *d_info = d_Tout + nT;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (T_lo) HIPCHK(c, hipMemcpyAsync(d_lo, T_lo, nT * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = optimize_on_stream(c, opt, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride,
                               T_lo ? d_lo : nullptr, d_Tout, d_info, c->B, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(T_out, d_Tout, nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info, d_info, nI * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
