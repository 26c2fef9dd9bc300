// gtop_capi_problem.cpp — the problem set of a context and what stands around an optimisation: path set-up
// (gtop_set_paths*) in front, trajectory post-processing (coefficients, statistics, samples) behind, the default bounds.
#include <cmath>

#include "gtop_ctx.h"
#include "gtop_minjerk_plan.h"

// (gtop_ctx.h) what every host form that goes from x to coefficients stages
int gtop_stage_coefficients(gtop_ctx *c, int B, const double *x) {
  const int m = c->m;
  const size_t n = 9 * (size_t)(m - 1), ncoef = (size_t)B * m * 18;
  HIPCHK(c, c->mma_g.reserve(ncoef > (size_t)B * n ? ncoef : (size_t)B * n));
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return gtop_coefficients_device(c, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, c->mma_g.data(),
                                  c->stream);
}

extern "C" {

int gtop_set_problem(gtop_ctx *c, int B, int m, const double *segment_time, int time_stride,
                     const double *Df) try {
  if (!c) return GTOP_ERR_INVALID;
  if (B < 1 || m < 2 || !segment_time || !Df || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "set_problem: need B >= 1, m >= 2, time_stride in {0, m}");
  const size_t nT = time_stride ? (size_t)B * m : (size_t)m;
  for (size_t i = 0; i < nT; ++i)
    if (!(segment_time[i] > 0.0)) return fail(c, GTOP_ERR_INVALID, "segment_time must be > 0");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1);
  HIPCHK(c, c->d_T.reserve(nT));
  HIPCHK(c, c->d_Df.reserve((size_t)B * 18));
  HIPCHK(c, c->d_x.reserve((size_t)B * n));
  HIPCHK(c, c->d_grad.reserve((size_t)B * n));
  HIPCHK(c, c->d_cost.reserve((size_t)B));
  HIPCHK(c, hipMemcpyAsync(c->d_T.data(), segment_time, nT * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_Df.data(), Df, (size_t)B * 18 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->B = B; c->m = m; c->t_stride = time_stride;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- setup (f3) and post-processing (f4) ----
int gtop_setup_paths_device(gtop_ctx *c, int B, int m, const void *d_wp, double mean_v, double init_time,
                            void *d_T, void *d_Df, void *d_x0, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (B < 0 || m < 2 || !(mean_v > 0.0)) return fail(c, GTOP_ERR_INVALID, "setup_paths: need B >= 0, m >= 2, mean_v > 0");
  if (B == 0) return GTOP_OK;
  if (!d_wp || !d_T || !d_Df || !d_x0) return fail(c, GTOP_ERR_INVALID, "setup_paths: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_setup_paths(B, m, static_cast<const double *>(d_wp), mean_v, init_time,
                                    static_cast<double *>(d_T), static_cast<double *>(d_Df),
                                    static_cast<double *>(d_x0), static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_set_paths(gtop_ctx *c, int B, int m, const double *waypoints, double mean_v, double init_time,
                   double *x0) try {
  if (!c) return GTOP_ERR_INVALID;
  if (B < 1 || m < 2 || !waypoints || !(mean_v > 0.0))
    return fail(c, GTOP_ERR_INVALID, "set_paths: need B >= 1, m >= 2 (3+ waypoints), mean_v > 0");
  // same rule as gtop_set_problem: every segment time must be > 0.  Coincident consecutive waypoints give
  // T_s = 0 (grad_traj_optimizer.cpp:73-81), a singular A_s in the reference and NaN here.
  for (int b = 0; b < B; ++b)
    for (int s = 0; s < m; ++s) {
      const double *p = waypoints + ((size_t)b * (m + 1) + s) * 3;
      const double dx = p[0] - p[3], dy = p[1] - p[4], dz = p[2] - p[5];
      const double T = std::sqrt(dx * dx + dy * dy + dz * dz) / mean_v + (s == 0 ? init_time : 0.0);
      if (!(T > 0.0)) return fail(c, GTOP_ERR_INVALID, "set_paths: coincident consecutive waypoints (segment time 0)");
    }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), nwp = (size_t)B * (m + 1) * 3;
  int rc;
  HIPCHK(c, c->d_T.reserve((size_t)B * m));
  HIPCHK(c, c->d_Df.reserve((size_t)B * 18));
  HIPCHK(c, c->d_x.reserve((size_t)B * n));
  HIPCHK(c, c->d_grad.reserve((size_t)B * n));
  HIPCHK(c, c->d_cost.reserve((size_t)B));
  HIPCHK(c, c->d_pts.reserve(nwp));   // staging, shared with the obstacle list
  HIPCHK(c, hipMemcpyAsync(c->d_pts.data(), waypoints, nwp * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = gtop_setup_paths_device(c, B, m, c->d_pts.data(), mean_v, init_time, c->d_T.data(), c->d_Df.data(),
                                    c->d_x.data(), c->stream)))
    return rc;
  if (x0) HIPCHK(c, hipMemcpyAsync(x0, c->d_x.data(), (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->B = B; c->m = m; c->t_stride = m;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- the minimum-jerk start point (gtop_minjerk.hip) ----
int gtop_min_jerk_start_device(gtop_ctx *c, int B, int m, void *d_x, const void *d_Df, const void *d_T, int time_stride,
                               void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  GtopMinJerkPlan plan;
  if (!gtop_minjerk_plan(B, m, &plan) || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "min_jerk_start: need B >= 0, 2 <= m <= 227, time_stride in {0, m}");
  if (!d_x || !d_Df || !d_T) return fail(c, GTOP_ERR_INVALID, "min_jerk_start: NULL buffer");
  if (B == 0) return GTOP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_min_jerk_start(B, m, static_cast<double *>(d_x), static_cast<const double *>(d_Df),
                                       static_cast<const double *>(d_T), time_stride,
                                       static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_min_jerk_start(gtop_ctx *c, int B, double *x) try {
  if (!c) return GTOP_ERR_INVALID;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  if (B < 1 || B > c->B || !x) return fail(c, GTOP_ERR_INVALID, "min_jerk_start: 1 <= B <= problem batch, x required");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)B * 9 * (size_t)(c->m - 1) * sizeof(double);
  int rc;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = gtop_min_jerk_start_device(c, B, c->m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(x, c->d_x.data(), bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_get_problem(gtop_ctx *c, double *segment_time, double *Df) try {
  if (!c) return GTOP_ERR_INVALID;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "no problem set");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nT = c->t_stride ? (size_t)c->B * c->m : (size_t)c->m;
  if (segment_time)
    HIPCHK(c, hipMemcpyAsync(segment_time, c->d_T.data(), nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (Df) HIPCHK(c, hipMemcpyAsync(Df, c->d_Df.data(), (size_t)c->B * 18 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_coefficients_device(gtop_ctx *c, int B, int m, const void *d_x, const void *d_Df, const void *d_T,
                             int time_stride, void *d_coeff, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (B < 0 || m < 2 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "coefficients: need B >= 0, m >= 2, time_stride in {0, m}");
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_coeff) return fail(c, GTOP_ERR_INVALID, "coefficients: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_coefficients(B, m, static_cast<const double *>(d_x), static_cast<const double *>(d_Df),
                                     static_cast<const double *>(d_T), time_stride, static_cast<double *>(d_coeff),
                                     static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_sample_trajectories_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                    double dt_sample, void *d_stats, void *d_samples, int max_samples,
                                    void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (B < 0 || m < 1 || !(dt_sample > 0.0) || (time_stride != 0 && time_stride != m) || max_samples < 0)
    return fail(c, GTOP_ERR_INVALID, "eval_trajectories: need B >= 0, m >= 1, dt_sample > 0, time_stride in {0, m}");
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_stats || (max_samples > 0 && !d_samples))
    return fail(c, GTOP_ERR_INVALID, "eval_trajectories: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_eval_trajectories(B, m, static_cast<const double *>(d_coeff), static_cast<const double *>(d_T),
                                          time_stride, dt_sample, static_cast<double *>(d_stats),
                                          max_samples > 0 ? static_cast<double *>(d_samples) : nullptr, max_samples,
                                          static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_eval_trajectories_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                  double dt_sample, void *d_stats, void *hip_stream) try {
  return gtop_sample_trajectories_device(c, B, m, d_coeff, d_T, time_stride, dt_sample, d_stats, nullptr, 0, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_trajectory_stats(gtop_ctx *c, int B, const double *x, double dt_sample, double *coeff, double *stats) try {
  return gtop_trajectory_samples(c, B, x, dt_sample, coeff, stats, nullptr, 0);
} GTOP_CATCH_STATUS(c)

int gtop_trajectory_samples(gtop_ctx *c, int B, const double *x, double dt_sample, double *coeff, double *stats,
                            double *samples, int max_samples) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && (coeff || stats || samples) && max_samples >= 0 && !(samples && max_samples == 0),
                              "trajectory_stats: 1 <= B <= problem batch, x and an output required")))
    return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const int m = c->m;
  const size_t ncoef = (size_t)B * m * 18;
  HIPCHK(c, c->mma_f.reserve((size_t)B * GTOP_TRAJ_STATS));
  if ((rc = gtop_stage_coefficients(c, B, x))) return rc;
  if (coeff) HIPCHK(c, hipMemcpyAsync(coeff, c->mma_g.data(), ncoef * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (stats || samples) {
    const size_t ns = samples ? (size_t)B * max_samples * 3 : 0;
    if (ns) HIPCHK(c, c->d_q.reserve(ns));   // (the query staging buffer doubles as sample scratch)
    if (ns) HIPCHK(c, hipMemsetAsync(c->d_q.data(), 0, ns * sizeof(double), c->stream));   // rows past a trajectory's count read 0
    if ((rc = gtop_sample_trajectories_device(c, B, m, c->mma_g.data(), c->d_T.data(), c->t_stride, dt_sample, c->mma_f.data(),
                                              samples ? c->d_q.data() : nullptr, samples ? max_samples : 0, c->stream)))
      return rc;
    if (stats)
      HIPCHK(c, hipMemcpyAsync(stats, c->mma_f.data(), (size_t)B * GTOP_TRAJ_STATS * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
    if (samples) HIPCHK(c, hipMemcpyAsync(samples, c->d_q.data(), ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// grad_traj_optimizer.cpp:151-179
int gtop_default_bounds(int B, int m, const double *path, double bos, double vos, double aos, double *lb,
                        double *ub) {
  if (B < 1 || m < 2 || !path || !lb || !ub) return GTOP_ERR_INVALID;
  const int num_dp = 3 * m - 3;
  const size_t n = 3 * (size_t)num_dp;
  for (int b = 0; b < B; ++b) {
    const double *p = path + (size_t)b * (m + 1) * 3;
    double *l = lb + (size_t)b * n, *u = ub + (size_t)b * n;
    for (int i = 0; i < num_dp; ++i)
      for (int a = 0; a < 3; ++a) {
        const size_t j = (size_t)i + (size_t)a * num_dp;
        if (i % 3 == 0) {
          l[j] = p[(i / 3 + 1) * 3 + a] - bos;
          u[j] = p[(i / 3 + 1) * 3 + a] + bos;
        } else if (i % 3 == 1) {
          l[j] = -vos;
          u[j] = vos;
        } else {
          l[j] = -aos;
          u[j] = aos;
        }
      }
  }
  return GTOP_OK;
}

}  // extern "C"
