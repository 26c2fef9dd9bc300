// gtop_capi_swarm.cpp — the entry points of the companion header include/gtop_swarm.h: the swarm separation cost and
// its gradient (gtop_swarm.hip) in a device form (no allocation, no synchronisation: capturable) and a host form over
// the problem set, and the swarm optimizer: sweeps of the batched MMA loop's two-launch form (gtop_capi_eval.cpp) with
// the swarm term added between its launches.
#include <cmath>

#include "gtop_ctx.h"
#include "gtop_swarm.h"

namespace {

// the rules of a swarm term over B rows, before anything is staged or launched
int swarm_ready(gtop_ctx *c, const char *who, int B, int m, int time_stride, const gtop_swarm_opts *o) {
  const std::string w = who;
  if (!o) return fail(c, GTOP_ERR_INVALID, w + ": options is NULL");
  if (o->reserved[0] != 0 || o->reserved[1] != 0) return fail(c, GTOP_ERR_INVALID, w + ": reserved must be 0");
  if (!std::isfinite(o->t_lo) || !std::isfinite(o->dt) || !(o->dt > 0.0) || o->n_samples < 1 ||
      o->n_samples > GTOP_SEP_MAX_SAMPLES || (o->hold_ends != 0 && o->hold_ends != 1))
    return fail(c, GTOP_ERR_INVALID, w + ": need finite t_lo, finite dt > 0, n_samples in 1 .. 65536, hold_ends in {0, 1}");
  if (!std::isfinite(o->w) || !(o->w >= 0.0) || !std::isfinite(o->radius) || !(o->radius > 0.0))
    return fail(c, GTOP_ERR_INVALID, w + ": need a finite w >= 0 and a finite radius > 0");
  if (B < 0 || B > GTOP_SEP_MAX_B || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, w + ": need 0 <= B <= 4096, 2 <= m <= 227, time_stride in {0, m}");
  if (B > 0 && c->t0_count > 1 && c->t0_count != B)
    return fail(c, GTOP_ERR_INVALID, w + ": the start times set are neither none, one, nor one per row");
  return GTOP_OK;
}

GtopSwarmGrid swarm_grid(const gtop_swarm_opts *o) { return {o->t_lo, o->dt, o->n_samples, o->hold_ends}; }

int gradient_on_stream(gtop_ctx *c, const gtop_swarm_opts *o, int B, int m, const void *d_coeff, const void *d_frozen,
                       const void *d_T, int time_stride, void *d_S, void *d_grad, void *d_active, void *d_work,
                       size_t work_bytes, void *hip_stream) {
  if (int rc = swarm_ready(c, "swarm_gradient", B, m, time_stride, o)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_S || !d_grad || !d_work) return fail(c, GTOP_ERR_INVALID, "swarm_gradient: NULL buffer");
  if (work_bytes < gtop_swarm_work_bytes(B, m, o->n_samples))
    return fail(c, GTOP_ERR_INVALID, "swarm_gradient: work_bytes is below gtop_swarm_workspace_bytes(B, m, n_samples)");
  const GtopStartTimes st = gtop_start_times(c);
  const GtopSwarmGrid g = swarm_grid(o);
  const double *T = static_cast<const double *>(d_T);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_swarm_sample(g, B, m, static_cast<const double *>(d_coeff), T, time_stride, st.t0, st.stride, 0,
                                     d_work, s));
  if (d_frozen)
    HIPCHK(c, gtop_launch_swarm_sample(g, B, m, static_cast<const double *>(d_frozen), T, time_stride, st.t0, st.stride,
                                       1, d_work, s));
  HIPCHK(c, gtop_launch_swarm_terms(g, o->w, o->radius, B, m, T, time_stride, st.t0, st.stride, d_frozen ? 1 : 0, 0,
                                    static_cast<double *>(d_S), static_cast<double *>(d_grad),
                                    static_cast<double *>(d_active), d_work, s));
  return GTOP_OK;
}

// what a round of a sweep adds between the evaluation and the update
struct SwarmRound {
  const gtop_swarm_opts *o;
  int B, m, time_stride;
  const void *d_Df, *d_T;
  void *d_work;
};

int swarm_round(void *user, gtop_ctx *c, const double *d_xcur, double *d_f, double *d_grad, hipStream_t s) {
  const SwarmRound &r = *static_cast<const SwarmRound *>(user);
  const GtopStartTimes st = gtop_start_times(c);
  const GtopSwarmGrid g = swarm_grid(r.o);
  const double *T = static_cast<const double *>(r.d_T);
  double *coeff = gtop_swarm_coeff_scratch(r.d_work, r.B, r.m, r.o->n_samples);
  HIPCHK(c, gtop_launch_coefficients(r.B, r.m, d_xcur, static_cast<const double *>(r.d_Df), T, r.time_stride, coeff, s));
  HIPCHK(c, gtop_launch_swarm_sample(g, r.B, r.m, coeff, T, r.time_stride, st.t0, st.stride, 0, r.d_work, s));
  HIPCHK(c, gtop_launch_swarm_terms(g, r.o->w, r.o->radius, r.B, r.m, T, r.time_stride, st.t0, st.stride, 1, 1, d_f, d_grad,
                                    nullptr, r.d_work, s));
  return GTOP_OK;
}

int optimize_on_stream(gtop_ctx *c, const gtop_swarm_opts *o, const gtop_swarm_stop *stop, int B, int m, void *d_x,
                       const void *d_Df, const void *d_T, int time_stride, const void *d_lb, const void *d_ub,
                       void *d_min_cost, void *d_joint, void *d_work, size_t work_bytes, void *hip_stream, int problem_B) {
  if (!c->have_params) return fail(c, GTOP_ERR_STATE, "gtop_set_params has not been called");
  if (!c->field.have_grid) return fail(c, GTOP_ERR_STATE, "no distance field set");
  if (c->opt_dtype == GTOP_F32)
    return fail(c, GTOP_ERR_STATE, "optimize_swarm: fp32 evaluations (gtop_set_optimizer_precision) have no two-launch form");
  if (c->moving_cost != 0)
    return fail(c, GTOP_ERR_STATE, "optimize_swarm: the moving-obstacle cost is switched on; the two terms together are not built");
  if (int rc = swarm_ready(c, "optimize_swarm", B, m, time_stride, o)) return rc;
  if (!stop || stop->sweeps < 1 || stop->evals_per_sweep < 1 || stop->reserved[0] != 0 || stop->reserved[1] != 0)
    return fail(c, GTOP_ERR_INVALID, "optimize_swarm: need stop rules with sweeps >= 1, evals_per_sweep >= 1, reserved 0");
  if (m > 118) return fail(c, GTOP_ERR_INVALID, "optimize_swarm: the optimizer serves up to 118 segments");
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_lb || !d_ub || !d_min_cost || !d_work)
    return fail(c, GTOP_ERR_INVALID, "optimize_swarm: NULL buffer");
  if (work_bytes < gtop_swarm_work_bytes(B, m, o->n_samples))
    return fail(c, GTOP_ERR_INVALID, "optimize_swarm: work_bytes is below gtop_swarm_workspace_bytes(B, m, n_samples)");
  if (int rc = c->field.need_records64(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const GtopStartTimes st = gtop_start_times(c);
  const GtopSwarmGrid g = swarm_grid(o);
  const double *T = static_cast<const double *>(d_T), *Df = static_cast<const double *>(d_Df);
  double *coeff = gtop_swarm_coeff_scratch(d_work, B, m, o->n_samples);
  const bool swarm = o->w != 0.0;   // w == 0: the term and its gradient are +0; nothing of it is enqueued
  SwarmRound round = {o, B, m, time_stride, d_Df, d_T, d_work};
  const GtopRoundHook hook = {swarm_round, &round};
  const GtopRoundHook none = {[](void *, gtop_ctx *, const double *, double *, double *, hipStream_t) { return (int)GTOP_OK; },
                              nullptr};
  for (int sweep = 0; sweep < stop->sweeps; ++sweep) {
    if (swarm) {   // (1) the rows as the sweep finds them: the frozen side
      HIPCHK(c, gtop_launch_coefficients(B, m, static_cast<const double *>(d_x), Df, T, time_stride, coeff, s));
      HIPCHK(c, gtop_launch_swarm_sample(g, B, m, coeff, T, time_stride, st.t0, st.stride, 1, d_work, s));
    }
    // (2), (3): the rounds, and every row's best point back in d_x
    if (int rc = gtop_optimize_rounds(c, B, m, d_x, d_Df, d_T, time_stride, d_lb, d_ub, stop->evals_per_sweep, d_min_cost,
                                      hip_stream, problem_B, swarm ? &hook : &none))
      return rc;
  }
  if (d_joint) {   // the closing joint evaluation: the others unfrozen
    double *S = nullptr;
    // (the rounds left mma_f and mma_g large enough for a cost and a gradient of B rows)
    if (int rc = gtop_eval_device(c, GTOP_F64, B, m, d_x, d_Df, d_T, time_stride, c->mma_f.data(), c->mma_g.data(), hip_stream))
      return rc;
    if (swarm) {
      S = gtop_swarm_joint_scratch(d_work, B, m, o->n_samples);
      HIPCHK(c, gtop_launch_coefficients(B, m, static_cast<const double *>(d_x), Df, T, time_stride, coeff, s));
      HIPCHK(c, gtop_launch_swarm_sample(g, B, m, coeff, T, time_stride, st.t0, st.stride, 0, d_work, s));
      HIPCHK(c, gtop_launch_swarm_terms(g, o->w, o->radius, B, m, T, time_stride, st.t0, st.stride, 0, 0, S, c->mma_g.data(),
                                        nullptr, d_work, s));
    }
    HIPCHK(c, gtop_launch_swarm_joint(B, c->mma_f.data(), S, static_cast<double *>(d_joint), s));
  }
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_swarm_abi_version(void) { return GTOP_SWARM_ABI_VERSION; }

int gtop_swarm_workspace_bytes(int B, int m, int n_samples, size_t *bytes) try {
  if (!bytes || B < 0 || B > GTOP_SEP_MAX_B || m < 2 || m > 227 || n_samples < 1 || n_samples > GTOP_SEP_MAX_SAMPLES)
    return GTOP_ERR_INVALID;
  *bytes = gtop_swarm_work_bytes(B, m, n_samples);
  return GTOP_OK;
} GTOP_CATCH_STATUS(static_cast<gtop_ctx *>(nullptr))

int gtop_swarm_gradient_device(gtop_ctx *c, const gtop_swarm_opts *opt, int B, int m, const void *d_coeff,
                               const void *d_coeff_frozen, const void *d_T, int time_stride, void *d_S, void *d_grad,
                               void *d_active, void *d_work, size_t work_bytes, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return gradient_on_stream(c, opt, B, m, d_coeff, d_coeff_frozen, d_T, time_stride, d_S, d_grad, d_active, d_work,
                            work_bytes, hip_stream);
} GTOP_CATCH_STATUS(c)

// Staged as gtop_separation_batch stages: x_frozen -> d_x -> the frozen rows' coefficients in the staging buffer, x ->
// d_x -> the coefficients in the coefficient scratch, the launches on the context's stream, copies, one wait.
int gtop_swarm_gradient_batch(gtop_ctx *c, const gtop_swarm_opts *opt, int B, const double *x, const double *x_frozen,
                              double *S, double *grad, double *active) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && S && grad, "swarm_gradient_batch: 1 <= B <= problem batch; x, S and grad required")))
    return rc;
  const int m = c->m;
  if ((rc = swarm_ready(c, "swarm_gradient_batch", B, m, c->t_stride, opt))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), bn = (size_t)B * n, ncoef = (size_t)B * m * 18;
  const size_t work_bytes = gtop_swarm_work_bytes(B, m, opt->n_samples);
  HIPCHK(c, c->swarm_stage.reserve(ncoef + 2 * (size_t)B + bn + (work_bytes + sizeof(double) - 1) / sizeof(double)));
  double *d_frozen = c->swarm_stage.data(), *d_S = d_frozen + ncoef, *d_grad = d_S + B, *d_active = d_grad + bn,
         *d_work = d_active + B;
  if (x_frozen) {
    HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x_frozen, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = gtop_coefficients_device(c, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, d_frozen, c->stream)))
      return rc;
  }
  if ((rc = gtop_stage_coefficients(c, B, x))) return rc;
  if ((rc = gradient_on_stream(c, opt, B, m, c->mma_g.data(), x_frozen ? d_frozen : nullptr, c->d_T.data(), c->t_stride,
                               d_S, d_grad, d_active, d_work, work_bytes, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(S, d_S, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(grad, d_grad, bn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (active) HIPCHK(c, hipMemcpyAsync(active, d_active, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_optimize_swarm_device(gtop_ctx *c, const gtop_swarm_opts *opt, const gtop_swarm_stop *stop, int B, int m,
                               void *d_x, const void *d_Df, const void *d_T, int time_stride, const void *d_lb,
                               const void *d_ub, void *d_min_cost, void *d_joint, void *d_work, size_t work_bytes,
                               void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return optimize_on_stream(c, opt, stop, B, m, d_x, d_Df, d_T, time_stride, d_lb, d_ub, d_min_cost, d_joint, d_work,
                            work_bytes, hip_stream, 0);
} GTOP_CATCH_STATUS(c)

int gtop_optimize_swarm(gtop_ctx *c, const gtop_swarm_opts *opt, const gtop_swarm_stop *stop, int B, double *x,
                        const double *lb, const double *ub, double *min_cost, double *joint) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && lb && ub && min_cost,
                              "optimize_swarm: 1 <= B <= problem batch; x, lb, ub and min_cost required")))
    return rc;
  const int m = c->m;
  if ((rc = swarm_ready(c, "optimize_swarm", B, m, c->t_stride, opt))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), bn = (size_t)B * n;
  const size_t work_bytes = gtop_swarm_work_bytes(B, m, opt->n_samples);
  HIPCHK(c, c->mma_lb.reserve(bn));
  HIPCHK(c, c->mma_ub.reserve(bn));
  HIPCHK(c, c->swarm_stage.reserve(2 * (size_t)B + (work_bytes + sizeof(double) - 1) / sizeof(double)));
  double *d_joint = c->swarm_stage.data(), *d_work = d_joint + 2 * (size_t)B;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->mma_lb.data(), lb, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->mma_ub.data(), ub, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = optimize_on_stream(c, opt, stop, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride,
                               c->mma_lb.data(), c->mma_ub.data(), c->d_cost.data(), joint ? d_joint : nullptr, d_work,
                               work_bytes, c->stream, c->B)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(x, c->d_x.data(), bn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(min_cost, c->d_cost.data(), (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (joint) HIPCHK(c, hipMemcpyAsync(joint, d_joint, 2 * (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
