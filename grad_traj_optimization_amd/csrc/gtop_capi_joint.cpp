// gtop_capi_joint.cpp — the entry points of the companion header include/gtop_joint.h: the cost with its derivatives
// with respect to the free waypoint values and the segment times from one pass (gtop_joint.hip), and the optimizer of
// the stacked variable: the batched MMA loop's two-launch form (gtop_mma.hip) around that pass, its whole state in the
// caller's workspace.  Each in a device form (no allocation, no synchronisation: capturable) and a host form over the
// problem set.
#include <cmath>

#include "gtop_capi_time.h"
#include "gtop_joint.h"

namespace {

size_t joint_nz(int m) { return 10 * (size_t)m - 9; }

// the workspace in doubles: the six n_z-vectors | zlb | zub | g, B n_z each; f [B]; the five scalars [B] each; the
// integers k | state | nevals | code | evaluations, B each
size_t joint_work_doubles(int B, int m) {
  const size_t b = (size_t)B;
  return 9 * b * joint_nz(m) + 6 * b + (5 * b + 1) / 2;
}

int check_jointopt(gtop_ctx *c, const gtop_jointopt *o) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "optimize_joint: options is NULL");
  if (o->reserved != 0) return fail(c, GTOP_ERR_INVALID, "optimize_joint: reserved must be 0");
  if (!(o->rho >= 0.0) || !std::isfinite(o->rho))
    return fail(c, GTOP_ERR_INVALID, "optimize_joint: rho must be finite and >= 0");
  if (!(o->t_min >= 0.0301) || !(o->t_min <= o->t_max) || !std::isfinite(o->t_max))
    return fail(c, GTOP_ERR_INVALID, "optimize_joint: need 0.0301 <= t_min <= t_max, both finite");
  if (!(o->ftol_rel >= 0.0) || !(o->xtol_rel >= 0.0))
    return fail(c, GTOP_ERR_INVALID, "optimize_joint: ftol_rel and xtol_rel must be >= 0");
  if (o->max_evals < 1) return fail(c, GTOP_ERR_INVALID, "optimize_joint: max_evals must be >= 1");
  return GTOP_OK;
}

int gradient_on_stream(gtop_ctx *c, int B, int m, const void *d_x, const void *d_Df, const void *d_T, int time_stride,
                       void *d_cost, void *d_gx, void *d_gT, void *d_parts, void *hip_stream) {
  if (int rc = gtop_time_ready(c, "joint_gradient", B, m, time_stride, true)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_cost || !d_gx || !d_gT) return fail(c, GTOP_ERR_INVALID, "joint_gradient: NULL buffer");
  if (int rc = c->field.need_records64(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1);
  const GtopJointRows rows = {static_cast<const double *>(d_x), n, static_cast<const double *>(d_T), (size_t)time_stride,
                              static_cast<double *>(d_cost), 1, static_cast<double *>(d_gx), n,
                              static_cast<double *>(d_gT), (size_t)m, nullptr, 0, 0};
  HIPCHK(c, gtop_launch_joint_pass(c->field.grid, c->field.rec64.data(), gtop_time_cost(c), B, m, rows,
                                   static_cast<const double *>(d_Df), 0, 0.0, static_cast<double *>(d_parts),
                                   static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

int optimize_on_stream(gtop_ctx *c, const gtop_jointopt *o, int B, int m, void *d_x, const void *d_Df, const void *d_T,
                       int time_stride, const void *d_lb, const void *d_ub, const void *d_T_lo, void *d_T_out,
                       void *d_info, void *d_work, size_t work_bytes, void *hip_stream) {
  if (int rc = check_jointopt(c, o)) return rc;
  if (int rc = gtop_time_ready(c, "optimize_joint", B, m, time_stride, true)) return rc;
  if (c->opt_dtype == GTOP_F32)
    return fail(c, GTOP_ERR_STATE, "optimize_joint: fp32 evaluations (gtop_set_optimizer_precision): the joint pass is fp64 only");
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_lb || !d_ub || !d_T_out || !d_info || !d_work)
    return fail(c, GTOP_ERR_INVALID, "optimize_joint: NULL buffer");
  if (d_T_out == d_T) return fail(c, GTOP_ERR_INVALID, "optimize_joint: T_out may not alias T");
  if (work_bytes < joint_work_doubles(B, m) * sizeof(double))
    return fail(c, GTOP_ERR_INVALID, "optimize_joint: work_bytes is below gtop_joint_workspace_bytes(B, m)");
  if (int rc = c->field.need_records64(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const size_t n = 9 * (size_t)(m - 1), nz = joint_nz(m), bz = (size_t)B * nz;
  double *w = static_cast<double *>(d_work);
  GtopMmaState st{};
  st.x = w; st.xcur = st.x + bz; st.xprev = st.xcur + bz; st.xprevprev = st.xprev + bz;
  st.dfdx = st.xprevprev + bz; st.sigma = st.dfdx + bz;
  double *zlb = st.sigma + bz, *zub = zlb + bz, *g = zub + bz, *f = g + bz;
  st.lb = zlb; st.ub = zub;
  st.rho = f + B; st.minf = st.rho + B; st.gval = st.minf + B; st.wval = st.gval + B; st.fprev = st.wval + B;
  st.k = reinterpret_cast<int *>(st.fprev + B); st.state = st.k + B; st.nevals = st.state + B;
  int *code = st.nevals + B, *nevals = code + B;
  st.iters = 1;
  st.max_evals = o->max_evals;
  st.ftol_rel = o->ftol_rel;
  st.xtol_rel = o->xtol_rel;
  st.max_ticks = 0;
  const double *Df = static_cast<const double *>(d_Df);
  double *info = static_cast<double *>(d_info);
  const GtopTimeCost cost = gtop_time_cost(c);
  // the start point travels through g (free until the first pass writes it)
  HIPCHK(c, gtop_launch_joint_pack(B, m, static_cast<const double *>(d_x), static_cast<const double *>(d_T), time_stride,
                                   static_cast<const double *>(d_lb), static_cast<const double *>(d_ub),
                                   static_cast<const double *>(d_T_lo), o->t_min, o->t_max, g, zlb, zub, s));
  HIPCHK(c, gtop_launch_mma_init(st, B, (int)nz, g, s));
  GtopJointRows rows = {st.xcur, nz, st.xcur + n, nz, f, 1, g, nz, g + n, nz, info + 2, GTOP_JOINT_INFO, 0};
  for (int it = 0; it < o->max_evals; ++it) {
    if (it == 1) rows.aux = nullptr;   // (F at the clamped start: the first round's alone)
    HIPCHK(c, gtop_launch_joint_pass(c->field.grid, c->field.rec64.data(), cost, B, m, rows, Df, 1, o->rho, nullptr, s));
    HIPCHK(c, gtop_launch_mma_update(st, B, (int)nz, f, g, s));
  }
  // the closing pass at the best point: its cost, and the gradient the report reads
  rows.x = st.x; rows.T = st.x + n;
  rows.aux = info + 4; rows.aux_plain = 1;
  HIPCHK(c, gtop_launch_joint_pass(c->field.grid, c->field.rec64.data(), cost, B, m, rows, Df, 1, o->rho, nullptr, s));
  HIPCHK(c, gtop_launch_mma_finish(st, B, code, nevals, s));
  HIPCHK(c, gtop_launch_joint_report(B, m, st.x, g, zlb, zub, st.minf, code, nevals, static_cast<double *>(d_x),
                                     static_cast<double *>(d_T_out), info, s));
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_joint_abi_version(void) { return GTOP_JOINT_ABI_VERSION; }

int gtop_joint_workspace_bytes(int B, int m, size_t *bytes) try {
  if (!bytes || B < 0 || m < 2 || m > 227) return GTOP_ERR_INVALID;
  *bytes = joint_work_doubles(B, m) * sizeof(double);
  return GTOP_OK;
} GTOP_CATCH_STATUS(static_cast<gtop_ctx *>(nullptr))

int gtop_joint_gradient_device(gtop_ctx *c, int B, int m, const void *d_x, const void *d_Df, const void *d_T,
                               int time_stride, void *d_cost, void *d_gx, void *d_gT, void *d_parts,
                               void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return gradient_on_stream(c, B, m, d_x, d_Df, d_T, time_stride, d_cost, d_gx, d_gT, d_parts, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_joint_gradient_batch(gtop_ctx *c, int B, const double *x, double *cost, double *gx, double *gT,
                              double *parts) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && cost && gx && gT,
                              "joint_gradient_batch: 1 <= B <= problem batch; x, cost, gx and gT required")))
    return rc;
  const int m = c->m;
  if ((rc = gtop_time_ready(c, "joint_gradient_batch", B, m, c->t_stride, true))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), bn = (size_t)B * n, nT = (size_t)B * m;
  // the segment staging: cost | gx | gT | parts
  HIPCHK(c, c->seg_rep.reserve((size_t)B + bn + nT * (1 + GTOP_TIME_PARTS)));
  double *d_cost = c->seg_rep.data(), *d_gx = d_cost + B, *d_gT = d_gx + bn, *d_parts = d_gT + nT;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = gradient_on_stream(c, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, d_cost, d_gx, d_gT,
                               parts ? d_parts : nullptr, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(cost, d_cost, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(gx, d_gx, bn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(gT, d_gT, nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (parts)
    HIPCHK(c, hipMemcpyAsync(parts, d_parts, nT * GTOP_TIME_PARTS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_optimize_joint_device(gtop_ctx *c, const gtop_jointopt *opt, int B, int m, void *d_x, const void *d_Df,
                               const void *d_T, int time_stride, const void *d_lb, const void *d_ub, const void *d_T_lo,
                               void *d_T_out, void *d_info, void *d_work, size_t work_bytes, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return optimize_on_stream(c, opt, B, m, d_x, d_Df, d_T, time_stride, d_lb, d_ub, d_T_lo, d_T_out, d_info, d_work,
                            work_bytes, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_optimize_joint(gtop_ctx *c, const gtop_jointopt *opt, int B, double *x, const double *lb, const double *ub,
                        const double *T_lo, double *T_out, double *info) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = check_jointopt(c, opt))) return rc;
  if ((rc = gtop_problem_rows(c, B, x && lb && ub && T_out && info,
                              "optimize_joint: 1 <= B <= problem batch; x, lb, ub, T_out and info required")))
    return rc;
  const int m = c->m;
  if ((rc = gtop_time_ready(c, "optimize_joint", B, m, c->t_stride, true))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(m - 1), bn = (size_t)B * n, nT = (size_t)B * m, nI = (size_t)B * GTOP_JOINT_INFO;
  const size_t nW = joint_work_doubles(B, m);
  HIPCHK(c, c->mma_lb.reserve(bn));
  HIPCHK(c, c->mma_ub.reserve(bn));
  // the segment staging: T_lo | T_out | info | the workspace
  HIPCHK(c, c->seg_rep.reserve(2 * nT + nI + nW));
  double *d_lo = c->seg_rep.data(), *d_Tout = d_lo + nT, *d_info = d_Tout + nT, *d_work = d_info + nI;
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->mma_lb.data(), lb, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->mma_ub.data(), ub, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (T_lo) HIPCHK(c, hipMemcpyAsync(d_lo, T_lo, nT * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = optimize_on_stream(c, opt, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, c->mma_lb.data(),
                               c->mma_ub.data(), T_lo ? d_lo : nullptr, d_Tout, d_info, d_work, nW * sizeof(double),
                               c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(x, c->d_x.data(), bn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(T_out, d_Tout, nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info, d_info, nI * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
