// gtop_capi_report.cpp — what judges a batch of trajectories against the field and the moving boxes: the sampled reports
// (whole trajectory, gtop_validate.hip; per segment, gtop_segments.hip), the selection of the best passing row, and the
// continuous-time certificates (gtop_certify.hip) of the static field and of the field with the boxes.  Each in a
// device form (no allocation, no synchronisation: capturable) and a host form over the problem set.
#include <cmath>
#include <string>

#include "gtop_ctx.h"

namespace {

int check_limits(gtop_ctx *c, const gtop_limits *lim) {
  if (!lim) return fail(c, GTOP_ERR_INVALID, "validate: limits is NULL");
  if (!std::isfinite(lim->margin) || !std::isfinite(lim->max_vel) || !std::isfinite(lim->max_acc))
    return fail(c, GTOP_ERR_INVALID, "validate: margin, max_vel and max_acc must be finite");
  return GTOP_OK;
}

// Either sampled report of B rows into d_out: the whole-trajectory one (gtop_validate.hip, [B][GTOP_TRAJ_REPORT]) or the
// per-segment one (gtop_segments.hip, [B][m][GTOP_SEG_REPORT]).  who: the entry's name in the NULL-buffer text
int report_on_stream(gtop_ctx *c, bool per_segment, const char *who, int B, int m, const void *d_coeff, const void *d_T,
                     int time_stride, double dt_sample, const gtop_limits *lim, void *d_out, hipStream_t s,
                     int problem_B) {
  if (int rc = gtop_validate_ready(c, B, m, time_stride, dt_sample, lim, problem_B)) return rc;
  const bool boxes = lim->use_boxes != 0;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_out) return fail(c, GTOP_ERR_INVALID, std::string(who) + ": NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  const GtopBoxList list = gtop_box_list(c, boxes ? c->nbox : 0);
  const GtopStartTimes st = gtop_start_times(c, boxes);
  const double *coeff = static_cast<const double *>(d_coeff), *T = static_cast<const double *>(d_T);
  double *out = static_cast<double *>(d_out);
  if (per_segment)
    HIPCHK(c, gtop_launch_traj_segments(c->field.grid, c->field.rec64.data(), list, B, m, coeff, T, time_stride, dt_sample,
                                        st.t0, st.stride, lim->margin, out, s));
  else
    HIPCHK(c, gtop_launch_traj_report(c->field.grid, c->field.rec64.data(), list, B, m, coeff, T, time_stride, dt_sample,
                                      st.t0, st.stride, lim->margin, out, c->simds, s));
  return GTOP_OK;
}

// Every selection: of the rows that pass the report (family 0), of those whose clearance certificate row passes
// `require` too (1), or (2, include/gtop_kinematics.h) of those whose kinematic certificate row passes it as well, with
// the clearance certificate optional.  d_cert, d_kin and require are read only by the family that has them.
const char *const kSelectNeeds[3] = {"select_best: need B >= 0, best, and report and cost for B > 0",
                                     "select_best_certified: need B >= 0, best, and report, cert and cost for B > 0",
                                     "select_best_kin_certified: need B >= 0, best, and report, kin and cost for B > 0"};

}  // namespace

int gtop_select_on_stream(gtop_ctx *c, int family, int B, const void *d_report, const void *d_cert, const void *d_kin,
                          const void *d_cost, const gtop_limits *limits, int require, void *d_pass, void *d_best,
                          void *hip_stream) {
  if (int rc = check_limits(c, limits)) return rc;
  if (family != 0 && require != GTOP_CERT_REQUIRE_SAFE && require != GTOP_CERT_REQUIRE_NOT_UNSAFE)
    return fail(c, GTOP_ERR_INVALID, family == 1 ? "select_best_certified: require is neither SAFE nor NOT_UNSAFE"
                                                 : "select_best_kin_certified: require is neither SAFE nor NOT_UNSAFE");
  if (B < 0 || !d_best || (B > 0 && (!d_report || !d_cost || (family == 1 && !d_cert) || (family == 2 && !d_kin))))
    return fail(c, GTOP_ERR_INVALID, kSelectNeeds[family]);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_select_best(B, static_cast<const double *>(d_report), static_cast<const double *>(d_cost),
                                    limits->max_vel, limits->max_acc, limits->per_axis != 0, limits->allow_out_of_map != 0,
                                    family != 0 ? static_cast<const double *>(d_cert) : nullptr,
                                    family == 2 ? static_cast<const double *>(d_kin) : nullptr, family != 0 ? require : 0,
                                    static_cast<unsigned char *>(d_pass), static_cast<int *>(d_best), c->sel_part.data(),
                                    static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

namespace {

// ---- the certificates.  One path serves the static entries and the moving ones: a static entry's three options go
// through it as moving options with the boxes off (gtop_launch_traj_certify_moving launches the static kernel for no
// boxes), and `moving` says which family the entry is of — only the moving entries look at `reserved` and at the
// start-time list, and carry their own name in the options and NULL-buffer texts ----
const gtop_certify_moving_opts *boxes_off(const gtop_certify_opts *o, gtop_certify_moving_opts *as_moving) {
  if (!o) return nullptr;   // (refused below, under the entry's name)
  *as_moving = {o->margin, o->max_depth, o->max_refine, 0, 0};
  return as_moving;
}

// the rules of a certificate of B rows, before anything is staged or launched; problem_B as gtop_start_times_fit's
int certify_ready(gtop_ctx *c, bool moving, int B, int m, int time_stride, const gtop_certify_moving_opts *o,
                  int problem_B) {
  if (!o) return fail(c, GTOP_ERR_INVALID, moving ? "certify_moving: options is NULL" : "certify: options is NULL");
  if (moving && o->reserved != 0) return fail(c, GTOP_ERR_INVALID, "certify_moving: reserved must be 0");
  if (!std::isfinite(o->margin) || o->max_depth < 0 || o->max_depth > GTOP_CERT_MAX_DEPTH || o->max_refine < 0)
    return fail(c, GTOP_ERR_INVALID, "certify: need a finite margin, max_depth in 0 .. 3, max_refine >= 0");
  if (B < 0 || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "certify: need B >= 0, 2 <= m <= 227, time_stride in {0, m}");
  if (int rc = c->field.need_records64(c)) return rc;
  if (moving && !gtop_start_times_fit(c, B, problem_B))
    return fail(c, GTOP_ERR_INVALID, "certify_moving: the number of start times does not match the batch");
  return GTOP_OK;
}

int certify_on_stream(gtop_ctx *c, bool moving, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                      const gtop_certify_moving_opts *opt, void *d_cert, void *hip_stream, int problem_B) {
  if (int rc = certify_ready(c, moving, B, m, time_stride, opt, problem_B)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_cert)
    return fail(c, GTOP_ERR_INVALID, moving ? "certify_moving: NULL buffer" : "certify: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  const bool boxes = opt->use_boxes != 0;
  const GtopStartTimes st = gtop_start_times(c, boxes);
  HIPCHK(c, gtop_launch_traj_certify_moving(c->field.grid, c->field.rec64.data(), gtop_box_list(c, boxes ? c->nbox : 0), B,
                                            m, static_cast<const double *>(d_coeff), static_cast<const double *>(d_T),
                                            time_stride, st.t0, st.stride, opt->margin, opt->max_depth, opt->max_refine,
                                            static_cast<double *>(d_cert), static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

// the options of either family as the host path carries them
struct CertifyJob {
  bool moving;
  const gtop_certify_moving_opts *opt;
};

// the same of the problem's first B rows, from x to cert on the host; rows_text: the entry's opening refusal
int certify_host(gtop_ctx *c, bool moving, const char *rows_text, int B, const double *x,
                 const gtop_certify_moving_opts *opt, double *cert) {
  const CertifyJob job = {moving, opt};
  return gtop_certificate_host(
      c, rows_text, B, x, cert != nullptr, &job,
      [](gtop_ctx *c, int B, const void *j) {
        const CertifyJob *job = static_cast<const CertifyJob *>(j);
        return certify_ready(c, job->moving, B, c->m, c->t_stride, job->opt, c->B);
      },
      [](gtop_ctx *c, int B, const void *j, double *d_rows, double *) {
        const CertifyJob *job = static_cast<const CertifyJob *>(j);
        return certify_on_stream(c, job->moving, B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, job->opt, d_rows,
                                 c->stream, c->B);
      },
      GTOP_CERT_REPORT, cert, 0, nullptr);
}

}  // namespace

int gtop_validate_ready(gtop_ctx *c, int B, int m, int time_stride, double dt_sample, const gtop_limits *lim,
                        int problem_B) {
  if (B < 0 || m < 1 || !(dt_sample > 0.0) || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "validate: need B >= 0, m >= 1, dt_sample > 0, time_stride in {0, m}");
  if (int rc = check_limits(c, lim)) return rc;
  if (!gtop_start_times_fit(c, B, problem_B))
    return fail(c, GTOP_ERR_INVALID, "validate: the number of start times does not match the batch");
  return c->field.need_records64(c);
}

int gtop_certificate_host(gtop_ctx *c, const char *rows_text, int B, const double *x, bool given, const void *job,
                          gtop_certificate_ready_fn ready, gtop_certificate_launch_fn launch, int row_cols, double *rows,
                          int seg_cols, double *segs) {
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && given, rows_text))) return rc;
  if ((rc = ready(c, B, job))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nrows = (size_t)B * row_cols, nsegs = segs ? (size_t)B * c->m * seg_cols : 0;
  HIPCHK(c, c->val_rep.reserve(nrows + nsegs));
  if ((rc = gtop_stage_coefficients(c, B, x))) return rc;
  double *d_rows = c->val_rep.data(), *d_segs = segs ? d_rows + nrows : nullptr;
  if ((rc = launch(c, B, job, d_rows, d_segs))) return rc;
  HIPCHK(c, hipMemcpyAsync(rows, d_rows, nrows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (segs) HIPCHK(c, hipMemcpyAsync(segs, d_segs, nsegs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
}

int gtop_segments_staged(gtop_ctx *c, int B, const double *x, double dt_sample, const gtop_limits *limits) {
  HIPCHK(c, c->seg_rep.reserve((size_t)B * c->m * (GTOP_SEG_REPORT + 1)));   // report | T_out
  if (int rc = gtop_stage_coefficients(c, B, x)) return rc;
  return report_on_stream(c, true, "validate_segments", B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, dt_sample,
                          limits, c->seg_rep.data(), c->stream, c->B);
}

extern "C" {

// ---- trajectory report and selection (include/gtop.h; gtop_validate.hip) ----
int gtop_validate_trajectories_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                      double dt_sample, const gtop_limits *limits, void *d_report,
                                      void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return report_on_stream(c, false, "validate", B, m, d_coeff, d_T, time_stride, dt_sample, limits, d_report,
                          static_cast<hipStream_t>(hip_stream), 0);
} GTOP_CATCH_STATUS(c)

int gtop_select_best_device(gtop_ctx *c, int B, const void *d_report, const void *d_cost, const gtop_limits *limits,
                            void *d_pass, void *d_best, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return gtop_select_on_stream(c, 0, B, d_report, nullptr, nullptr, d_cost, limits, 0, d_pass, d_best, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_select_best_certified_device(gtop_ctx *c, int B, const void *d_report, const void *d_cert, const void *d_cost,
                                      const gtop_limits *limits, int require, void *d_pass, void *d_best,
                                      void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return gtop_select_on_stream(c, 1, B, d_report, d_cert, nullptr, d_cost, limits, require, d_pass, d_best, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_validate_batch(gtop_ctx *c, int B, const double *x, double dt_sample, const gtop_limits *limits,
                        const double *cost, double *report, unsigned char *pass, int32_t best[2]) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && report, "validate_batch: 1 <= B <= problem batch, x and report required")))
    return rc;
  if (!(dt_sample > 0.0)) return fail(c, GTOP_ERR_INVALID, "validate_batch: dt_sample must be > 0");
  if ((rc = gtop_validate_ready(c, B, c->m, c->t_stride, dt_sample, limits, c->B))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nrep = (size_t)B * GTOP_TRAJ_REPORT;
  // report | cost | best (2 x int32 in one double's room) | pass (B bytes)
  HIPCHK(c, c->val_rep.reserve(nrep + B + 1 + (B + 7) / 8));
  double *d_rep = c->val_rep.data(), *d_cost = d_rep + nrep;
  int *d_best = reinterpret_cast<int *>(d_cost + B);
  unsigned char *d_pass = reinterpret_cast<unsigned char *>(d_cost + B + 1);
  if ((rc = gtop_stage_coefficients(c, B, x))) return rc;
  if ((rc = report_on_stream(c, false, "validate", B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, dt_sample, limits,
                             d_rep, c->stream, c->B)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(report, d_rep, nrep * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (cost) {
    HIPCHK(c, hipMemcpyAsync(d_cost, cost, (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = gtop_select_on_stream(c, 0, B, d_rep, nullptr, nullptr, d_cost, limits, 0, d_pass, d_best, c->stream)))
      return rc;
    if (pass) HIPCHK(c, hipMemcpyAsync(pass, d_pass, (size_t)B, hipMemcpyDeviceToHost, c->stream));
    if (best) HIPCHK(c, hipMemcpyAsync(best, d_best, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- per-segment report (gtop_segments.hip) ----
int gtop_validate_segments_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                  double dt_sample, const gtop_limits *limits, void *d_seg_report, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return report_on_stream(c, true, "validate_segments", B, m, d_coeff, d_T, time_stride, dt_sample, limits, d_seg_report,
                          static_cast<hipStream_t>(hip_stream), 0);
} GTOP_CATCH_STATUS(c)

int gtop_validate_segments(gtop_ctx *c, int B, const double *x, double dt_sample, const gtop_limits *limits,
                           double *seg_report) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && seg_report,
                              "validate_segments: 1 <= B <= problem batch, x and seg_report required")))
    return rc;
  if ((rc = gtop_validate_ready(c, B, c->m, c->t_stride, dt_sample, limits, c->B))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = gtop_segments_staged(c, B, x, dt_sample, limits))) return rc;
  HIPCHK(c, hipMemcpyAsync(seg_report, c->seg_rep.data(), (size_t)B * c->m * GTOP_SEG_REPORT * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- continuous-time clearance certificate (gtop_certify.hip): of the static field, and against the moving boxes too ----
int gtop_certify_trajectories_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                     const gtop_certify_opts *opt, void *d_cert, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  gtop_certify_moving_opts o;
  return certify_on_stream(c, false, B, m, d_coeff, d_T, time_stride, boxes_off(opt, &o), d_cert, hip_stream, 0);
} GTOP_CATCH_STATUS(c)

int gtop_certify_moving_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                               const gtop_certify_moving_opts *opt, void *d_cert, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return certify_on_stream(c, true, B, m, d_coeff, d_T, time_stride, opt, d_cert, hip_stream, 0);
} GTOP_CATCH_STATUS(c)

int gtop_certify_batch(gtop_ctx *c, int B, const double *x, const gtop_certify_opts *opt, double *cert) try {
  if (!c) return GTOP_ERR_INVALID;
  gtop_certify_moving_opts o;
  return certify_host(c, false, "certify_batch: 1 <= B <= problem batch, x and cert required", B, x, boxes_off(opt, &o),
                      cert);
} GTOP_CATCH_STATUS(c)

int gtop_certify_moving_batch(gtop_ctx *c, int B, const double *x, const gtop_certify_moving_opts *opt,
                              double *cert) try {
  if (!c) return GTOP_ERR_INVALID;
  return certify_host(c, true, "certify_moving_batch: 1 <= B <= problem batch, x and cert required", B, x, opt, cert);
} GTOP_CATCH_STATUS(c)

}  // extern "C"
