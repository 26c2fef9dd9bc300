// gtop_capi_boxes.cpp — the moving boxes of a context (constant-velocity and polynomial lists), the start times on
// their clock, and what reads them beside the cost term: the distance queries, the trajectory report and the selection
// — and, beside the report, the continuous-time certificates (gtop_certify.hip): of the static field, and of the field
// with the boxes.  The two remedies for a row that fails live here too: the segment-time reallocation (gtop_retime.hip)
// and the waypoint insertion (gtop_insert.hip).
#include <cmath>
#include <string>
#include <vector>

#include "gtop_ctx.h"

static_assert(GTOP_MOVING_COST_MAX_BOXES == GTOP_MOVING_MAX_BOXES, "the public box limit is the kernels' own");

namespace {

// the rows the evaluation kernels read, made once with their fixed size: the address never moves
int ensure_box_rows(gtop_ctx *c) {
  HIPCHK(c, c->box_rows.reserve((size_t)GTOP_MOVING_COST_MAX_BOXES * kBoxRowPoly));
  return GTOP_OK;
}

// the first `count` boxes of the list as the query and report launchers take it (gtop_kernels.h)
GtopBoxList box_list(const gtop_ctx *c, int count) {
  const double *b = c->boxes.data();
  const size_t n3 = (size_t)c->nbox * 3;
  if (c->box_kind == GTOP_BOXES_POLYNOMIAL) return {GTOP_BOX_LIST_POLYNOMIAL, count, nullptr, nullptr, nullptr, b};
  return {GTOP_BOX_LIST_CONST_VEL, count, b, b + n3, b + 2 * n3, nullptr};
}

}  // namespace

int gtop_moving_args(gtop_ctx *c, int B, int problem_B, GtopMovingArgs *mov) {
  if (c->nbox > GTOP_MOVING_COST_MAX_BOXES)
    return fail(c, GTOP_ERR_INVALID, "moving-obstacle cost: more boxes set than GTOP_MOVING_COST_MAX_BOXES");
  if (!c->box_rows_ok)
    return fail(c, GTOP_ERR_INVALID, "moving-obstacle cost: the box list has a non-finite value or a negative extent");
  if (!gtop_start_times_fit(c, B, problem_B))
    return fail(c, GTOP_ERR_INVALID, "moving-obstacle cost: the number of start times does not match the batch");
  mov->rows = c->box_rows.data();
  mov->nbox = c->nbox;
  mov->t0 = c->t0_count > 0 ? c->t0_dev : nullptr;
  mov->t0_stride = c->t0_count > 1 ? 1 : 0;
  mov->poly = c->box_kind == GTOP_BOXES_POLYNOMIAL;
  return GTOP_OK;
}

extern "C" {

int gtop_set_moving_boxes(gtop_ctx *c, int nbox, const double *p0, const double *vel, const double *scale) try {
  if (!c) return GTOP_ERR_INVALID;
  if (nbox < 0 || (nbox > 0 && (!p0 || !vel || !scale))) return fail(c, GTOP_ERR_INVALID, "set_moving_boxes: bad box list");
  HIPCHK(c, hipSetDevice(c->device));
  c->nbox = 0;
  c->box_kind = GTOP_BOXES_CONST_VEL;
  if (nbox == 0) return GTOP_OK;
  int rc;
  const size_t n3 = (size_t)nbox * 3;
  HIPCHK(c, c->boxes.reserve(3 * n3));
  HIPCHK(c, hipMemcpyAsync(c->boxes.data(), p0, n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->boxes.data() + n3, vel, n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->boxes.data() + 2 * n3, scale, n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // the same list as the evaluation kernels read it (the moving-obstacle cost): rows of p0, vel, scale / 2, in a
  // buffer that never moves.  A list the cost term cannot take (too long, a non-finite value, a negative extent — its
  // slab distance is written for bmin <= bmax) still serves the queries; an evaluation in moving mode refuses it.
  c->box_rows_ok = false;
  if ((rc = ensure_box_rows(c))) return rc;
  if (nbox <= GTOP_MOVING_COST_MAX_BOXES) {
    double rows[GTOP_MOVING_COST_MAX_BOXES * 9];
    bool ok = true;
    for (int b = 0; b < nbox; ++b)
      for (int k = 0; k < 3; ++k) {
        const double p = p0[3 * b + k], v = vel[3 * b + k], sc = scale[3 * b + k];
        ok = ok && std::isfinite(p) && std::isfinite(v) && std::isfinite(sc) && sc >= 0.0;
        rows[9 * b + k] = p;
        rows[9 * b + 3 + k] = v;
        rows[9 * b + 6 + k] = 0.5 * sc;
      }
    HIPCHK(c, hipMemcpyAsync(c->box_rows.data(), rows, (size_t)nbox * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->box_rows_ok = ok;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host arrays may go away
  c->nbox = nbox;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- the polynomial box list (include/gtop.h) ----
// The checks of gtop_set_moving_box_polynomials / gtop_box_polynomial_centres (scale NULL: not checked); NULL = fine.
static const char *check_box_polynomials(int nbox, const double *coef, const double *t_range, const double *scale) {
  for (int b = 0; b < nbox; ++b) {
    for (int i = 0; i < 18; ++i)
      if (!std::isfinite(coef[18 * b + i])) return "box polynomials: a coefficient is not finite";
    if (t_range) {
      const double t1 = t_range[2 * b], t2 = t_range[2 * b + 1];
      if (std::isnan(t1) || std::isnan(t2) || t1 > t2) return "box polynomials: need t1 <= t2, neither NaN";
    }
    if (scale)
      for (int k = 0; k < 3; ++k)
        if (!(std::isfinite(scale[3 * b + k]) && scale[3 * b + k] >= 0.0))
          return "box polynomials: scale must be finite and >= 0";
  }
  return nullptr;
}
// The centre's arithmetic, as gtop_edt_lookup.h states it for the device: the clamp, then Horner in explicit fmas.
static double box_polynomial_centre(const double *c6, double t1, double t2, double tau) {
  const double tc = std::fmin(std::fmax(tau, t1), t2);
  double r = c6[5];
  for (int i = 4; i >= 0; --i) r = std::fma(r, tc, c6[i]);
  return r;
}

int gtop_box_polynomial_centres(int nbox, const double *coef, const double *t_range, int ntimes, const double *times,
                                double *centres) {
  if (nbox < 0 || ntimes < 0 || (nbox > 0 && !coef) || (ntimes > 0 && !times) || (nbox > 0 && ntimes > 0 && !centres))
    return GTOP_ERR_INVALID;
  if (check_box_polynomials(nbox, coef, t_range, nullptr)) return GTOP_ERR_INVALID;
  for (int i = 0; i < ntimes; ++i)
    for (int b = 0; b < nbox; ++b) {
      const double t1 = t_range ? t_range[2 * b] : -INFINITY, t2 = t_range ? t_range[2 * b + 1] : INFINITY;
      for (int k = 0; k < 3; ++k)
        centres[((size_t)i * nbox + b) * 3 + k] = box_polynomial_centre(coef + 18 * b + 6 * k, t1, t2, times[i]);
    }
  return GTOP_OK;
}

int gtop_set_moving_box_polynomials(gtop_ctx *c, int nbox, const double *coef, const double *t_range,
                                    const double *scale) try {
  if (!c) return GTOP_ERR_INVALID;
  if (nbox < 0 || (nbox > 0 && (!coef || !scale))) return fail(c, GTOP_ERR_INVALID, "set_moving_box_polynomials: bad box list");
  // a bad list is refused here and the list in force stays (the cost bodies' slab distance is written for
  // bmin <= bmax, and a NaN centre would make a box vanish from every min)
  if (const char *why = check_box_polynomials(nbox, coef, t_range, scale)) return fail(c, GTOP_ERR_INVALID, why);
  HIPCHK(c, hipSetDevice(c->device));
  if (nbox == 0) {
    c->nbox = 0;
    c->box_kind = GTOP_BOXES_CONST_VEL;
    return GTOP_OK;
  }
  std::vector<double> rows((size_t)nbox * kBoxRowPoly);
  for (int b = 0; b < nbox; ++b) {
    double *r = &rows[(size_t)b * kBoxRowPoly];
    for (int i = 0; i < 18; ++i) r[i] = coef[18 * b + i];
    for (int k = 0; k < 3; ++k) r[18 + k] = 0.5 * scale[3 * b + k];
    r[21] = t_range ? t_range[2 * b] : -INFINITY;
    r[22] = t_range ? t_range[2 * b + 1] : INFINITY;
    r[23] = 0.0;
  }
  int rc;
  c->nbox = 0;   // (a failure below leaves no list rather than half of one)
  c->box_kind = GTOP_BOXES_CONST_VEL;
  c->box_rows_ok = false;
  HIPCHK(c, c->boxes.reserve(rows.size()));
  if ((rc = ensure_box_rows(c))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->boxes.data(), rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // the same rows where the evaluation kernels read them, in the buffer that never moves; a list too long for the cost
  // term still serves the queries and the report, and an evaluation in moving mode refuses it
  if (nbox <= GTOP_MOVING_COST_MAX_BOXES) {
    HIPCHK(c, hipMemcpyAsync(c->box_rows.data(), rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->box_rows_ok = true;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));   // `rows` goes away
  c->nbox = nbox;
  c->box_kind = GTOP_BOXES_POLYNOMIAL;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_get_moving_box_kind(const gtop_ctx *c, int *kind, int *nbox) {
  if (!c || !kind || !nbox) return GTOP_ERR_INVALID;
  *kind = c->box_kind;
  *nbox = c->nbox;
  return GTOP_OK;
}

int gtop_set_moving_cost(gtop_ctx *c, int enable) try {
  if (!c) return GTOP_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (enable && (rc = ensure_box_rows(c))) return rc;   // (so that no evaluation ever allocates for it)
  c->moving_cost = enable != 0;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_get_moving_cost(const gtop_ctx *c, int *enable) {
  if (!c || !enable) return GTOP_ERR_INVALID;
  *enable = c->moving_cost;
  return GTOP_OK;
}

int gtop_set_start_times(gtop_ctx *c, int count, const double *t0_host) try {
  if (!c) return GTOP_ERR_INVALID;
  if (count < 0) return fail(c, GTOP_ERR_INVALID, "set_start_times: count < 0");
  if (count == 0 || !t0_host) {
    c->t0_count = 0;
    c->t0_dev = nullptr;
    return GTOP_OK;
  }
  for (int i = 0; i < count; ++i)
    if (!(std::isfinite(t0_host[i]) && t0_host[i] >= 0.0))
      return fail(c, GTOP_ERR_INVALID, "set_start_times: start times must be finite and >= 0");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->t0_own.reserve((size_t)count));
  HIPCHK(c, hipMemcpyAsync(c->t0_own.data(), t0_host, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host array may go away
  c->t0_dev = c->t0_own.data();
  c->t0_count = count;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_set_start_times_device(gtop_ctx *c, int count, const void *d_t0) try {
  if (!c) return GTOP_ERR_INVALID;
  if (count < 0) return fail(c, GTOP_ERR_INVALID, "set_start_times_device: count < 0");
  if (count == 0 || !d_t0) {
    c->t0_count = 0;
    c->t0_dev = nullptr;
    return GTOP_OK;
  }
  c->t0_dev = static_cast<const double *>(d_t0);   // borrowed: read by the launches, never copied
  c->t0_count = count;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// The interpolating query, or (coarse) EDTEnvironment::evaluateCoarseEDT (src/edt_environment.cpp:124-136): the voxel's
// own distance from the boundary copy, no gradient.  who: the entry's name in its error texts.
static int edt_query_on_stream(gtop_ctx *c, const char *who, int N, const void *d_pos, const void *d_time, void *d_dist,
                               void *d_grad, bool coarse, void *hip_stream) {
  if (int rc = coarse ? c->field.need_boundary(c) : c->field.need_records64(c)) return rc;
  if (N < 0) return fail(c, GTOP_ERR_INVALID, std::string(who) + ": N < 0");
  if (N == 0) return GTOP_OK;
  if (!d_pos || !d_time || !d_dist || (!coarse && !d_grad)) return fail(c, GTOP_ERR_INVALID, std::string(who) + ": NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_edt_query(c->field.grid, c->field.sdf64, c->field.rec64.data(), box_list(c, c->nbox), N,
                                  static_cast<const double *>(d_pos), static_cast<const double *>(d_time),
                                  static_cast<double *>(d_dist), coarse ? nullptr : static_cast<double *>(d_grad),
                                  static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

// the same from host arrays, through the staging buffer: pos | time | dist | grad
static int edt_query_host(gtop_ctx *c, const char *who, int N, const double *pos, const double *time, double *dist,
                          double *grad, bool coarse) {
  if (N < 0 || (N > 0 && (!pos || !time || !dist || (!coarse && !grad))))
    return fail(c, GTOP_ERR_INVALID, std::string(who) + ": bad arguments");
  if (N == 0) return GTOP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)N;
  HIPCHK(c, c->d_q.reserve((coarse ? 5 : 8) * n));
  double *dp = c->d_q.data(), *dt = dp + 3 * n, *dd = dt + n, *dg = dd + n;
  HIPCHK(c, hipMemcpyAsync(dp, pos, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dt, time, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (int rc = edt_query_on_stream(c, who, N, dp, dt, dd, dg, coarse, c->stream)) return rc;
  HIPCHK(c, hipMemcpyAsync(dist, dd, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (!coarse) HIPCHK(c, hipMemcpyAsync(grad, dg, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
}

int gtop_edt_query_device(gtop_ctx *c, int N, const void *d_pos, const void *d_time, void *d_dist, void *d_grad,
                          void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return edt_query_on_stream(c, "edt_query", N, d_pos, d_time, d_dist, d_grad, false, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_edt_query(gtop_ctx *c, int N, const double *pos, const double *time, double *dist, double *grad) try {
  if (!c) return GTOP_ERR_INVALID;
  return edt_query_host(c, "edt_query", N, pos, time, dist, grad, false);
} GTOP_CATCH_STATUS(c)

int gtop_edt_coarse_query_device(gtop_ctx *c, int N, const void *d_pos, const void *d_time, void *d_dist,
                                 void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return edt_query_on_stream(c, "edt_coarse_query", N, d_pos, d_time, d_dist, nullptr, true, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_edt_coarse_query(gtop_ctx *c, int N, const double *pos, const double *time, double *dist) try {
  if (!c) return GTOP_ERR_INVALID;
  return edt_query_host(c, "edt_coarse_query", N, pos, time, dist, nullptr, true);
} GTOP_CATCH_STATUS(c)

// ---- trajectory report and selection (include/gtop.h; gtop_validate.hip) ----
static int check_limits(gtop_ctx *c, const gtop_limits *lim) {
  if (!lim) return fail(c, GTOP_ERR_INVALID, "validate: limits is NULL");
  if (!std::isfinite(lim->margin) || !std::isfinite(lim->max_vel) || !std::isfinite(lim->max_acc))
    return fail(c, GTOP_ERR_INVALID, "validate: margin, max_vel and max_acc must be finite");
  return GTOP_OK;
}

// What a report of B rows asks of its arguments and of the context, before anything is staged or launched.
// problem_B: the batch of gtop_set_problem when the rows are its first B (a per-trajectory start-time list of that
// length serves them), 0 otherwise
static int validate_ready(gtop_ctx *c, int B, int m, int time_stride, double dt_sample, const gtop_limits *lim,
                          int problem_B) {
  if (B < 0 || m < 1 || !(dt_sample > 0.0) || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "validate: need B >= 0, m >= 1, dt_sample > 0, time_stride in {0, m}");
  if (int rc = check_limits(c, lim)) return rc;
  if (!gtop_start_times_fit(c, B, problem_B))
    return fail(c, GTOP_ERR_INVALID, "validate: the number of start times does not match the batch");
  return c->field.need_records64(c);
}

// Either sampled report of B rows into d_out: the whole-trajectory one (gtop_validate.hip, [B][GTOP_TRAJ_REPORT]) or the
// per-segment one (gtop_segments.hip, [B][m][GTOP_SEG_REPORT]).  who: the entry's name in the NULL-buffer text
static int report_on_stream(gtop_ctx *c, bool per_segment, const char *who, int B, int m, const void *d_coeff,
                            const void *d_T, int time_stride, double dt_sample, const gtop_limits *lim, void *d_out,
                            hipStream_t s, int problem_B) {
  if (int rc = validate_ready(c, B, m, time_stride, dt_sample, lim, problem_B)) return rc;
  const bool boxes = lim->use_boxes != 0;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_out) return fail(c, GTOP_ERR_INVALID, std::string(who) + ": NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  const GtopBoxList list = box_list(c, boxes ? c->nbox : 0);
  const double *coeff = static_cast<const double *>(d_coeff), *T = static_cast<const double *>(d_T);
  const double *t0 = (boxes && c->t0_count > 0) ? c->t0_dev : nullptr;
  const int t0_stride = c->t0_count > 1 ? 1 : 0;
  double *out = static_cast<double *>(d_out);
  if (per_segment)
    HIPCHK(c, gtop_launch_traj_segments(c->field.grid, c->field.rec64.data(), list, B, m, coeff, T, time_stride, dt_sample,
                                        t0, t0_stride, lim->margin, out, s));
  else
    HIPCHK(c, gtop_launch_traj_report(c->field.grid, c->field.rec64.data(), list, B, m, coeff, T, time_stride, dt_sample,
                                      t0, t0_stride, lim->margin, out, c->simds, s));
  return GTOP_OK;
}

// x of the problem's first B rows -> d_x -> their coefficients, left in mma_g (the coefficient scratch); no
// synchronisation
static int stage_coefficients(gtop_ctx *c, int B, const double *x) {
  const int m = c->m;
  const size_t n = 9 * (size_t)(m - 1), ncoef = (size_t)B * m * 18;
  HIPCHK(c, c->mma_g.reserve(ncoef > (size_t)B * n ? ncoef : (size_t)B * n));
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return gtop_coefficients_device(c, B, m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, c->mma_g.data(),
                                  c->stream);
}

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
  int rc;
  if ((rc = check_limits(c, limits))) return rc;
  if (B < 0 || !d_best || (B > 0 && (!d_report || !d_cost)))
    return fail(c, GTOP_ERR_INVALID, "select_best: need B >= 0, best, and report and cost for B > 0");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_select_best(B, static_cast<const double *>(d_report), static_cast<const double *>(d_cost),
                                    limits->max_vel, limits->max_acc, limits->per_axis != 0, limits->allow_out_of_map != 0,
                                    nullptr, 0, static_cast<unsigned char *>(d_pass), static_cast<int *>(d_best), c->sel_part.data(),
                                    static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_validate_batch(gtop_ctx *c, int B, const double *x, double dt_sample, const gtop_limits *limits,
                        const double *cost, double *report, unsigned char *pass, int32_t best[2]) try {
  if (!c) return GTOP_ERR_INVALID;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  if (B < 1 || B > c->B || !x || !report)
    return fail(c, GTOP_ERR_INVALID, "validate_batch: 1 <= B <= problem batch, x and report required");
  if (!(dt_sample > 0.0)) return fail(c, GTOP_ERR_INVALID, "validate_batch: dt_sample must be > 0");
  int rc = validate_ready(c, B, c->m, c->t_stride, dt_sample, limits, c->B);   // (before anything is staged)
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nrep = (size_t)B * GTOP_TRAJ_REPORT;
  // report | cost | best (2 x int32 in one double's room) | pass (B bytes)
  HIPCHK(c, c->val_rep.reserve(nrep + B + 1 + (B + 7) / 8));
  double *d_rep = c->val_rep.data(), *d_cost = d_rep + nrep;
  int *d_best = reinterpret_cast<int *>(d_cost + B);
  unsigned char *d_pass = reinterpret_cast<unsigned char *>(d_cost + B + 1);
  if ((rc = stage_coefficients(c, B, x))) return rc;
  if ((rc = report_on_stream(c, false, "validate", B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, dt_sample, limits,
                             d_rep, c->stream, c->B)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(report, d_rep, nrep * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (cost) {
    HIPCHK(c, hipMemcpyAsync(d_cost, cost, (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = gtop_select_best_device(c, B, d_rep, d_cost, limits, d_pass, d_best, c->stream))) return rc;
    if (pass) HIPCHK(c, hipMemcpyAsync(pass, d_pass, (size_t)B, hipMemcpyDeviceToHost, c->stream));
    if (best) HIPCHK(c, hipMemcpyAsync(best, d_best, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- continuous-time clearance certificate (gtop_certify.hip) ----
// the rules of a certificate of B rows, before anything is staged or launched
static int certify_ready(gtop_ctx *c, int B, int m, int time_stride, const gtop_certify_opts *o) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "certify: options is NULL");
  if (!std::isfinite(o->margin) || o->max_depth < 0 || o->max_depth > GTOP_CERT_MAX_DEPTH || o->max_refine < 0)
    return fail(c, GTOP_ERR_INVALID, "certify: need a finite margin, max_depth in 0 .. 3, max_refine >= 0");
  if (B < 0 || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "certify: need B >= 0, 2 <= m <= 227, time_stride in {0, m}");
  return c->field.need_records64(c);
}

int gtop_certify_trajectories_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                     const gtop_certify_opts *opt, void *d_cert, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = certify_ready(c, B, m, time_stride, opt)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_cert) return fail(c, GTOP_ERR_INVALID, "certify: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_traj_certify(c->field.grid, c->field.rec64.data(), B, m, static_cast<const double *>(d_coeff),
                                     static_cast<const double *>(d_T), time_stride, opt->margin, opt->max_depth,
                                     opt->max_refine, static_cast<double *>(d_cert), static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_certify_batch(gtop_ctx *c, int B, const double *x, const gtop_certify_opts *opt, double *cert) try {
  if (!c) return GTOP_ERR_INVALID;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  if (B < 1 || B > c->B || !x || !cert)
    return fail(c, GTOP_ERR_INVALID, "certify_batch: 1 <= B <= problem batch, x and cert required");
  int rc = certify_ready(c, B, c->m, c->t_stride, opt);   // (before anything is staged)
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t ncert = (size_t)B * GTOP_CERT_REPORT;
  HIPCHK(c, c->val_rep.reserve(ncert));
  if ((rc = stage_coefficients(c, B, x))) return rc;
  if ((rc = gtop_certify_trajectories_device(c, B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, opt,
                                             c->val_rep.data(), c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(cert, c->val_rep.data(), ncert * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- the certificate against the moving boxes too (gtop_certify.hip, traj_certify_moving_kernel) ----
// problem_B: as validate_ready's
static int certify_moving_ready(gtop_ctx *c, int B, int m, int time_stride, const gtop_certify_moving_opts *o,
                                int problem_B) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "certify_moving: options is NULL");
  if (o->reserved != 0) return fail(c, GTOP_ERR_INVALID, "certify_moving: reserved must be 0");
  const gtop_certify_opts base = {o->margin, o->max_depth, o->max_refine};
  if (int rc = certify_ready(c, B, m, time_stride, &base)) return rc;
  if (!gtop_start_times_fit(c, B, problem_B))
    return fail(c, GTOP_ERR_INVALID, "certify_moving: the number of start times does not match the batch");
  return GTOP_OK;
}

static int certify_moving_on_stream(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                    const gtop_certify_moving_opts *opt, void *d_cert, hipStream_t s, int problem_B) {
  if (int rc = certify_moving_ready(c, B, m, time_stride, opt, problem_B)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_cert) return fail(c, GTOP_ERR_INVALID, "certify_moving: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  const bool boxes = opt->use_boxes != 0;
  const double *t0 = (boxes && c->t0_count > 0) ? c->t0_dev : nullptr;
  HIPCHK(c, gtop_launch_traj_certify_moving(c->field.grid, c->field.rec64.data(), box_list(c, boxes ? c->nbox : 0), B, m,
                                            static_cast<const double *>(d_coeff), static_cast<const double *>(d_T),
                                            time_stride, t0, c->t0_count > 1 ? 1 : 0, opt->margin, opt->max_depth,
                                            opt->max_refine, static_cast<double *>(d_cert), s));
  return GTOP_OK;
}

int gtop_certify_moving_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                               const gtop_certify_moving_opts *opt, void *d_cert, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return certify_moving_on_stream(c, B, m, d_coeff, d_T, time_stride, opt, d_cert, static_cast<hipStream_t>(hip_stream), 0);
} GTOP_CATCH_STATUS(c)

int gtop_certify_moving_batch(gtop_ctx *c, int B, const double *x, const gtop_certify_moving_opts *opt,
                              double *cert) try {
  if (!c) return GTOP_ERR_INVALID;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  if (B < 1 || B > c->B || !x || !cert)
    return fail(c, GTOP_ERR_INVALID, "certify_moving_batch: 1 <= B <= problem batch, x and cert required");
  int rc = certify_moving_ready(c, B, c->m, c->t_stride, opt, c->B);   // (before anything is staged)
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t ncert = (size_t)B * GTOP_CERT_REPORT;
  HIPCHK(c, c->val_rep.reserve(ncert));
  if ((rc = stage_coefficients(c, B, x))) return rc;
  if ((rc = certify_moving_on_stream(c, B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, opt, c->val_rep.data(),
                                     c->stream, c->B)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(cert, c->val_rep.data(), ncert * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_select_best_certified_device(gtop_ctx *c, int B, const void *d_report, const void *d_cert, const void *d_cost,
                                      const gtop_limits *limits, int require, void *d_pass, void *d_best,
                                      void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = check_limits(c, limits)) return rc;
  if (require != GTOP_CERT_REQUIRE_SAFE && require != GTOP_CERT_REQUIRE_NOT_UNSAFE)
    return fail(c, GTOP_ERR_INVALID, "select_best_certified: require is neither SAFE nor NOT_UNSAFE");
  if (B < 0 || !d_best || (B > 0 && (!d_report || !d_cert || !d_cost)))
    return fail(c, GTOP_ERR_INVALID, "select_best_certified: need B >= 0, best, and report, cert and cost for B > 0");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_select_best(B, static_cast<const double *>(d_report), static_cast<const double *>(d_cost),
                                    limits->max_vel, limits->max_acc, limits->per_axis != 0, limits->allow_out_of_map != 0,
                                    static_cast<const double *>(d_cert), require, static_cast<unsigned char *>(d_pass),
                                    static_cast<int *>(d_best), c->sel_part.data(), static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- per-segment report (gtop_segments.hip) and segment-time reallocation (gtop_retime.hip) ----
int gtop_validate_segments_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                  double dt_sample, const gtop_limits *limits, void *d_seg_report, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return report_on_stream(c, true, "validate_segments", B, m, d_coeff, d_T, time_stride, dt_sample, limits, d_seg_report,
                          static_cast<hipStream_t>(hip_stream), 0);
} GTOP_CATCH_STATUS(c)

// x of the problem's first B rows -> their coefficients -> the segment report in seg_rep; no synchronisation
static int segments_staged(gtop_ctx *c, int B, const double *x, double dt_sample, const gtop_limits *limits) {
  HIPCHK(c, c->seg_rep.reserve((size_t)B * c->m * (GTOP_SEG_REPORT + 1)));   // report | T_out
  if (int rc = stage_coefficients(c, B, x)) return rc;
  return report_on_stream(c, true, "validate_segments", B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, dt_sample,
                          limits, c->seg_rep.data(), c->stream, c->B);
}

int gtop_validate_segments(gtop_ctx *c, int B, const double *x, double dt_sample, const gtop_limits *limits,
                           double *seg_report) try {
  if (!c) return GTOP_ERR_INVALID;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  if (B < 1 || B > c->B || !x || !seg_report)
    return fail(c, GTOP_ERR_INVALID, "validate_segments: 1 <= B <= problem batch, x and seg_report required");
  int rc = validate_ready(c, B, c->m, c->t_stride, dt_sample, limits, c->B);   // (before anything is staged)
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = segments_staged(c, B, x, dt_sample, limits))) return rc;
  HIPCHK(c, hipMemcpyAsync(seg_report, c->seg_rep.data(), (size_t)B * c->m * GTOP_SEG_REPORT * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// the rules of a gtop_retime, before anything is staged or launched
static int check_retime(gtop_ctx *c, const gtop_retime *o) {
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
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  int rc = check_retime(c, opt);
  if (rc) return rc;
  if (B < 1 || B > c->B || !x || !T_out)
    return fail(c, GTOP_ERR_INVALID, "reallocate_times: 1 <= B <= problem batch, x and T_out required");
  const int m = c->m;
  const size_t n = 9 * (size_t)(m - 1), nT = (size_t)B * m;
  const bool limits_mode = opt->mode == GTOP_RETIME_LIMITS;
  if (limits_mode && (rc = validate_ready(c, B, m, c->t_stride, dt_sample, limits, c->B))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (limits_mode) {
    if ((rc = segments_staged(c, B, x, dt_sample, limits))) return rc;
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
// the rules of a gtop_insert and of a call of B rows of m segments, before anything is staged or launched; which of the
// optional buffers are given: bounds (lb and ub), bounds_out (lb_out and ub_out)
static int insert_ready(gtop_ctx *c, const gtop_insert *o, int B, int m, int time_stride, int when_stride, bool has_lb,
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
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  const int m = c->m;
  int rc = insert_ready(c, opt, B, m, c->t_stride, 1, lb, ub, lb_out, ub_out);   // (before anything is staged)
  if (rc) return rc;
  const bool at_time = opt->mode == GTOP_INSERT_AT_TIME;
  if (B < 1 || B > c->B || !x || !x_out || !T_out || (at_time && !when))
    return fail(c, GTOP_ERR_INVALID,
                "insert_waypoints: 1 <= B <= problem batch; x, x_out and T_out required, when under AT_TIME");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n_old = (size_t)B * 9 * (m - 1), n_new = (size_t)B * 9 * m, n_T = (size_t)B * (m + 1);
  const size_t n_info = (size_t)B * GTOP_INSERT_INFO;
  // when | lb | ub | x_out | T_out | lb_out | ub_out | info
  HIPCHK(c, c->seg_rep.reserve(B + 2 * n_old + n_new + n_T + 2 * n_new + n_info));
  double *d_when = c->seg_rep.data(), *d_lb = d_when + B, *d_ub = d_lb + n_old, *d_x_out = d_ub + n_old;
  double *d_T_out = d_x_out + n_new, *d_lb_out = d_T_out + n_T, *d_ub_out = d_lb_out + n_new, *d_info = d_ub_out + n_new;
  if ((rc = stage_coefficients(c, B, x))) return rc;
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
