// gtop_capi_boxes.cpp — the moving boxes of a context (constant-velocity and polynomial lists), the switch of their cost
// term, the start times on their clock, and the distance queries that read them beside the cost term.  The reports and
// certificates that read them too: gtop_capi_report.cpp.
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

}  // namespace

int gtop_moving_args(gtop_ctx *c, int B, int problem_B, GtopMovingArgs *mov) {
  if (c->nbox > GTOP_MOVING_COST_MAX_BOXES)
    return fail(c, GTOP_ERR_INVALID, "moving-obstacle cost: more boxes set than GTOP_MOVING_COST_MAX_BOXES");
  if (!c->box_rows_ok)
    return fail(c, GTOP_ERR_INVALID, "moving-obstacle cost: the box list has a non-finite value or a negative extent");
  if (!gtop_start_times_fit(c, B, problem_B))
    return fail(c, GTOP_ERR_INVALID, "moving-obstacle cost: the number of start times does not match the batch");
  const GtopStartTimes st = gtop_start_times(c);
  mov->rows = c->box_rows.data();
  mov->nbox = c->nbox;
  mov->t0 = st.t0;
  mov->t0_stride = st.stride;
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
  HIPCHK(c, gtop_launch_edt_query(c->field.grid, c->field.sdf64, c->field.rec64.data(), gtop_box_list(c, c->nbox), N,
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

}  // extern "C"
