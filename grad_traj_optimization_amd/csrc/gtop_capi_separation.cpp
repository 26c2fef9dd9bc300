// gtop_capi_separation.cpp — the entry points of the companion header include/gtop_separation.h: the pairwise
// separation figures (gtop_separation.hip) in a device form (no allocation, no synchronisation: capturable) and a host
// form over the problem set, and the selection of distinct candidates that reads them.
#include <cmath>

#include "gtop_ctx.h"
#include "gtop_separation.h"

namespace {

// the rules of a separation of B rows, before anything is staged or launched
int separation_ready(gtop_ctx *c, int B, int m, int time_stride, const gtop_sep_opts *o) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "separation: options is NULL");
  if (o->reserved[0] != 0 || o->reserved[1] != 0) return fail(c, GTOP_ERR_INVALID, "separation: reserved must be 0");
  if (!std::isfinite(o->t_lo) || !std::isfinite(o->dt) || !(o->dt > 0.0) || o->n_samples < 1 ||
      o->n_samples > GTOP_SEP_MAX_SAMPLES || (o->hold_ends != 0 && o->hold_ends != 1))
    return fail(c, GTOP_ERR_INVALID,
                "separation: need finite t_lo, finite dt > 0, n_samples in 1 .. 65536, hold_ends in {0, 1}");
  if (B < 0 || B > GTOP_SEP_MAX_B || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "separation: need 0 <= B <= 4096, 2 <= m <= 227, time_stride in {0, m}");
  if (B > 0 && c->t0_count > 1 && c->t0_count != B)
    return fail(c, GTOP_ERR_INVALID, "separation: the start times set are neither none, one, nor one per row");
  return GTOP_OK;
}

int separation_on_stream(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                         const gtop_sep_opts *o, void *d_pair_min, void *d_pair_max, void *d_rows, void *d_work,
                         size_t work_bytes, void *hip_stream) {
  if (int rc = separation_ready(c, B, m, time_stride, o)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_pair_min || !d_pair_max || !d_rows || !d_work)
    return fail(c, GTOP_ERR_INVALID, "separation: NULL buffer");
  if (work_bytes < gtop_separation_work_bytes(B, o->n_samples))
    return fail(c, GTOP_ERR_INVALID, "separation: work_bytes is below gtop_separation_workspace_bytes(B, n_samples)");
  const GtopStartTimes st = gtop_start_times(c);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_separation(B, m, static_cast<const double *>(d_coeff), static_cast<const double *>(d_T),
                                   time_stride, st.t0, st.stride, o->t_lo, o->dt, o->n_samples, o->hold_ends, o->radius,
                                   static_cast<double *>(d_pair_min), static_cast<double *>(d_pair_max),
                                   static_cast<double *>(d_rows), d_work, static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_sep_abi_version(void) { return GTOP_SEP_ABI_VERSION; }

int gtop_separation_workspace_bytes(int B, int n_samples, size_t *bytes) try {
  if (!bytes || B < 0 || B > GTOP_SEP_MAX_B || n_samples < 1 || n_samples > GTOP_SEP_MAX_SAMPLES) return GTOP_ERR_INVALID;
  *bytes = gtop_separation_work_bytes(B, n_samples);
  return GTOP_OK;
} GTOP_CATCH_STATUS(static_cast<gtop_ctx *>(nullptr))

int gtop_separation_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                           const gtop_sep_opts *opt, void *d_pair_min, void *d_pair_max, void *d_rows, void *d_work,
                           size_t work_bytes, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return separation_on_stream(c, B, m, d_coeff, d_T, time_stride, opt, d_pair_min, d_pair_max, d_rows, d_work,
                              work_bytes, hip_stream);
} GTOP_CATCH_STATUS(c)

// Staged as gtop_certify_batch stages: x -> d_x -> the coefficients in the coefficient scratch, the launches on the
// context's stream into a staging buffer of the context's (pair_min | pair_max | rows | workspace), copies, one wait.
int gtop_separation_batch(gtop_ctx *c, int B, const double *x, const gtop_sep_opts *opt, double *pair_min,
                          double *pair_max, double *rows) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && pair_min && pair_max && rows,
                              "separation_batch: 1 <= B <= problem batch, x, pair_min, pair_max and rows required")))
    return rc;
  if ((rc = separation_ready(c, B, c->m, c->t_stride, opt))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nmat = (size_t)B * B, nrows = (size_t)B * GTOP_SEP_ROW;
  const size_t work_bytes = gtop_separation_work_bytes(B, opt->n_samples);
  HIPCHK(c, c->sep_stage.reserve(2 * nmat + nrows + (work_bytes + sizeof(double) - 1) / sizeof(double)));
  if ((rc = gtop_stage_coefficients(c, B, x))) return rc;
  double *d_min = c->sep_stage.data(), *d_max = d_min + nmat, *d_rows = d_max + nmat, *d_work = d_rows + nrows;
  if ((rc = separation_on_stream(c, B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, opt, d_min, d_max, d_rows,
                                 d_work, work_bytes, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(pair_min, d_min, nmat * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(pair_max, d_max, nmat * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(rows, d_rows, nrows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_select_distinct_device(gtop_ctx *c, int B, const void *d_pass, const void *d_cost, const void *d_pair_max,
                                double min_gap, int K, void *d_chosen, void *d_count, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (K < 1 || K > GTOP_SEP_MAX_DISTINCT || !std::isfinite(min_gap) || B < 0 || B > GTOP_SEP_MAX_B)
    return fail(c, GTOP_ERR_INVALID, "select_distinct: need 1 <= K <= 64, a finite min_gap, 0 <= B <= 4096");
  if (B > 0 && (!d_cost || !d_pair_max || !d_chosen || !d_count))
    return fail(c, GTOP_ERR_INVALID, "select_distinct: NULL buffer");
  if (!d_chosen && !d_count) return GTOP_OK;   // (B = 0 and nowhere to write)
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_select_distinct(B, static_cast<const unsigned char *>(d_pass), static_cast<const double *>(d_cost),
                                        static_cast<const double *>(d_pair_max), min_gap, K, static_cast<int *>(d_chosen),
                                        static_cast<int *>(d_count), static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
