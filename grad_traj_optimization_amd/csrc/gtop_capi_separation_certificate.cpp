// gtop_capi_separation_certificate.cpp — the entry points of the companion header
// include/gtop_separation_certificate.h: the continuous-time certificate of pairwise separation
// (gtop_separation_certificate.hip) in a device form (no allocation, no synchronisation: capturable) and a host form
// over the problem set.
#include <cmath>

#include "gtop_ctx.h"
#include "gtop_separation_certificate.h"

namespace {

// the rules of a separation certificate of B rows, before anything is staged or launched
int sepcert_ready(gtop_ctx *c, int B, int m, int time_stride, const gtop_sepcert_opts *o) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "certify_separation: options is NULL");
  if (o->reserved[0] != 0 || o->reserved[1] != 0)
    return fail(c, GTOP_ERR_INVALID, "certify_separation: reserved must be 0");
  if (!std::isfinite(o->min_sep) || !(o->min_sep > 0.0) || !(o->t_lo <= o->t_hi) ||
      (o->hold_ends != 0 && o->hold_ends != 1) || (o->cull != 0 && o->cull != 1) ||
      (o->hold_ends == 1 && (!std::isfinite(o->t_lo) || !std::isfinite(o->t_hi))))
    return fail(c, GTOP_ERR_INVALID,
                "certify_separation: need finite min_sep > 0, t_lo <= t_hi (finite with hold_ends), hold_ends and cull in {0, 1}");
  if (o->max_depth < 0 || o->max_depth > GTOP_CERT_MAX_DEPTH || o->max_refine < 0)
    return fail(c, GTOP_ERR_INVALID, "certify_separation: need max_depth in 0 .. 3, max_refine >= 0");
  if (B < 0 || B > GTOP_SEPCERT_MAX_B || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "certify_separation: need 0 <= B <= 2048, 2 <= m <= 227, time_stride in {0, m}");
  if (B > 0 && c->t0_count > 1 && c->t0_count != B)
    return fail(c, GTOP_ERR_INVALID, "certify_separation: the start times set are neither none, one, nor one per row");
  return GTOP_OK;
}

int sepcert_on_stream(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                      const gtop_sepcert_opts *o, void *d_pairs, void *d_rows, void *d_work, size_t work_bytes,
                      void *hip_stream) {
  if (int rc = sepcert_ready(c, B, m, time_stride, o)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_pairs || !d_rows || !d_work)
    return fail(c, GTOP_ERR_INVALID, "certify_separation: NULL buffer");
  if (work_bytes < gtop_sepcert_work_bytes(B))
    return fail(c, GTOP_ERR_INVALID, "certify_separation: work_bytes is below gtop_sepcert_workspace_bytes(B)");
  const GtopStartTimes st = gtop_start_times(c);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_certify_separation(B, m, static_cast<const double *>(d_coeff), static_cast<const double *>(d_T),
                                           time_stride, st.t0, st.stride, o->min_sep, o->t_lo, o->t_hi, o->max_depth,
                                           o->max_refine, o->hold_ends, o->cull, static_cast<double *>(d_pairs),
                                           static_cast<double *>(d_rows), d_work, static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_sepcert_abi_version(void) { return GTOP_SEPCERT_ABI_VERSION; }

int gtop_sepcert_workspace_bytes(int B, size_t *bytes) try {
  if (!bytes || B < 0 || B > GTOP_SEPCERT_MAX_B) return GTOP_ERR_INVALID;
  *bytes = gtop_sepcert_work_bytes(B);
  return GTOP_OK;
} GTOP_CATCH_STATUS(static_cast<gtop_ctx *>(nullptr))

int gtop_certify_separation_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                   const gtop_sepcert_opts *opt, void *d_pairs, void *d_rows, void *d_work,
                                   size_t work_bytes, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return sepcert_on_stream(c, B, m, d_coeff, d_T, time_stride, opt, d_pairs, d_rows, d_work, work_bytes, hip_stream);
} GTOP_CATCH_STATUS(c)

// Staged as gtop_separation_batch stages: x -> d_x -> the coefficients in the coefficient scratch, the launches on the
// context's stream into a staging buffer of the context's (pairs | rows | workspace), copies, one wait.
int gtop_certify_separation_batch(gtop_ctx *c, int B, const double *x, const gtop_sepcert_opts *opt, double *pairs,
                                  double *rows) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc;
  if ((rc = gtop_problem_rows(c, B, x && pairs && rows,
                              "certify_separation_batch: 1 <= B <= problem batch, x, pairs and rows required")))
    return rc;
  if ((rc = sepcert_ready(c, B, c->m, c->t_stride, opt))) return rc;   // (before anything is staged)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t npairs = (size_t)B * B * GTOP_SEPCERT_PAIR, nrows = (size_t)B * GTOP_SEPCERT_ROW;
  const size_t work_bytes = gtop_sepcert_work_bytes(B);
  HIPCHK(c, c->sepcert_stage.reserve(npairs + nrows + (work_bytes + sizeof(double) - 1) / sizeof(double)));
  if ((rc = gtop_stage_coefficients(c, B, x))) return rc;
  double *d_pairs = c->sepcert_stage.data(), *d_rows = d_pairs + npairs, *d_work = d_rows + nrows;
  if ((rc = sepcert_on_stream(c, B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride, opt, d_pairs, d_rows, d_work,
                              work_bytes, c->stream)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(pairs, d_pairs, npairs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(rows, d_rows, nrows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
