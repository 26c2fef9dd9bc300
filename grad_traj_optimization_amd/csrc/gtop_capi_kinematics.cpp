// gtop_capi_kinematics.cpp — the entry points of the companion header include/gtop_kinematics.h: the continuous-time
// kinematic certificate (gtop_kinematics.hip) in a device form (no allocation, no synchronisation: capturable) and a
// host form over the problem set, and the selection that takes its rows.  The host form goes through the one
// certificate host path, the selection through the one selection, of gtop_capi_report.cpp.
#include <cmath>

#include "gtop_ctx.h"
#include "gtop_kinematics.h"

namespace {

// the rules of a kinematic certificate of B rows, before anything is staged or launched
int kinematics_ready(gtop_ctx *c, int B, int m, int time_stride, const gtop_kin_opts *o) {
  if (!o) return fail(c, GTOP_ERR_INVALID, "certify_kinematics: options is NULL");
  if (o->reserved != 0) return fail(c, GTOP_ERR_INVALID, "certify_kinematics: reserved must be 0");
  if (o->max_depth < 0 || o->max_depth > GTOP_CERT_MAX_DEPTH || o->max_refine < 0 || std::isinf(o->max_vel) ||
      std::isinf(o->max_acc))
    return fail(c, GTOP_ERR_INVALID,
                "certify_kinematics: need max_depth in 0 .. 3, max_refine >= 0, no infinite limit (<= 0 or NaN: off)");
  if (B < 0 || m < 2 || m > 227 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "certify_kinematics: need B >= 0, 2 <= m <= 227, time_stride in {0, m}");
  return GTOP_OK;
}

int kinematics_on_stream(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                         const gtop_kin_opts *o, void *d_kin, void *d_seg, void *hip_stream) {
  if (int rc = kinematics_ready(c, B, m, time_stride, o)) return rc;
  if (B == 0) return GTOP_OK;
  if (!d_coeff || !d_T || !d_kin) return fail(c, GTOP_ERR_INVALID, "certify_kinematics: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_traj_kinematics(B, m, static_cast<const double *>(d_coeff), static_cast<const double *>(d_T),
                                        time_stride, o->max_vel, o->max_acc, o->per_axis != 0, o->max_depth,
                                        o->max_refine, static_cast<double *>(d_kin), static_cast<double *>(d_seg),
                                        static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_kin_abi_version(void) { return GTOP_KIN_ABI_VERSION; }

int gtop_certify_kinematics_device(gtop_ctx *c, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                   const gtop_kin_opts *opt, void *d_kin, void *d_seg, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return kinematics_on_stream(c, B, m, d_coeff, d_T, time_stride, opt, d_kin, d_seg, hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_certify_kinematics_batch(gtop_ctx *c, int B, const double *x, const gtop_kin_opts *opt, double *kin,
                                  double *seg) try {
  if (!c) return GTOP_ERR_INVALID;
  return gtop_certificate_host(
      c, "certify_kinematics_batch: 1 <= B <= problem batch, x and kin required", B, x, kin != nullptr, opt,
      [](gtop_ctx *c, int B, const void *o) {
        return kinematics_ready(c, B, c->m, c->t_stride, static_cast<const gtop_kin_opts *>(o));
      },
      [](gtop_ctx *c, int B, const void *o, double *d_rows, double *d_segs) {
        return kinematics_on_stream(c, B, c->m, c->mma_g.data(), c->d_T.data(), c->t_stride,
                                    static_cast<const gtop_kin_opts *>(o), d_rows, d_segs, c->stream);
      },
      GTOP_KIN_REPORT, kin, GTOP_KIN_SEG, seg);
} GTOP_CATCH_STATUS(c)

int gtop_select_best_kin_certified_device(gtop_ctx *c, int B, const void *d_report, const void *d_cert,
                                          const void *d_kin, const void *d_cost, const gtop_limits *limits, int require,
                                          void *d_pass, void *d_best, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  return gtop_select_on_stream(c, 2, B, d_report, d_cert, d_kin, d_cost, limits, require, d_pass, d_best, hip_stream);
} GTOP_CATCH_STATUS(c)

}  // extern "C"
