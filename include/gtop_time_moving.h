/*
 * gtop_time_moving.h — the SEGMENT TIMES as variables under the MOVING-OBSTACLE cost: the derivative of the cost with
 * respect to every segment time and to the start time, and the device optimizer of the time allocation on it.  The
 * seventh companion of gtop.h, exported from the same libgtop_hip.so.
 *
 * Why a header of its own.  gtop_time.h refuses while gtop_set_moving_cost is switched on: under absolute sample
 * times T_s moves the lookups of every later segment, and that derivative is not formed there.  It is formed here.
 * gtop_time.h, its four entry points and their refusal stay as they are; what is declared here is versioned on its
 * own (gtop_time_moving_abi_version, GTOP_TIME_MOVING_ABI_VERSION).  A library that lacks
 * gtop_time_moving_abi_version does not have this header's entry points.  gtop_time.h is included for gtop_timeopt,
 * which is reused unchanged, and for GTOP_TIMEOPT_INFO.
 *
 * What is differentiated.  The cost gtop_eval_device returns in fp64 for the context's state.  With the moving cost
 * in force (switched on and at least one box set) that state includes the box list of either kind
 * (gtop_set_moving_boxes, gtop_set_moving_box_polynomials) and the start times of gtop_set_start_times.  With the
 * mode off, or on without boxes, the result is that of gtop_time_gradient_device — the entry points of this header do
 * not refuse then — with the columns added here 0.  The conventions are those of gtop_time.h
 * (GTOP_GRADIENT_CONSISTENT), and there is one derivative whatever gtop_set_gradient_mode says.
 *
 * The clock.  Segment s of row b starts at tau_s = ((t0[b] + T_0) + ...) + T_{s-1}, summed left to right in fp64, and
 * its sample i sits at tau = tau_s + t_i: the evaluation's own expression.  So d tau / d T_s' = 1 for every earlier
 * segment s' < s, and d tau / d T_s = i / 30 for the segment's own samples (0 for a sample past the loop bound).
 *
 * The time derivative of the lookup.  The lookup is evaluateEDTWithGrad(pos, tau) as gtop_edt_query_device states it:
 * each of the 8 corner values of the cell becomes min(static value, distance from the corner voxel's centre pt to the
 * box at tau), box by box in list order, and the result is their trilinear blend.  The centre's velocity c'_k:
 *   constant-velocity list     c'_k = vel_k
 *   polynomial list            tc = clamp(tau, t1, t2); for t1 < tau < t2
 *                              c'_k = fma(fma(fma(fma(5 c5, tc, 4 c4), tc, 3 c3), tc, 2 c2), tc, c1);
 *                              outside the interval and at its ends c'_k = 0: the box stands.
 * Per axis k and corner offset o, d1[k][o] is 0 inside the slab [bmin_k, bmax_k], else the distance to the nearer
 * face, and its derivative with respect to tau is
 *   inside the slab 0          pt < bmin: +c'_k          pt > bmax: -c'_k.
 * d2 = sqrt(sum_k d1_k^2) replaces a corner value only where it is STRICTLY smaller — the static value wins a tie, and
 * the earlier box wins among boxes.  A replaced corner carries d2 > 0 ? (sum_k d1_k d1_k') / d2 : 0; a corner left
 * static carries 0.  (A box skipped by the lookup's exact skip lowers no corner.)  d dist / d tau is the trilinear
 * blend of the 8 corner derivatives with the value's own weights; it is 0 out of the map and 0 for tau < 0.
 *
 * The terms.  dist and grad of gtop_time.h's per-sample formulas are the box-lowered lookup's.  parts[b][s] has
 * GTOP_TIME_MOVING_PARTS = 6 entries (gd, vn, dt, wc as in gtop_time.h; ddist_i = d dist / d tau at sample i):
 *   [0] [1] [2] as in gtop_time.h
 *   [3] the segment's own derivative: gtop_time.h's expression + sum_i wc gd_i ddist_i (i / 30) vn_i dt
 *   [4] q_s = sum_i wc gd_i ddist_i vn_i dt: what the segment's cost gains per second of delay of its start
 *   [5] R_s: R_{m-1} = 0, R_s = R_{s+1} + q_{s+1}, summed from the last segment to the first
 *   gT[b][s] = ([2] + [3]) + [5]          gt0[b] = R_0 + q_0 (d cost / d t0[b]; may be NULL)
 * cost[b] is as in gtop_time.h.  The dyn block does not depend on tau.
 *
 * The optimizer is gtop_time.h's loop word for word — gtop_timeopt, the clamp, the acceptance rule, the codes, the
 * eight info entries — with the pass above as its evaluation; info[5] is, bit for bit, the cost
 * gtop_time_gradient_moving_device returns at T_out.  With the mode off, or on without boxes, it returns
 * gtop_optimize_times_device's bits.  The start time is not a variable: gt0 is returned so that a caller can use it.
 *
 * The kernels (csrc/gtop_time_moving.hip) are gtop_time.h's with the boxes staged once per workgroup in LDS: one
 * wavefront per trajectory, a row's bits depend on its own inputs only, every output entry is written exactly once,
 * a NaN row disturbs only itself, every loop is bounded.  The device forms enqueue one launch each: no allocation, no
 * synchronisation, capturable; the box list and the start times are read by the launch, so a list refreshed in place
 * on the stream (gtop_refresh_box_predictions_device) is picked up by a replay.  The host forms serve the first B
 * rows of the context's problem as gtop_time.h's do.
 * GTOP_ERR_STATE, nothing launched: no parameters, no field.  GTOP_ERR_INVALID, nothing launched: every
 * GTOP_ERR_INVALID of gtop_time.h (B < 0, m outside 2 .. 227, a time_stride that is neither 0 nor m, a NULL required
 * buffer with B > 0, the gtop_timeopt rules, d_T_out == d_T), and with the moving cost in force the refusals of a
 * moving-mode evaluation: a box list with a non-finite value or a negative extent, more than
 * GTOP_MOVING_COST_MAX_BOXES (32) boxes, a start-time count that fits neither 1, B nor the problem's batch.
 * B = 0 launches nothing.  fp64 only.  The gtop_group_* entry points do not forward these calls.
 */
#ifndef GTOP_TIME_MOVING_H_
#define GTOP_TIME_MOVING_H_

#include "gtop_time.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTOP_TIME_MOVING_ABI_VERSION 1
#define GTOP_TIME_MOVING_PARTS 6

/* GTOP_TIME_MOVING_ABI_VERSION of the library. */
int gtop_time_moving_abi_version(void);
int gtop_time_gradient_moving_device(gtop_ctx *ctx, int B, int m, const void *d_x, const void *d_Df, const void *d_T,
                                     int time_stride, void *d_cost /* B */, void *d_gT /* B x m */,
                                     void *d_gt0 /* may be NULL: B */,
                                     void *d_parts /* may be NULL: B x m x GTOP_TIME_MOVING_PARTS */, void *hip_stream);
int gtop_time_gradient_moving_batch(gtop_ctx *ctx, int B, const double *x, double *cost, double *gT,
                                    double *gt0 /* may be NULL */, double *parts /* may be NULL */);
int gtop_optimize_times_moving_device(gtop_ctx *ctx, const gtop_timeopt *opt, int B, int m, const void *d_x,
                                      const void *d_Df, const void *d_T, int time_stride,
                                      const void *d_T_lo /* may be NULL: B x m */, void *d_T_out /* B x m */,
                                      void *d_info /* B x GTOP_TIMEOPT_INFO */, void *hip_stream);
int gtop_optimize_times_moving(gtop_ctx *ctx, const gtop_timeopt *opt, int B, const double *x,
                               const double *T_lo /* may be NULL */, double *T_out, double *info);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_TIME_MOVING_H_ */
