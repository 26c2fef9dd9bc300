/*
 * gtop_joint.h — WAYPOINT DERIVATIVES AND SEGMENT TIMES TOGETHER: the cost with its
 * derivative with respect to every free waypoint value x and every segment time T from
 * one pass, and a device optimizer of the stacked variable z = [x | T].  A companion of
 * gtop.h, exported from the same libgtop_hip.so.
 *
 * Why a header of its own.  gtop.h is a frozen surface (see gtop_kinematics.h).  What
 * is declared here is versioned on its own (gtop_joint_abi_version,
 * GTOP_JOINT_ABI_VERSION) and adds nothing to gtop.h or to the other companion
 * headers.  A library that lacks gtop_joint_abi_version does not have this header's
 * entry points.  gtop.h is included for gtop_ctx and the status codes.
 *
 * The cost, gT and parts are gtop_time.h's, word for word: the fp64 cost of
 * gtop_eval_device for the context's gtop_params under the conventions of
 * GTOP_GRADIENT_CONSISTENT (the float round trips as the identity, the field as
 * differentiable inside a cell, out of the map dist = -1 and the field gradient 0,
 * d vn / d v = v / vn, sgn(+-0) = 0, the sample count held, a segment with T < 0.0301
 * on the replayed addition chain).  There is one derivative, whatever
 * gtop_set_gradient_mode says, and a signed field is read as it is.  cost[b], gT[b][s]
 * and parts[b][s][GTOP_TIME_PARTS] carry the bits gtop_time_gradient_device returns
 * for the same row: the kernel evaluates that header's expressions, not a restatement.
 *
 * gx is new.  gx[b][i + axis (3m - 3)] is the derivative with respect to
 * x[b][i + axis (3m - 3)], i = 3 (w - 1) + (0 position, 1 velocity, 2 acceleration) of
 * interior waypoint w = 1 .. m - 1.  No + 1e-5 is added (that constant belongs to the
 * callback's gradient vector, as gtop_time.h says of gT).  The start and end values live
 * in Df: they are not variables and nothing is written for them.
 *
 * Per segment (T = T_s) and axis k write d = (p0, v0, a0, pT, vT, aT) for the waypoint
 * values at its ends.  The coefficients are linear in d: c0 = p0, c1 = v0, c2 = a0 / 2,
 *            d/dp0      d/dv0     d/da0       d/dpT      d/dvT     d/daT
 *     c3   -10/T^3    -6/T^2    -3/(2T)      10/T^3    -4/T^2     1/(2T)
 *     c4    15/T^4     8/T^3     3/(2T^2)   -15/T^4     7/T^3    -1/T^2
 *     c5    -6/T^5    -3/T^4    -1/(2T^3)     6/T^5    -3/T^4     1/(2T^3)
 * so that h_j(t) = d p(t) / d d_j, h_j' = d v / d d_j and h_j'' = d a / d d_j are
 * fixed polynomials in t.  A live sample i (time t = t_i, weight dt; gtop_time.h's vn,
 * cd, gd, grad, cv_k, ca_k, S) adds to d cost / d d_{k,j}
 *     collision    wc ( gd grad_k vn dt h_j + cd (v_k / vn) dt h_j' )
 *     dyn (enable_dyn at step 2)
 *                  ( cv_k / r_v sgn(v_k) h_j' + ca_k / r_a sgn(a_k) h_j'' ) vn dt
 *                  + S (v_k / vn) dt h_j'
 * the consistent gradient's terms of gtop.h (gtop_set_gradient_mode) in waypoint form.
 * Per sample the three weights of axis k are formed once,
 *     Wp = wc gd vn dt grad_k
 *     Wv = wc cd dt (v_k / vn)  [+ cv_k / r_v sgn(v_k) vn dt + S (v_k / vn) dt]
 *     Wa =                      [  ca_k / r_a sgn(a_k) vn dt ]          ([..]: dyn)
 * (0 for a sample that is not live), and the sample's share of entry j of axis k is
 * Wp h_j + Wv h_j' + Wa h_j'', with h_j = (dc3/dd_j t^3 + dc4/dd_j t^4 + dc5/dd_j t^5)
 * + (1, t, t^2 / 2 for p0, v0, a0; nothing for pT, vT, aT) and its two derivatives in
 * t.  The 18 shares (3 axes x 6 entries) are summed over the segment's samples by the
 * half-wavefront butterfly that sums the cost (xor 16, 8, 4, 2, 1 over the 32 lanes of
 * the half: 18 sums per segment, each in that order).  The smoothness term's
 * derivative is ws 2 (q3 dc3/dd_j + q4 dc4/dd_j + q5 dc5/dd_j) with q3 .. q5 as
 * gtop_time.h's jerk term forms them (q_n = row n of Q c), summed left to right; an
 * entry of a segment is
 *     (smoothness term) + (the samples' sum)              in that order.
 * Interior waypoint w gets (end part of segment w - 1) + (start part of segment w), in
 * that order, as one rounded addition.  |wc| < 1e-4 skips the samples (their sum is 0), as the
 * callback does; at step 1 ws counts as 0.  Every gx and gT entry is written exactly
 * once.
 *
 * The optimizer.  Per row, minimise F(x, T) = cost(x, T) + rho sum_s T_s over
 * lb <= x <= ub and lo_s <= T_s <= t_max; lo_s = max(t_min, T_lo[b][s]) (T_lo NULL:
 * t_min), and lo_s > t_max pins the segment at lo_s — gtop_time.h's rule, so the output
 * of gtop_reallocate_times_device(GTOP_RETIME_LIMITS) is a legal d_T_lo.  The variable
 * is z = [x | T] with n_z = 10 m - 9 entries; a pinned segment is lb = ub, which the
 * MMA update returns bit for bit.  The loop is the batched MMA's two-launch form
 * (gtop_optimize_device_ex with fusion 0), on the caller's stream:
 *     pack z0 = [x | T] and the bounds; gtop's MMA initialisation (the start point is
 *     clamped into its box);
 *     max_evals times:  (1) the joint pass at the state's trial point: F and
 *                           g = [gx | gT + rho]; sum_s T_s is taken in a fixed order
 *                           (lane l adds s = l, l + 64, ..., then the wavefront's
 *                           butterfly);
 *                       (2) the MMA update over n_z variables, unmodified;
 *     a closing pass at the best point (its cost is [4], its gradient gives [6], [7]);
 *     the MMA finish (code, evaluations) and the report.
 * A row that has stopped keeps its state; the launches still run over it.  All state
 * lives in d_work (gtop_joint_workspace_bytes: the six n_z-vectors, the packed bounds,
 * the scalars and f | g): nothing is allocated and nothing is synchronised, so the
 * call is capturable.  The codes are gtop_optimize_device_ex's.  info[b] has
 * GTOP_JOINT_INFO = 8 entries:
 *   [0] code (3 FTOL, 4 XTOL, 5 MAXEVAL)   [1] evaluations (the closing pass not counted)
 *   [2] F at the clamped start             [3] F returned (the least F seen)
 *   [4] the cost returned, without the rho term
 *   [5] sum_s T_out
 *   [6] max |g| over the x entries not held at a bound by their gradient (held: lb = ub,
 *       x = lb with g > 0, x = ub with g < 0)            [7] the same over T (g = gT + rho)
 * [4] is, bit for bit, the cost gtop_joint_gradient_device returns at (x_out, T_out).
 * x_out (written over d_x) and T_out lie inside their bounds exactly.  d_T_out may not
 * alias d_T.
 *
 * The moving-obstacle cost.  As in gtop_time.h: while gtop_set_moving_cost is switched
 * on every entry point of this header returns GTOP_ERR_STATE and launches nothing
 * (alternate gtop_optimize_device_ex and gtop_time_moving.h's optimizer there).
 *
 * The kernel (csrc/gtop_joint.hip over csrc/gtop_time_pass.h): one wavefront per
 * trajectory, gtop_time.h's lane map; a row's bits depend on its own inputs only: not
 * on B, on the row's place or on time_stride.  A NaN input or a zero segment time
 * gives garbage in that row only; every loop is bounded.  Nothing per sample is written
 * to HBM.  The gradient's device form enqueues one launch.  The host forms serve the
 * first B rows of the context's problem (1 <= B <= the problem's batch; GTOP_ERR_STATE
 * when none is set) with the problem's own segment times as T.
 * GTOP_ERR_STATE, nothing launched: no parameters, no field, the moving-obstacle cost
 * switched on; in the optimizer fp32 optimizer precision
 * (gtop_set_optimizer_precision).  GTOP_ERR_INVALID, nothing launched: B < 0, m outside
 * 2 .. 227, a time_stride that is neither 0 nor m, a NULL required buffer with B > 0; in
 * the optimizer opt NULL, reserved != 0, rho not finite or < 0, t_min < 0.0301,
 * t_min > t_max, a bound of opt that is not finite, ftol_rel or xtol_rel < 0 or NaN,
 * max_evals < 1, d_T_out == d_T, work_bytes below gtop_joint_workspace_bytes(B, m).
 * gtop_joint_workspace_bytes refuses bytes NULL, B < 0 and m outside 2 .. 227.  B = 0
 * launches nothing.  fp64 only.  The gtop_group_* entry points do not forward these
 * calls.
 */
#ifndef GTOP_JOINT_H_
#define GTOP_JOINT_H_

#include <stddef.h>

#include "gtop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double rho;                /* >= 0: weight of sum_s T_s */
  double t_min, t_max;       /* 0.0301 <= t_min <= t_max, finite */
  double ftol_rel, xtol_rel; /* >= 0: the MMA loop's stop rules, per row */
  int32_t max_evals;         /* >= 1 */
  int32_t reserved;          /* must be 0 */
} gtop_jointopt;
#define GTOP_JOINT_ABI_VERSION 1
#define GTOP_JOINT_INFO 8

/* GTOP_JOINT_ABI_VERSION of the library. */
int gtop_joint_abi_version(void);
int gtop_joint_gradient_device(gtop_ctx *ctx, int B, int m, const void *d_x, const void *d_Df, const void *d_T,
                               int time_stride, void *d_cost /* B */, void *d_gx /* B x 9(m-1) */,
                               void *d_gT /* B x m */, void *d_parts /* may be NULL: B x m x GTOP_TIME_PARTS */,
                               void *hip_stream);
int gtop_joint_gradient_batch(gtop_ctx *ctx, int B, const double *x, double *cost, double *gx, double *gT,
                              double *parts /* may be NULL */);
int gtop_joint_workspace_bytes(int B, int m, size_t *bytes);
int gtop_optimize_joint_device(gtop_ctx *ctx, const gtop_jointopt *opt, int B, int m, void *d_x /* in, out */,
                               const void *d_Df, const void *d_T, int time_stride,
                               const void *d_lb, const void *d_ub /* B x 9(m-1), as gtop_optimize_device_ex */,
                               const void *d_T_lo /* may be NULL: B x m */, void *d_T_out /* B x m, may not alias d_T */,
                               void *d_info /* B x GTOP_JOINT_INFO */, void *d_work, size_t work_bytes,
                               void *hip_stream);
int gtop_optimize_joint(gtop_ctx *ctx, const gtop_jointopt *opt, int B, double *x /* in, out */, const double *lb,
                        const double *ub, const double *T_lo /* may be NULL */, double *T_out, double *info);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_JOINT_H_ */
