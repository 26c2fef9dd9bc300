/*
 * gtop_time.h — the SEGMENT TIMES as variables: the derivative of the cost with respect
 * to every segment time, and a device optimizer of the time allocation.  A companion of
 * gtop.h, exported from the same libgtop_hip.so.
 *
 * Why a header of its own.  gtop.h is a frozen surface (see gtop_kinematics.h).  What
 * is declared here is versioned on its own (gtop_time_abi_version,
 * GTOP_TIME_ABI_VERSION) and adds nothing to gtop.h.  A library that lacks
 * gtop_time_abi_version does not have this header's entry points.  gtop.h is included
 * for gtop_ctx and the status codes.
 *
 * What is differentiated.  Everything gtop.h optimises is a function of the free
 * waypoint derivatives x at FIXED segment times T.  With the waypoint positions,
 * velocities and accelerations held in x and Df, segment s depends on T_s alone: its
 * coefficients are c_s = A_s^-1(T_s) d_s, its jerk integral is closed-form in T_s and
 * its collision samples sit at 1e-3 + i T_s / 30.  So d cost / d T_s needs segment s
 * only.  The cost is the one gtop_eval_device returns in fp64 for the context's
 * gtop_params, `step` and the enable_dyn block included, under the conventions of
 * GTOP_GRADIENT_CONSISTENT: the float round trips are taken as the identity, the field
 * as differentiable inside a cell, out of the map dist = -1 and the field gradient 0,
 * d vn / d v = v / vn, sgn(+-0) = 0.  There is one derivative: the result does not
 * depend on gtop_set_gradient_mode, and a signed field is read as it is.
 *
 * Per segment (T = T_s; p0, v0, a0 and pT, vT, aT the waypoint values at its ends,
 * per axis):
 *     P = pT - p0 - v0 T - a0 T^2 / 2     V = (vT - v0 - a0 T) T     A = (aT - a0) T^2
 *     P' = -v0 - a0 T                     V' = vT - v0 - 2 a0 T      A' = 2 (aT - a0) T
 *     N3 = 10 P - 4 V + A / 2     c3 = N3 / T^3     c3' = N3' / T^3 - 3 c3 / T
 *     N4 = 7 V - 15 P - A         c4 = N4 / T^4     c4' = N4' / T^4 - 4 c4 / T
 *     N5 = 6 P - 3 V + A / 2      c5 = N5 / T^5     c5' = N5' / T^5 - 5 c5 / T
 * and c0 = p0, c1 = v0, c2 = a0 / 2 do not move.  The jerk term of the segment is
 *     J = sum_k 36 T c3^2 + 144 T^2 c3 c4 + 240 T^3 c3 c5 + 192 T^3 c4^2
 *               + 720 T^4 c4 c5 + 720 T^5 c5^2
 * and its derivative the explicit part (the powers of T differentiated) plus
 * sum_i dJ/dc_i c_i'.  The weight is ws, 0 at step 1.
 * The samples are the evaluation's own: i = 0 .. 29 at t_i = 1e-3 + i dt, dt = T / 30;
 * a segment with T < 0.0301 replays the reference's addition chain (t starts at 1e-3,
 * dt = T / 30 is added i times, the sample counts while t < T).  The count is held
 * fixed and d t_i / d T = i / 30.  With p, v, a, j the position, velocity, acceleration
 * and jerk of the segment at t_i (p, v and a rounded to float as the callback rounds
 * them; the cell is found in double from the rounded position):
 *     p' = sum_j c_j' t^j + v i/30      v' = sum_j j c_j' t^(j-1) + a i/30
 *     a' = sum_j j (j-1) c_j' t^(j-2) + j i/30
 *     vn = |v| + 1e-5      e = exp(-(dist - d0) / r)      cd = alpha e      gd = -(alpha / r) e
 *     collision cost       wc cd vn dt
 *     its derivative       wc ( gd (grad . p') vn dt + cd (v . v' / vn) dt + cd vn / 30 )
 * and under enable_dyn at step 2, with cv_k = alpha_v exp((|v_k| - v0) / r_v), ca_k
 * likewise on a_k, S = sum_k cv_k + ca_k:
 *     cost                 S vn dt
 *     its derivative       ( sum_k cv_k / r_v sgn(v_k) v_k' + ca_k / r_a sgn(a_k) a_k' ) vn dt
 *                          + S (v . v' / vn) dt + S vn / 30.
 * |wc| < 1e-4 skips the samples, as the callback does.
 *
 * Outputs of the gradient.  cost[b] is the callback's cost, its + 1e-3 included.
 * gT[b][s] is the derivative; no + 1e-5 is added (that constant belongs to the
 * callback's gradient vector).  parts[b][s] (may be NULL) has GTOP_TIME_PARTS = 4
 * entries, each weighted as the callback adds it:
 *   [0] the segment's smoothness cost      [1] its collision + dyn cost
 *   [2] d [0] / d T_s                      [3] d [1] / d T_s
 * gT = [2] + [3], and cost = (sum_s [0] + [1], segments in order) + 1e-3.
 *
 * The moving-obstacle cost.  Under absolute sample times T_s moves the lookups of
 * every later segment; that derivative is not formed here.  While
 * gtop_set_moving_cost is switched on every entry point of this header returns
 * GTOP_ERR_STATE and launches nothing.
 *
 * The optimizer.  Per row, minimise F(T) = cost(x, T) + rho sum_s T_s over
 * lo_s <= T_s <= t_max with x fixed; lo_s = max(t_min, T_lo[b][s]) (T_lo NULL:
 * t_min), and lo_s > t_max pins the segment at lo_s.  clamp(T)_s is lo_s for a pinned
 * segment, else min(max(T_s, lo_s), t_max).  An evaluation is one pass of the gradient
 * body: it gives F and g = gT + rho together.
 *     T = clamp(T_in); (F, g) = eval(T); evals = 1
 *     gmax = max_s |g_s|; gmax == 0 (or no finite g): stop, XTOL
 *     a = first_move / gmax
 *     loop:
 *       backtracks = 0
 *       repeat:
 *         T' = clamp(T - a g)
 *         if max_s |T'_s - T_s| <= xtol_abs: stop, XTOL          (T is returned)
 *         if evals == max_evals: stop, MAXEVAL                   (T is returned)
 *         (F', g') = eval(T'); evals += 1
 *         accept if F' <= F + 1e-4 sum_s g_s (T'_s - T_s)        (a NaN F' is a rejection)
 *         else a *= 0.5, backtracks += 1
 *       decrease = F - F'; T, F, g = T', F', g'; accepted += 1
 *       if decrease <= ftol_rel |F|: stop, FTOL
 *       if backtracks == 0: a *= 2
 * The codes are gtop_optimize_device_ex's: 3 FTOL, 4 XTOL, 5 MAXEVAL.  info[b] has
 * GTOP_TIMEOPT_INFO = 8 entries:
 *   [0] code   [1] accepted steps   [2] evaluations   [3] F at the clamped input
 *   [4] F returned   [5] the cost returned, without the rho term
 *   [6] max_s |g_s| over the segments not held at a bound by their gradient (a pinned
 *       segment, T_s == lo_s with g_s > 0 and T_s == t_max with g_s < 0 are held)
 *   [7] sum_s T_out
 * T_out lies inside its bounds exactly; F never rises; [5] is, bit for bit, the cost
 * gtop_time_gradient_device returns at T_out.  The output of
 * gtop_reallocate_times_device(GTOP_RETIME_LIMITS) is a legal d_T_lo — "never faster
 * than the limits allow" — whether it was driven by sampled or by certified figures
 * (gtop_kinematics.h, seg).  d_T_out may not alias d_T.
 *
 * Both kernels (csrc/gtop_time.hip): one wavefront per trajectory; the lanes run over
 * (segment of a pair, sample), the per-segment sums are taken in a fixed order, so a
 * row's bits depend on its own inputs only: not on B, on the row's place or on
 * time_stride.  Every output entry is written exactly once.  A NaN input or a zero
 * segment time gives garbage in that row only; every loop is bounded.  Nothing per
 * sample or per iteration is written to HBM.  The device forms enqueue one launch each:
 * no allocation, no synchronisation, capturable.  The host forms serve the first B rows
 * of the context's problem at free variables x (1 <= B <= the problem's batch;
 * GTOP_ERR_STATE when none is set) with the problem's own segment times.
 * GTOP_ERR_STATE, nothing launched: no parameters, no field, the moving-obstacle cost
 * switched on.  GTOP_ERR_INVALID, nothing launched: B < 0, m outside 2 .. 227, a
 * time_stride that is neither 0 nor m, a NULL required buffer with B > 0; in the
 * optimizer opt NULL, reserved != 0, rho not finite or < 0, t_min < 0.0301,
 * t_min > t_max, a bound that is not finite, first_move not finite or <= 0, ftol_rel
 * or xtol_abs < 0 or NaN, max_evals < 1, d_T_out == d_T.  B = 0 launches nothing.
 * fp64 only.  The gtop_group_* entry points do not forward these calls.
 */
#ifndef GTOP_TIME_H_
#define GTOP_TIME_H_

#include "gtop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double rho;                /* >= 0: weight of sum_s T_s */
  double t_min, t_max;       /* 0.0301 <= t_min <= t_max, finite */
  double first_move;         /* > 0: seconds the first trial moves the segment of largest |g| */
  double ftol_rel, xtol_abs; /* >= 0 */
  int32_t max_evals;         /* >= 1 */
  int32_t reserved;          /* must be 0 */
} gtop_timeopt;
#define GTOP_TIME_ABI_VERSION 1
#define GTOP_TIME_PARTS 4
#define GTOP_TIMEOPT_INFO 8

/* GTOP_TIME_ABI_VERSION of the library. */
int gtop_time_abi_version(void);
int gtop_time_gradient_device(gtop_ctx *ctx, int B, int m, const void *d_x, const void *d_Df, const void *d_T,
                              int time_stride, void *d_cost /* B */, void *d_gT /* B x m */,
                              void *d_parts /* may be NULL: B x m x GTOP_TIME_PARTS */, void *hip_stream);
int gtop_time_gradient_batch(gtop_ctx *ctx, int B, const double *x, double *cost, double *gT,
                             double *parts /* may be NULL */);
int gtop_optimize_times_device(gtop_ctx *ctx, const gtop_timeopt *opt, int B, int m, const void *d_x,
                               const void *d_Df, const void *d_T, int time_stride,
                               const void *d_T_lo /* may be NULL: B x m */, void *d_T_out /* B x m */,
                               void *d_info /* B x GTOP_TIMEOPT_INFO */, void *hip_stream);
int gtop_optimize_times(gtop_ctx *ctx, const gtop_timeopt *opt, int B, const double *x,
                        const double *T_lo /* may be NULL */, double *T_out, double *info);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_TIME_H_ */
