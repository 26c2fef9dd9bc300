/*
 * gtop_kinematics.h — the continuous-time KINEMATIC certificate: velocity and
 * acceleration limits certified over whole time intervals.  A companion of gtop.h,
 * exported from the same libgtop_hip.so.
 *
 * Why a header of its own.  gtop.h is a frozen surface: its declarations, its
 * GTOP_ABI_VERSION and the legal values of its option structs are pinned by the
 * suite, so that a caller compiled against ABI 12 finds exactly ABI 12.  What is
 * declared here is versioned on its own (gtop_kin_abi_version, GTOP_KIN_ABI_VERSION)
 * and adds nothing to gtop.h: no declaration, no new legal value of an existing
 * option struct, no change of gtop_abi_version().  A library that lacks
 * gtop_kin_abi_version does not have this header's entry points.  gtop.h is included
 * for gtop_ctx, gtop_limits, the status codes and GTOP_CERT_REQUIRE_*.
 *
 * What is certified.  Every velocity and acceleration figure of gtop.h (entries
 * 7 .. 10 of the trajectory report, 6 .. 9 of the per-segment report) is a maximum
 * over the getTraj samples; gtop_select_best[_certified]_device apply max_vel /
 * max_acc to those, and gtop_reallocate_times_device(GTOP_RETIME_LIMITS) stretches by
 * them.  Between two samples they say nothing.  This certificate gives, per
 * trajectory and per segment, the maximum over [0, time_sum] of
 *     ‖v‖, ‖a‖, max_k |v_k|, max_k |a_k|
 * as a CERTIFIED UPPER bound (ub) and an ATTAINED LOWER bound (lo: a value the curve
 * takes at an evaluated time), and a verdict against max_vel / max_acc.
 *
 * The interval tree is gtop_certify_trajectories_device's (gtop.h).  An interval is
 * [a, a + w] in a segment's local time.  Level 0 cuts a segment of time Ts into 64
 * intervals, w = 0.015625 Ts, a = j w, j = 0 .. 63; refining an interval replaces it
 * by its 64 children, w' = 0.015625 w, a' = a + j w'.  An OPEN interval is refined
 * while its level is below max_depth (0 .. GTOP_CERT_MAX_DEPTH) and fewer than
 * max_refine refinements have been spent on the trajectory; after that it is an
 * undecided leaf.  Segments in order, within a segment depth-first in ascending
 * time; level 0 of every segment is always evaluated.  The trajectory time of a
 * segment's start, t_off, is the segment times summed left to right.
 *
 * The arithmetic.  Every step below is ONE rounded fp64 operation in the order
 * written (a product of three factors is taken left to right), nothing fused.
 * Per segment (time Ts, T2 = Ts Ts) and axis k, with c_j the axis' coefficients in
 * ascending powers and q_j = |c_j|:
 *     J  = 6 q3 + 24 q4 Ts + 60 q5 T2                        bounds |jerk| on [0, Ts]
 *     S  = 24 q4 + 120 q5 Ts                                 bounds |snap|
 *     Vk = (((5 q5 Ts + 4 q4) Ts + 3 q3) Ts + 2 q2) Ts + q1  what v's rounding scales with
 *     Ak = ((20 q5 Ts + 12 q4) Ts + 6 q3) Ts + 2 q2          what a's rounding scales with
 * Per interval: h = 0.5 w, tc = a + h, t = t_off + tc, and per axis, the integer
 * factor applied to the coefficient first:
 *     v  = ((((5 c5) tc + 4 c4) tc + 3 c3) tc + 2 c2) tc + c1
 *     ac = (((20 c5) tc + 12 c4) tc + 6 c3) tc + 2 c2
 *     j  = ((60 c5) tc + 24 c4) tc + 6 c3
 *     rv = (|ac| h + 0.5 J h h) (1 + 2^-40) + 2^-40 Vk
 *     ra = (|j|  h + 0.5 S h h) (1 + 2^-40) + 2^-40 Ak
 *     Uv_k = |v| + rv          Ua_k = |ac| + ra
 * Midpoint figures: mvn = sqrt(v0 v0 + v1 v1 + v2 v2) (summed left to right), mvx =
 * max_k |v_k|; man, max likewise from ac.  Upper bounds: uvn = sqrt(Uv0 Uv0 + Uv1
 * Uv1 + Uv2 Uv2) (1 + 2^-40), uvx = max_k Uv_k; uan, uax likewise.  A maximum
 * ignores a NaN operand; where a norm's upper bound is NaN it and its per-axis
 * companion become +inf: a NaN certifies nothing.
 * By Taylor's theorem about tc, |v_k(t) - v_k(tc)| <= |ac| |t - tc| + J (t - tc)^2 / 2
 * with |t - tc| <= h, likewise for ac with j and S; the 2^-40 terms are over a
 * hundred times the rounding of the interval ends and of the Horner sums
 * (DESIGN.md 5.17).  So Uv_k >= |v_k| and uvn >= ‖v‖ on the whole interval.
 *
 * Status.  Fv / Fa are the norm figures (mvn, uvn / man, uan), or under per_axis the
 * per-axis ones (mvx, uvx / max, uax).  A limit <= 0 (or NaN) is off: it makes no
 * interval OPEN or a VIOLATION.
 *     VIOLATION  if an active limit has F_mid > limit (the report passes figure <=
 *                limit).  A VIOLATION is never refined.
 *     CERTIFIED  else if every active limit has F_ub <= limit.
 *     OPEN       else.
 * With both limits off every level-0 interval is CERTIFIED: the bounds are level 0's.
 *
 * lo_* is the largest midpoint figure over every evaluated midpoint of every level,
 * ub_* the largest upper bound over the LEAVES (certified, violating and undecided
 * ones), for all four figures, per segment; the trajectory's are the maxima over its
 * segments.  For the chosen figures the trajectory keeps the earliest trajectory time
 * that attains lo (value descending, then time ascending).
 *
 * kin is B x GTOP_KIN_REPORT doubles per trajectory; entries 1, 2, 4, 5 are the
 * chosen figure (the norm, or the per-axis one under per_axis):
 *   [0] verdict: -1 EXCEEDS (an evaluated midpoint broke an active limit), +1 WITHIN
 *       (no violation and no undecided leaf), 0 UNDECIDED
 *   [1] ub_v   [2] lo_v   [3] the time of the earliest midpoint attaining lo_v
 *   [4] ub_a   [5] lo_a   [6] its time
 *   [7] the time of the earliest violating midpoint, -1 if none
 *   [8] undecided leaves   [9] refinements done   [10] time_sum
 * seg (may be NULL) is B x m x GTOP_KIN_SEG doubles:
 *   [0] the segment's verdict by the same rule (a violating midpoint in it; else no
 *       undecided leaf in it)       [1] the refinements spent in it
 *   [2] lo ‖v‖  [3] lo ‖a‖  [4] lo max|v_k|  [5] lo max|a_k|
 *   [6] ub ‖v‖  [7] ub ‖a‖  [8] ub max|v_k|  [9] ub max|a_k|
 * GTOP_KIN_SEG == GTOP_SEG_REPORT, and columns 6 .. 9 sit where
 * gtop_reallocate_times_device(GTOP_RETIME_LIMITS) reads the per-segment report's
 * figures: a seg buffer is legal d_seg_report input to it, with or without per_axis
 * — the segments are then stretched by certified figures instead of sampled ones.
 * WITHIN implies ub <= limit for every active limit.  Every entry is written exactly
 * once.  A row's bits depend on its own inputs only: not on B, on the row's place or
 * on time_stride.  A NaN coefficient or a zero segment time gives garbage or +inf in
 * that row only; every loop is bounded.  One wavefront per trajectory
 * (csrc/gtop_kinematics.hip), nothing per interval goes to HBM.  The kernel reads no
 * field, no parameters and no boxes.
 *
 * gtop_certify_kinematics_device only enqueues one launch: no allocation, no
 * synchronisation, capturable.  gtop_certify_kinematics_batch serves the first B rows
 * of the context's problem at free variables x (1 <= B <= the problem's batch;
 * GTOP_ERR_STATE when none is set), staged as gtop_certify_batch stages.
 * gtop_select_best_kin_certified_device is gtop_select_best_certified_device's rule
 * (d_cert NULL: gtop_select_best_device's) plus the same `require` on kin[b][0]:
 * GTOP_CERT_REQUIRE_SAFE verdict == +1, GTOP_CERT_REQUIRE_NOT_UNSAFE verdict != -1 —
 * the same two launches, workspace and ordering rule.
 * GTOP_ERR_INVALID, nothing launched: opt NULL, reserved != 0, max_depth outside
 * 0 .. GTOP_CERT_MAX_DEPTH, max_refine < 0, an infinite limit, B < 0, m outside
 * 2 .. 227, a time_stride that is neither 0 nor m, NULL coeff / T / kin with B > 0;
 * in the selection NULL d_kin (report, cost) with B > 0, NULL best, a `require` that
 * is neither value, the limits rules of gtop_select_best_device.  B = 0 launches
 * nothing (the selection writes best = {-1, 0}).  fp64 only.  The gtop_group_* entry
 * points do not forward these calls.
 */
#ifndef GTOP_KINEMATICS_H_
#define GTOP_KINEMATICS_H_

#include "gtop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double max_vel, max_acc; /* <= 0 or NaN: that limit is off */
  int32_t per_axis;        /* 0: the limits apply to the norms; else to the largest |component| */
  int32_t max_depth;       /* 0 .. GTOP_CERT_MAX_DEPTH: levels of refinement below the 64 intervals of a segment */
  int32_t max_refine;      /* >= 0: refinements per trajectory */
  int32_t reserved;        /* must be 0 */
} gtop_kin_opts;
#define GTOP_KIN_ABI_VERSION 1
#define GTOP_KIN_REPORT 11
#define GTOP_KIN_SEG 10

/* GTOP_KIN_ABI_VERSION of the library. */
int gtop_kin_abi_version(void);
int gtop_certify_kinematics_device(gtop_ctx *ctx, int B, int m, const void *d_coeff, const void *d_T,
                                   int time_stride, const gtop_kin_opts *opt, void *d_kin,
                                   void *d_seg /* may be NULL */, void *hip_stream);
int gtop_certify_kinematics_batch(gtop_ctx *ctx, int B, const double *x, const gtop_kin_opts *opt,
                                  double *kin, double *seg /* may be NULL */);
int gtop_select_best_kin_certified_device(gtop_ctx *ctx, int B, const void *d_report,
                                          const void *d_cert /* may be NULL */, const void *d_kin,
                                          const void *d_cost, const gtop_limits *limits, int require,
                                          void *d_pass, void *d_best, void *hip_stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_KINEMATICS_H_ */
