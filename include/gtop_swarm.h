/*
 * gtop_swarm.h — PAIRWISE SEPARATION AS A COST: a penalty on rows of a batch that come
 * closer than a radius on the common clock, its gradient with respect to every row's
 * free variables, and a swarm optimizer in sweeps.  A companion of gtop.h, exported
 * from the same libgtop_hip.so.
 *
 * Why a header of its own.  gtop.h is a frozen surface (see gtop_kinematics.h).  What
 * is declared here is versioned on its own (gtop_swarm_abi_version,
 * GTOP_SWARM_ABI_VERSION) and adds nothing to gtop.h.  A library that lacks
 * gtop_swarm_abi_version does not have this header's entry points.  gtop.h is included
 * for gtop_ctx and the status codes; gtop_separation.h for the limits.
 *
 * What it is for.  gtop_separation_device reports the mutual clearance of the robots
 * of a swarm and gtop_certify_separation_device certifies it; neither changes a plan.
 * This header is the term that does: every robot optimises its own trajectory against
 * the current plans of the others, in sweeps (the decentralised formulation).
 *
 * THE ARITHMETIC.  Every step below is ONE rounded fp64 operation in the order written,
 * nothing fused (csrc/gtop_swarm.hip is compiled with contraction off): a restatement
 * in numpy reproduces the bits (tests/swarm_twin.py), and the same lines in rational
 * arithmetic are exact.
 *
 * Grid, start times, flown samples, positions: exactly those of gtop_separation.h —
 * tau_k = t_lo + (double)k dt, start_b, time_sum_b, hold_ends, the segment walk, the
 * value of the segment's polynomial.  The two files share one sample kernel, so the
 * positions are bit for bit the ones pair_min is taken over.  u_k and s_k below are the
 * local time and the segment the walk ends with.
 *
 * The penalty.  R2 = R R, R = radius.  For rows i != j both flown at k:
 *     dx = x_i - x_j  (dy, dz likewise)     d2 = ((dx dx + dy dy) + dz dz)
 *     e  = R2 - d2        ACTIVE iff e > 0  (a NaN is not active)
 *     e2 = e e            e3 = e2 e
 * An active term adds e3 to C_ik and e2 dx, e2 dy, e2 dz to Fx_ik, Fy_ik, Fz_ik (the
 * product rounded, then the sum).  Each of the four sums starts at +0 and runs over
 * the partners j ascending; inactive terms are skipped.  (A kernel that adds +0 for
 * them produces the same bits: a sum that starts at +0 is never -0, and x + 0 = x.)
 * The cubic hinge in the SQUARED distance: twice continuously differentiable at the
 * radius and exactly zero beyond it, so culls are exact; no singularity where two rows
 * touch; no sqrt and no exp.
 *
 * Per row.   S_b = (w dt) (sum_k C_bk), k ascending from +0 over the grid (a sample at
 * which the row is not flown has C = +0); active_b = the number of active (j, k) terms.
 * The swarm's total is 1/2 sum_b S_b; because the penalty is symmetric,
 * d total / d x_b = d S_b / d x_b with the other rows held fixed.  That is the gradient
 * returned, and d e3 / d x_i = -6 e2 dx.
 *
 * The chain to the free variables.  A position in segment s at local time u is
 * sum_n c_n u^n with c = A^-1(T_s) (p0, v0, a0, pT, vT, aT).  Per segment s and axis,
 * with the powers as the polynomial's value forms them (u2 = u u, u3 = u2 u,
 * u4 = u2 u2, u5 = u4 u):
 *     G_0 = sum_k F_k          G_n = sum_k (F_k u_k^n), n = 1 .. 5
 * over the flown samples k of the row with s_k = s, k ascending, from +0.  With T = T_s,
 * T2 = T T, T3 = T2 T, T4 = T2 T2, T5 = T4 T, every coefficient below ONE division of
 * the constant by the power, every product rounded, the sums from left to right:
 *     h_p0 = (((G_0 + (-10 / T3) G_3) + (15 / T4) G_4) + (-6 / T5) G_5)
 *     h_v0 = (((G_1 + (-6 / T2) G_3) + (8 / T3) G_4) + (-3 / T4) G_5)
 *     h_a0 = (((0.5 G_2 + (-1.5 / T) G_3) + (1.5 / T2) G_4) + (-0.5 / T3) G_5)
 *     h_pT = (((10 / T3) G_3 + (-15 / T4) G_4) + (6 / T5) G_5)
 *     h_vT = (((-4 / T2) G_3 + (7 / T3) G_4) + (-3 / T4) G_5)
 *     h_aT = (((0.5 / T) G_3 + (-1 / T2) G_4) + (0.5 / T3) G_5)
 * (d c / d q in closed form: P, V, A, N3 .. N5 of gtop_time.h differentiated.)  With
 * K = ((-6 w) dt), interior waypoint j = 1 .. m-1, q in {p, v, a} = {0, 1, 2}:
 *     grad[3 (j-1) + q + axis (3m-3)] = (K h_qT of segment j-1) + (K h_q0 of segment j)
 * — the layout of x.  The Df ends are not free and get nothing.
 *
 * gtop_swarm_gradient_device.  coeff is B x m x 18, T is B x m (time_stride m) or m
 * shared values (time_stride 0), as for gtop_separation_device.  With d_coeff_frozen
 * NULL the partners of a row are the other rows of the batch.  With d_coeff_frozen
 * given, row i's partners are the FROZEN rows j != i — the same B, m, T and start
 * times at another x; row i's own frozen copy is skipped.  This is the function a
 * sweep of the optimizer minimises.  Outputs: S [B], grad [B][9 (m-1)], active [B]
 * doubles (may be NULL).  It only enqueues launches on the caller's stream
 * (csrc/gtop_swarm.hip: sample, pairs, rows): no allocation, no synchronisation,
 * capturable.  No field is read, so none is required.  A row's figures depend on
 * neither B nor the row's place, and the results are deterministic.  Non-finite inputs
 * give unspecified figures in the rows they touch; every loop is bounded and the call
 * stays memory-safe.  gtop_swarm_gradient_batch serves the first B rows of the
 * context's problem at free variables x (and x_frozen), staged as
 * gtop_separation_batch stages.
 *
 * gtop_swarm_workspace_bytes is pure (no context): the bytes d_work needs for B rows
 * of m segments on n_samples samples (0 for B = 0); GTOP_ERR_INVALID for a NULL
 * `bytes`, B outside 0 .. GTOP_SEP_MAX_B, m outside 2 .. 227, n_samples outside
 * 1 .. GTOP_SEP_MAX_SAMPLES.  The layout is private.
 *
 * GTOP_ERR_INVALID, nothing launched: opt NULL, w not finite or < 0, radius not finite
 * or <= 0, a non-finite t_lo or dt, dt <= 0, n_samples outside
 * 1 .. GTOP_SEP_MAX_SAMPLES, hold_ends neither 0 nor 1, a reserved word not 0, B < 0
 * or B > GTOP_SEP_MAX_B, m outside 2 .. 227, a time_stride that is neither 0 nor m, a
 * NULL required buffer with B > 0, work_bytes below gtop_swarm_workspace_bytes, a
 * start-time count that is not 0, 1 or B.  B = 0 launches nothing.
 *
 * gtop_optimize_swarm_device runs stop->sweeps sweeps.  In a sweep (1) every row's
 * trajectory at the sweep's start is sampled into the frozen side of the workspace;
 * (2) the batched MMA loop of gtop_optimize_device_ex runs stop->evals_per_sweep rounds
 * in its two-launch form from freshly initialised state, each round: the context's own
 * evaluation at the trial points, their coefficients, sample, the pair launch of trial
 * rows against frozen rows, the row launch that ADDS S_b to the row's cost and
 * d S_b / d x_b to its gradient, the MMA update; (3) every row's best point becomes
 * its x.  Per row a sweep is gtop_optimize_device_ex with an evaluation count as its
 * only stop rule on f_b(x_b) = cost_b(x_b) + S_b(x_b; frozen others) — a fixed
 * function within the sweep, so the best-so-far is meaningful.  min_cost[b] is the
 * last sweep's least f_b.  d_joint (may be NULL: B x 2) gets one closing joint
 * evaluation at the returned x: [0] the context's own cost of the row
 * (gtop_eval_device), [1] S_b with the others unfrozen (gtop_swarm_gradient_device).
 * The two-launch form is taken whatever gtop_set_optimizer_fusion says.  With w == 0
 * no sample, pair or row launch is enqueued (d_joint[1] is +0).  GTOP_ERR_STATE,
 * nothing launched: no parameters, no field, gtop_set_optimizer_precision(GTOP_F32),
 * the moving-obstacle cost switched on.  GTOP_ERR_INVALID also: stop NULL, sweeps or
 * evals_per_sweep < 1, a reserved word not 0, m above 118.  The call does not
 * synchronise the host; the context's optimizer state grows on a first call, as for
 * gtop_optimize_device_ex, and the call is capturable after that.  gtop_optimize_swarm
 * serves the first B rows of the context's problem from host buffers.
 *
 * fp64 only.  The gtop_group_* entry points do not forward these calls.
 */
#ifndef GTOP_SWARM_H_
#define GTOP_SWARM_H_

#include "gtop.h"
#include "gtop_separation.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double t_lo, dt;      /* the common grid, as gtop_sep_opts */
  double w, radius;     /* w >= 0 finite; radius > 0 finite */
  int32_t n_samples;    /* 1 .. GTOP_SEP_MAX_SAMPLES */
  int32_t hold_ends;    /* 0 / 1, as gtop_sep_opts */
  int32_t reserved[2];  /* must be 0 */
} gtop_swarm_opts;
typedef struct {
  int32_t sweeps, evals_per_sweep; /* each >= 1 */
  int32_t reserved[2];             /* must be 0 */
} gtop_swarm_stop;
#define GTOP_SWARM_ABI_VERSION 1

/* GTOP_SWARM_ABI_VERSION of the library. */
int gtop_swarm_abi_version(void);
int gtop_swarm_workspace_bytes(int B, int m, int n_samples, size_t *bytes);
int gtop_swarm_gradient_device(gtop_ctx *ctx, const gtop_swarm_opts *opt, int B, int m, const void *d_coeff,
                               const void *d_coeff_frozen /* may be NULL */, const void *d_T, int time_stride,
                               void *d_S /* B */, void *d_grad /* B x 9(m-1) */,
                               void *d_active /* may be NULL: B doubles */, void *d_work, size_t work_bytes,
                               void *hip_stream);
int gtop_swarm_gradient_batch(gtop_ctx *ctx, const gtop_swarm_opts *opt, int B, const double *x,
                              const double *x_frozen /* may be NULL */, double *S, double *grad,
                              double *active /* may be NULL */);
int gtop_optimize_swarm_device(gtop_ctx *ctx, const gtop_swarm_opts *opt, const gtop_swarm_stop *stop, int B, int m,
                               void *d_x /* in: start, out: result */, const void *d_Df, const void *d_T,
                               int time_stride, const void *d_lb, const void *d_ub, void *d_min_cost /* B */,
                               void *d_joint /* may be NULL: B x 2 */, void *d_work, size_t work_bytes,
                               void *hip_stream);
int gtop_optimize_swarm(gtop_ctx *ctx, const gtop_swarm_opts *opt, const gtop_swarm_stop *stop, int B, double *x,
                        const double *lb, const double *ub, double *min_cost, double *joint /* may be NULL */);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_SWARM_H_ */
