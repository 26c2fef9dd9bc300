/*
 * gtop_prediction.h — moving-obstacle predictions FITTED from observation histories:
 * the reference's ObjPredictor (src/obj_predictor.cpp: predictPolyFit, a regularised
 * least-squares quintic through an object's recent (x, y, z, t) history, and
 * predictConstVel, a line through the last two observations) as a batched device
 * kernel, an in-place refresh of the context's polynomial box list, and a host form
 * with the same bits.  A companion of gtop.h, exported from the same libgtop_hip.so.
 *
 * Why a header of its own.  gtop.h is a frozen surface (see gtop_kinematics.h).  What
 * is declared here is versioned on its own (gtop_pred_abi_version,
 * GTOP_PRED_ABI_VERSION) and adds nothing to gtop.h.  A library that lacks
 * gtop_pred_abi_version does not have this header's entry points.  gtop.h is included
 * for gtop_ctx and the status codes.
 *
 * What is fitted.  Per axis, predictPolyFit minimises
 *     J(c) = sum_i (p(t_i) - q_i)^2 + lambda int_{t1}^{t2} p''(t)^2 dt,
 * p(t) = sum_{j=0..5} c_j t^j, t1 and t2 the first and last history times; its 6 x 6
 * system (lines 96-133) is the normal equations of J times 2, built in absolute time
 * with powers up to t^10.  The same minimiser is computed here in the shifted and
 * scaled time s = (t - t_last) / sigma, sigma = t_last - t_first, and converted to the
 * row's absolute-time monomials only at the end.
 *
 * The inputs.  hist is N x H x 4 fp64: x, y, z, t per slot (the device buffer must be
 * 16-byte aligned).  count is N int32, each in 0 .. H.  head (N int32, NULL: all 0)
 * makes each history a ring: sample i of object n is slot (head[n] + i) mod H (the
 * non-negative remainder), oldest first — the reference's push_back / pop_front deque
 * as a device buffer.
 *
 * The options (gtop_predict_opts):
 *   mode      GTOP_PREDICT_POLYFIT or GTOP_PREDICT_CONST_VEL
 *   degree    1 .. 5 (predictPolyFit: 5)
 *   lambda    >= 0, finite (prediction/lambda: 1.0)
 *   horizon   >= 0, +inf allowed.  The row is valid on [t_first, t_last + horizon];
 *             0 is the reference's setTime(t1, t2).  The library's consumers hold a
 *             box still outside its interval: without a horizon a fitted box stands at
 *             its last observation, so this option is what makes the fit a prediction.
 *   regularise_horizon  0 or 1.  1 takes the integral to t_last + horizon, which keeps
 *             an extrapolated quintic tame; refused together with an infinite horizon.
 *   inflate   >= 0, finite: gtop_refresh_box_predictions_device grows a box by this
 *             many times the fit's own miss (below).
 *   reserved  must be 0.
 *
 * The arithmetic.  Every step below is ONE rounded fp64 operation in the order
 * written; nothing is fused except where fma is named; sqrt and division are
 * correctly rounded.  tests/predict_twin.py restates it and reproduces the bits.
 *   checks    Samples in order i = 0 .. count-1; t_first is the time of sample 0,
 *             t_last that of sample count-1.  A count outside 0 .. H is clamped into
 *             it and the object is BAD.  count == 0: EMPTY.  A non-finite entry among
 *             the count samples: BAD.  count >= 2 and not (t_last - t_first > 0): BAD.
 *             On EMPTY or BAD only the info row is written (status, count, zeros): the
 *             object's coef, t_range, local and context row are left untouched and the
 *             prediction in force stays — a vanished box would make the unknown look
 *             safe.
 *   count == 1, either mode: the constant q on [t, t + horizon], degree 0, LOWERED;
 *             local: g_0 = q, sigma = 0.
 *   CONST_VEL, count >= 2: the last two samples (q1, t1), (q2, t2); not (t1 < t2):
 *             BAD.  sigma = t2 - t1, d = q2 - q1, c1 = d / sigma, c0 = q2 - c1 t2, the
 *             rest 0; the interval is [t1, t2 + horizon]; degree 1; local: g_0 = q2,
 *             g_1 = d.
 *   POLYFIT   deg = min(degree, count - 1), LOWERED if that is below degree.
 *             sigma = t_last - t_first, s_i = (t_i - t_last) / sigma,
 *             e = regularise_horizon ? horizon / sigma : 0,
 *             lam_e = lambda / ((sigma sigma) sigma).
 *             Per sample the powers s^0 = 1, s^j = s^(j-1) s up to s^10, and the
 *             products s^j q_k, j = 0 .. 5.
 *     sums    29 of them: S_p = sum_i s_i^p (p = 0 .. 10), M_jk = sum_i s_i^j q_ik.
 *             Samples are taken in chunks of 64, sample i in chunk i / 64 at place
 *             i mod 64; missing places contribute +0.0.  A chunk is reduced by the
 *             balanced pair tree — places 2k and 2k+1, then pairs of pairs, six
 *             levels (addition commutes, so any exchange that forms these pairs gives
 *             these bits) — and the chunk sums are added in chunk order, from +0.0.
 *     system  A_jk = S_{j+k} + [j, k >= 2] (lam_e w_jk) (e^p - (-1)^p), p = j + k - 3,
 *             w_jk = (double)(j (j-1) k (k-1)) / (double)p, e^p by repeated product;
 *             b_jk = M_jk.  This is the reference's system in s, halved.
 *     factor  Cholesky of the leading (deg+1)^2 block, row by row: for k = 0 .. j,
 *             acc = A_jk, then acc = acc - L_jp L_kp for p = 0 .. k-1 in order;
 *             k < j: L_jk = acc / L_kk; k == j: the pivot d = acc, L_jj = sqrt(d).  A
 *             pivot breaks down when not (d > 2^-40 A_jj): deg is lowered by one and
 *             the block factored again (degree 0 always succeeds: A_00 = count);
 *             LOWERED.
 *     solve   per axis, y_j = (b_j - sum_{p<j} L_jp y_p) / L_jj for j = 0 .. deg, then
 *             g_j = (y_j - sum_{p=j+1..deg} L_pj g_p) / L_jj for j = deg .. 0, each sum
 *             subtracted term by term in ascending p; g_j = 0 above deg.  A non-finite
 *             g: BAD.
 *     row     a_j = g_j / sigma^j (sigma^j by repeated product from 1), then the Taylor
 *             shift to absolute time: c = a; for i = 0 .. 5: for j = 4 down to i:
 *             c_j = c_j + c_{j+1} (-t_last) (the product rounded, then the sum).
 *   all       A non-finite c: BAD.  t_range = {start, t_last + horizon}, start =
 *             t_first (CONST_VEL: t1).
 *   residual  r_ik = centre_k(t_i) - q_ik over all count samples, the centre being the
 *             consumers' own expression (gtop.h: Horner in explicit fmas) at the
 *             unclamped t_i, so the figure says what the cost will see.
 *             resmax_k = max_i |r_ik|; rms = sqrt(E / (double)(3 count)), E the sum of
 *             (r_i0 r_i0 + r_i1 r_i1) + r_i2 r_i2 by the chunks and the tree above.
 *
 * The outputs.  coef N x 18 and t_range N x 2 are laid out as
 * gtop_set_moving_box_polynomials takes them.  info is N x GTOP_PRED_INFO:
 *   [0] status: GTOP_PRED_OK, _LOWERED, _EMPTY, _BAD   [1] count (clamped)
 *   [2] the degree used   [3] the interval's start   [4] t_last   [5] the interval's end
 *   [6..8] resmax per axis   [9] rms   [10], [11] 0
 * local (optional) is N x GTOP_PRED_LOCAL: g (18, axis-major), t_last, sigma — the
 * accurate form, p(t) = sum_j g_j ((t - t_last) / sigma)^j.
 *
 * gtop_fit_predictions_device: one launch on the caller's stream
 * (csrc/gtop_prediction.hip, one wavefront per object), no allocation, no
 * synchronisation, capturable.  N = 0 launches nothing.
 *
 * gtop_refresh_box_predictions_device: the same fit written straight into the
 * context's box list, in one launch.  It needs a polynomial list
 * (gtop_set_moving_box_polynomials) of exactly N boxes in force; otherwise
 * GTOP_ERR_STATE and nothing is written.  Every fitted object's coefficients, t1 and
 * t2 go into its row of the context's box buffer and, when N <=
 * GTOP_MOVING_COST_MAX_BOXES, into its row of the buffer the cost bodies read (which
 * never moves).  With d_scale (N x 3, the full extents as the setter takes them; a
 * non-finite or negative entry makes the object BAD) the half extent written is
 * 0.5 scale_k + inflate resmax_k (the product rounded, then the sum): a caller's box
 * grows with the fit's own miss.  With d_scale NULL the extents in force stay and
 * inflate is not used.  Evaluations, optimizer runs, queries, reports and
 * certificates enqueued behind it on that stream see the new rows, and a captured
 * graph of "refresh, then any of those" replays on new histories — on ONE condition:
 * a later setter that grows the list moves the queries' buffer, after which the
 * capture must be made again (as for every captured query today).  The list's kind
 * and count do not change, so no kernel selection changes.
 *
 * gtop_fit_predictions: the host form — no context, no device, like
 * gtop_box_polynomial_centres — with the same bits.  local may be NULL.
 *
 * GTOP_ERR_INVALID, nothing written: opts NULL or outside the ranges above, N < 0,
 * H < 1, a NULL hist, count, coef, t_range or info with N > 0 (the refresh: hist,
 * count, info), a device hist that is not 16-byte aligned.
 *
 * fp64 only.  The gtop_group_* entry points do not forward these calls.
 */
#ifndef GTOP_PREDICTION_H_
#define GTOP_PREDICTION_H_

#include "gtop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t mode;               /* GTOP_PREDICT_POLYFIT or GTOP_PREDICT_CONST_VEL */
  int32_t degree;             /* 1 .. 5 */
  double lambda;              /* >= 0 */
  double horizon;             /* >= 0, +inf allowed: the row is valid on [t_first, t_last + horizon] */
  double inflate;             /* >= 0: the refresh adds inflate * resmax_k to the half extent */
  int32_t regularise_horizon; /* 0, or 1: the integral runs to t_last + horizon (a finite one) */
  int32_t reserved;           /* must be 0 */
} gtop_predict_opts;
#define GTOP_PRED_ABI_VERSION 1
#define GTOP_PREDICT_POLYFIT 0
#define GTOP_PREDICT_CONST_VEL 1
#define GTOP_PRED_INFO 12
#define GTOP_PRED_LOCAL 20
#define GTOP_PRED_OK 0
#define GTOP_PRED_LOWERED 1
#define GTOP_PRED_EMPTY 2
#define GTOP_PRED_BAD 3

/* GTOP_PRED_ABI_VERSION of the library. */
int gtop_pred_abi_version(void);
int gtop_fit_predictions_device(gtop_ctx *ctx, int N, int H, const void *d_hist, const void *d_count,
                                const void *d_head /* may be NULL */, const gtop_predict_opts *opts, void *d_coef,
                                void *d_t_range, void *d_info, void *d_local /* may be NULL */, void *hip_stream);
int gtop_refresh_box_predictions_device(gtop_ctx *ctx, int N, int H, const void *d_hist, const void *d_count,
                                        const void *d_head /* may be NULL */, const gtop_predict_opts *opts,
                                        const void *d_scale /* may be NULL: keep the extents */, void *d_info,
                                        void *hip_stream);
int gtop_fit_predictions(int N, int H, const double *hist, const int32_t *count, const int32_t *head /* may be NULL */,
                         const gtop_predict_opts *opts, double *coef, double *t_range, double *info,
                         double *local /* may be NULL */);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_PREDICTION_H_ */
