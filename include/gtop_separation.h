/*
 * gtop_separation.h — PAIRWISE figures of a batch of trajectories: for every pair of
 * rows the least and the greatest distance between the two curves on a common time
 * grid, a per-row summary, and the selection of distinct candidates built on it.  A
 * companion of gtop.h, exported from the same libgtop_hip.so.
 *
 * Why a header of its own.  gtop.h is a frozen surface (see gtop_kinematics.h).  What
 * is declared here is versioned on its own (gtop_sep_abi_version,
 * GTOP_SEP_ABI_VERSION) and adds nothing to gtop.h.  A library that lacks
 * gtop_sep_abi_version does not have this header's entry points.  gtop.h is included
 * for gtop_ctx and the status codes.
 *
 * What it is for.  Every other figure of the library speaks of one row alone.  Two
 * uses need two rows together: rows that are the robots of a swarm (the least
 * distance is their mutual clearance on the common clock, with the per-row start
 * times of gtop_set_start_times[_device]), and candidates of one robot, of which a
 * replanning loop wants the cheapest passing ones that are really different curves
 * (the greatest distance: candidates that share start and goal always have least
 * distance 0).
 *
 * The arithmetic.  Every step below is ONE rounded fp64 operation in the order
 * written, nothing fused; min and max are exact, so no figure depends on how the
 * kernels tile the work.
 *   start_b     the row's start time as gtop_set_start_times[_device] left it: 0 when
 *               none is set, the one value when one is set, else one per row (the
 *               count must then be B).  Read when the kernels run: a captured launch
 *               reads what the buffer holds at replay.
 *   time_sum_b  the row's segment times added in order, from 0, as the reports form
 *               their entry 11.
 *   tau_k       t_lo + (double)k * dt, k = 0 .. n_samples-1: the product rounded,
 *               then the sum rounded.
 *   u           tau_k - start_b.  hold_ends == 0: row b is FLOWN at k iff u >= 0 and
 *               u <= time_sum_b.  hold_ends == 1: u is clamped into [0, time_sum_b]
 *               (u < 0 becomes 0, u > time_sum_b becomes time_sum_b) and the row is
 *               flown at every k.  The flown samples of a row are contiguous in k.
 *   position    the segment walk of the reports (while s < m-1 and T_s <= u: u -= T_s,
 *               ++s; the last segment is extended at u == time_sum_b), then per axis
 *               the value of the segment's polynomial as the library's every sample
 *               forms it: t2 = u u, t3 = t2 u, t4 = t2 t2, t5 = t4 u,
 *               ((((((0 + t5 c5) + t4 c4) + t3 c3) + t2 c2) + u c1) + c0).
 *   d2(i,j,k)   both rows flown at k: dx = x_i - x_j (dy, dz likewise),
 *               d2 = ((dx dx + dy dy) + dz dz).  Symmetric in (i, j) to the bit.
 * pair_min[i][j] = sqrt(min_k d2), pair_max[i][j] = sqrt(max_k d2) over the common
 * flown samples, one sqrt at the end.  No common sample: pair_min = +inf, pair_max =
 * -inf; the diagonal likewise.  Both are B x B row-major fp64 and symmetric bit for
 * bit.  rows is B x GTOP_SEP_ROW doubles:
 *   [0] the least pair_min[i][j] over j != i; +inf if there is none
 *   [1] that j, the least j on a tie; -1 if [0] is +inf
 *   [2] tau_k of the earliest common sample of (i, j) whose d2 equals the minimum;
 *       -1 if there is none
 *   [3] the number of j != i with pair_min[i][j] < radius (radius <= 0 or NaN: 0)
 *   [4] the number of j != i that have a common sample with i
 *   [5] the number of grid samples at which row i is flown
 * A pair's figures depend on neither B nor the two rows' places in the batch, and the
 * results are deterministic.  Coefficients, times and start times must be finite and
 * every position must be finite; with non-finite ones the figures are unspecified
 * (a sample with a non-finite d2 may be left out of a minimum or a maximum), but
 * every loop is bounded and the call stays memory-safe.
 *
 * gtop_separation_workspace_bytes is pure (no context): the bytes d_work needs for B
 * rows and n_samples samples (0 for B = 0); GTOP_ERR_INVALID for a NULL `bytes`, B
 * outside 0 .. GTOP_SEP_MAX_B or n_samples outside 1 .. GTOP_SEP_MAX_SAMPLES.  The
 * workspace's layout is private; nothing beyond the reported size is touched.
 *
 * gtop_separation_device only enqueues three launches on the caller's stream
 * (csrc/gtop_separation.hip: sample, pairs, rows): no allocation, no
 * synchronisation, capturable.  coeff is B x m x 18, T is B x m (time_stride m) or m
 * shared values (time_stride 0), as for the certificates.  GTOP_ERR_INVALID, nothing
 * launched: opt NULL, a non-finite t_lo or dt, dt <= 0, n_samples outside
 * 1 .. GTOP_SEP_MAX_SAMPLES, hold_ends neither 0 nor 1, a reserved word not 0,
 * B < 0 or B > GTOP_SEP_MAX_B, m outside 2 .. 227, a time_stride that is neither 0
 * nor m, a NULL buffer with B > 0, work_bytes below what
 * gtop_separation_workspace_bytes returns, a start-time count that is not 0, 1 or B.
 * B = 0 launches nothing; no field is read, so none is required.
 *
 * gtop_separation_batch serves the first B rows of the context's problem at free
 * variables x (1 <= B <= the problem's batch, B <= GTOP_SEP_MAX_B; GTOP_ERR_STATE when
 * none is set), staged as gtop_certify_batch stages; all three host outputs are
 * required.
 *
 * gtop_select_distinct_device: one launch of one workgroup; it uses no context
 * workspace, so it has no ordering rule against other calls.  pass is B bytes (may be
 * NULL), cost B doubles, pair_max B x B doubles, chosen K int32, count one int32.  A
 * row is ELIGIBLE when pass[b] != 0 (d_pass NULL: always) and cost[b] is finite.
 * chosen[0] is the eligible row of least cost, the lowest index on a tie — best[0]
 * of the gtop_select_best* family on the same pass and cost.  chosen[t] is, among the
 * eligible rows r not yet chosen with pair_max[r][c] >= min_gap against EVERY chosen
 * c (a NaN or -inf entry fails), the one of least cost, lowest index on a tie.  The
 * loop ends when no row qualifies or K rows are chosen; the remaining entries of
 * chosen are -1 and count[0] is the number chosen.  B = 0 gives count 0 and every
 * entry -1.  GTOP_ERR_INVALID, nothing launched: K outside 1 .. GTOP_SEP_MAX_DISTINCT,
 * a non-finite min_gap, B < 0 or B > GTOP_SEP_MAX_B, NULL d_cost, d_pair_max,
 * d_chosen or d_count with B > 0 (B = 0 writes the outputs that are given).
 *
 * fp64 only.  The gtop_group_* entry points do not forward these calls.
 */
#ifndef GTOP_SEPARATION_H_
#define GTOP_SEPARATION_H_

#include "gtop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double t_lo, dt;     /* the grid on the common clock: tau_k = t_lo + k*dt, k = 0 .. n_samples-1 */
  double radius;       /* row summary: pairs whose least distance is < radius are counted; <= 0 or NaN: none */
  int32_t n_samples;   /* 1 .. GTOP_SEP_MAX_SAMPLES */
  int32_t hold_ends;   /* 0: a row exists only while it is flown; 1: it stands at its start before and at its end after */
  int32_t reserved[2]; /* must be 0 */
} gtop_sep_opts;
#define GTOP_SEP_ABI_VERSION 1
#define GTOP_SEP_ROW 6
#define GTOP_SEP_MAX_SAMPLES 65536
#define GTOP_SEP_MAX_B 4096 /* two B x B fp64 matrices: 2 x 128 MiB at the limit */
#define GTOP_SEP_MAX_DISTINCT 64

/* GTOP_SEP_ABI_VERSION of the library. */
int gtop_sep_abi_version(void);
int gtop_separation_workspace_bytes(int B, int n_samples, size_t *bytes);
int gtop_separation_device(gtop_ctx *ctx, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                           const gtop_sep_opts *opt, void *d_pair_min, void *d_pair_max, void *d_rows,
                           void *d_work, size_t work_bytes, void *hip_stream);
int gtop_separation_batch(gtop_ctx *ctx, int B, const double *x, const gtop_sep_opts *opt, double *pair_min,
                          double *pair_max, double *rows);
int gtop_select_distinct_device(gtop_ctx *ctx, int B, const void *d_pass /* may be NULL */, const void *d_cost,
                                const void *d_pair_max, double min_gap, int K, void *d_chosen, void *d_count,
                                void *hip_stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_SEPARATION_H_ */
