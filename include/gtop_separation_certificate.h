/*
 * gtop_separation_certificate.h — a CONTINUOUS-TIME certificate of the pairwise
 * separation of a batch of trajectories: for every pair of rows a certified lower
 * bound of the distance between the two curves over the pair's whole common window
 * of time, not at grid samples.  A companion of gtop.h, exported from the same
 * libgtop_hip.so.
 *
 * Why a header of its own.  gtop.h is a frozen surface and gtop_separation.h is
 * pinned at its version 1 (see gtop_kinematics.h).  What is declared here is
 * versioned on its own (gtop_sepcert_abi_version, GTOP_SEPCERT_ABI_VERSION) and adds
 * nothing to either.  A library that lacks gtop_sepcert_abi_version does not have
 * this header's entry points.  gtop.h is included for gtop_ctx and the status codes.
 *
 * What it is for.  gtop_separation_device gives the least distance of two rows on a
 * time grid and knows nothing between two samples: two robots that cross at 2 m/s
 * each close 4 cm per 10 ms sample.  This call bounds the distance over whole time
 * intervals on the interval tree of the other certificates,
 * with their statuses, their budget and their rounding allowances
 * (GTOP_CERT_MAX_DEPTH = 3, INFLATE = 1 + 2^-40, SLACK = 2^-40).
 *
 * The definition.  Every step below is ONE rounded fp64 operation in the order
 * written, nothing fused; min and max are exact.  tests/sepcert_twin.py restates it.
 *   start_b     the row's start time, as gtop_separation.h states it (read when the
 *               kernels run).
 *   off_{b,k}   off_{b,0} = 0, off_{b,k+1} = off_{b,k} + T_{b,k}: accumulated as the
 *               reports accumulate time_sum.  bp_{b,k} = start_b + off_{b,k} are the
 *               row's breakpoints on the common clock, end_b = bp_{b,m}.
 *   window      hold_ends == 0: [max(max(t_lo, start_i), start_j),
 *               min(min(t_hi, end_i), end_j)].  hold_ends == 1: [t_lo, t_hi].  The
 *               pair has NO COMMON TIME unless lo <= hi.
 *   state of a row at a time a:
 *               hold_ends == 1 and a < start_b: STANDING before its start, at c0 of its
 *               first segment; hold_ends == 1 and a >= end_b: STANDING after its end,
 *               per axis at the value the library's every sample forms at u = T_{m-1}
 *               of the last segment (t2 = u u, t3 = t2 u, t4 = t2 t2, t5 = t4 u,
 *               ((((((0 + t5 c5) + t4 c4) + t3 c3) + t2 c2) + u c1) + c0)); otherwise
 *               in segment s: s = 0, and while s < m-1 and bp_{b,s+1} <= a: ++s.  A
 *               standing row is a segment with coefficients (S, 0, 0, 0, 0, 0) per
 *               axis, duration 0 and off = 0: its velocity and its second-derivative
 *               bound are 0.
 *   pieces      a = the window's lower end.  Repeat: nxt = the window's upper end,
 *               min'ed with, per row: start_b if it stands before its start; nothing if
 *               it stands after its end; else bp_{b,s+1}.  The piece is [a, nxt] with
 *               both rows in the state they have at a; it is walked when nxt > a, or
 *               when it is the first and the window is one instant (that instant is
 *               evaluated).  Stop when nxt >= the upper end or not nxt > a; else a = nxt.
 *               At most 2 m + 3 pieces (under hold_ends the 2 m + 2 breakpoints of the two
 *               rows may all lie inside the window), and the walk takes no more turns
 *               than that whatever the times are.  Symmetric in (i, j).
 *   per piece   per row and axis k, with q_n = |c_n| and T the segment's duration:
 *                 Acc_k = ((20 q5 T + 12 q4) T + 6 q3) T + 2 q2
 *                 Vel_k = (((5 q5 T + 4 q4) T + 3 q3) T + 2 q2) T + q1
 *                 Pos_k = ((((q5 T + q4) T + q3) T + q2) T + q1) T + q0
 *               A_k = Acc_{i,k} + Acc_{j,k};  remc = 0.5 sqrt((A_x A_x + A_y A_y) + A_z A_z);
 *               tmag = max(max(|a|, |nxt|), max(|start_i|, |start_j|));
 *               Pos_b = (Pos_x + Pos_y) + Pos_z, Vel_b likewise;
 *               E = GTOP_CERT_SLACK * ((Pos_i + Pos_j) + (Vel_i + Vel_j) * tmag).
 *               The tree's level 0 cuts [a, a + w0], w0 = nxt - a, into 64 intervals of
 *               width 0.015625 w0 from base a.
 *   interval [a, a + w]:
 *               h = 0.5 w, tc = a + h; per row u = (tc - start) - off;
 *               P_k = ((((c5 u + c4) u + c3) u + c2) u + c1) u + c0
 *               V_k = ((((5 c5) u + 4 c4) u + 3 c3) u + 2 c2) u + c1
 *               D = P_i - P_j, W = V_i - V_j, dmid = sqrt((Dx Dx + Dy Dy) + Dz Dz);
 *               DW = (Dx Wx + Dy Wy) + Dz Wz, WW = (Wx Wx + Wy Wy) + Wz Wz, q = (-DW) / WW;
 *               s = 0 where WW == 0 or q is NaN, else min(max(q, -h), h);
 *               L_k = D_k + W_k s, dlin = sqrt((Lx Lx + Ly Ly) + Lz Lz);
 *               rem = (remc h) h;
 *               lb = ((dlin (1 - 2^-40)) - rem GTOP_CERT_INFLATE) - E; a NaN lb is -inf.
 *               Sound because |D(t)| >= min_s |D + W s| - |R| with |R_k| <= A_k h^2 / 2.
 *   status      VIOLATION if dmid < min_sep; else CERTIFIED if lb >= min_sep; else OPEN.
 *               Every midpoint enters hi: the least dmid, the earliest tc on a tie.  A
 *               leaf of the tree commits lb into lo = the least leaf bound.
 *   cull == 1   a prepass gives each row a box of its whole curve: per segment 64
 *               intervals of width w = 0.015625 T, a = (double)lane w, h = 0.5 w,
 *               tc = a + h; per axis r = ((|V_k| h + ((0.5 Acc_k) h) h) INFLATE) +
 *               SLACK Pos_k, the face pair P_k - r, P_k + r, min and max over all; a NaN
 *               face anywhere makes the row's box the whole space (-inf, +inf per axis).
 *               g_k = max(max(lo_{i,k} - hi_{j,k}, lo_{j,k} - hi_{i,k}), 0),
 *               boxdist = sqrt((gx gx + gy gy) + gz gz).  A pair
 *               with boxdist >= min_sep is certified at once; every other pair is
 *               computed exactly as with cull == 0.
 *
 * pairs is B x B x GTOP_SEPCERT_PAIR doubles, symmetric bit for bit:
 *   [0] verdict: 1 SAFE, 0 UNDECIDED, -1 UNSAFE; no common time gives 1
 *   [1] lo: the certified lower bound of the distance over the pair's whole window;
 *       +inf without common time
 *   [2] hi: the least midpoint distance evaluated, at every level; +inf if none
 *   [3] the common-clock time of the earliest midpoint attaining hi; -1 if none
 *   [4] the common-clock time of the earliest violating midpoint; -1 if none
 *   [5] OPEN intervals left   [6] refinements done (max_refine is per PAIR)
 *   [7] pieces walked; -1 when the pair was certified by its boxes
 * The diagonal is (1, +inf, +inf, -1, -1, 0, 0, 0); a pair certified by its boxes is
 * (1, boxdist (1 - 2^-40), +inf, -1, -1, 0, 0, -1).  A SAFE pair that walked the tree
 * has lo >= min_sep; a pair certified by its boxes has boxdist >= min_sep, and its lo,
 * which is boxdist lowered past the rounding of the one sqrt, may be below min_sep by
 * up to min_sep 2^-40: for such a pair the law is lo >= min_sep (1 - 2^-40).
 * rows is B x GTOP_SEPCERT_ROW doubles, row i from row i of pairs over j != i:
 *   [0] verdict: -1 if any pair is UNSAFE, else 0 if any is UNDECIDED, else 1
 *   [1] the least lo   [2] its j, the least j on a tie; -1 if [1] is +inf
 *   [3] the least hi   [4] its j, the least j on a tie; -1 if [3] is +inf
 *   [5] that pair's entry 3; -1 if [3] is +inf
 *   [6] the earliest violation time over the UNSAFE pairs; -1 if none
 *   [7] the number of UNSAFE pairs   [8] of UNDECIDED pairs
 *   [9] pairs certified by their boxes
 * A pair's row depends on neither B nor the two rows' places in the batch.  Inputs
 * must be finite; with non-finite ones the figures are unspecified, but a NaN bound
 * certifies nothing, every loop is bounded and the call stays memory-safe.
 *
 * gtop_sepcert_workspace_bytes is pure (no context): the bytes d_work needs for B rows
 * (0 for B = 0); GTOP_ERR_INVALID for a NULL `bytes` or B outside
 * 0 .. GTOP_SEPCERT_MAX_B.  The layout is private.
 *
 * gtop_certify_separation_device only enqueues launches on the caller's stream
 * (csrc/gtop_separation_certificate.hip: boxes when cull == 1, pairs, rows): no
 * allocation, no synchronisation, capturable.  coeff is B x m x 18, T is B x m
 * (time_stride m) or m shared values (time_stride 0).  GTOP_ERR_INVALID, nothing
 * launched: opt NULL, min_sep not finite or <= 0, a NaN t_lo or t_hi, t_lo > t_hi,
 * hold_ends == 1 with an infinite t_lo or t_hi, max_depth outside
 * 0 .. GTOP_CERT_MAX_DEPTH, max_refine < 0, hold_ends or cull neither 0 nor 1, a
 * reserved word not 0, B < 0 or B > GTOP_SEPCERT_MAX_B, m outside 2 .. 227, a
 * time_stride that is neither 0 nor m, a NULL buffer with B > 0, work_bytes below what
 * gtop_sepcert_workspace_bytes returns, a start-time count that is not 0, 1 or B.
 * B = 0 launches nothing; no field is read, so none is required.
 *
 * gtop_certify_separation_batch serves the first B rows of the context's problem at
 * free variables x (1 <= B <= the problem's batch, B <= GTOP_SEPCERT_MAX_B;
 * GTOP_ERR_STATE when none is set), staged as gtop_separation_batch stages; both host
 * outputs are required.
 *
 * fp64 only.  The gtop_group_* entry points do not forward these calls.
 */
#ifndef GTOP_SEPARATION_CERTIFICATE_H_
#define GTOP_SEPARATION_CERTIFICATE_H_

#include "gtop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double min_sep;      /* the separation required: finite, > 0 */
  double t_lo, t_hi;   /* the window on the common clock, t_lo <= t_hi; with hold_ends == 0 either may be
                          infinite (the rows' own flown ranges bound it); with hold_ends == 1 both finite */
  int32_t max_depth;   /* 0 .. GTOP_CERT_MAX_DEPTH */
  int32_t max_refine;  /* >= 0: refinements per PAIR */
  int32_t hold_ends;   /* 0 / 1, as gtop_sep_opts */
  int32_t cull;        /* 0: every pair walks the tree; 1: pairs whose row boxes are >= min_sep apart are certified at once */
  int32_t reserved[2]; /* must be 0 */
} gtop_sepcert_opts;
#define GTOP_SEPCERT_ABI_VERSION 1
#define GTOP_SEPCERT_PAIR 8
#define GTOP_SEPCERT_ROW 10
#define GTOP_SEPCERT_MAX_B 2048 /* pairs is B x B x 8 fp64: 256 MiB at the limit */

/* GTOP_SEPCERT_ABI_VERSION of the library. */
int gtop_sepcert_abi_version(void);
int gtop_sepcert_workspace_bytes(int B, size_t *bytes);
int gtop_certify_separation_device(gtop_ctx *ctx, int B, int m, const void *d_coeff, const void *d_T, int time_stride,
                                   const gtop_sepcert_opts *opt, void *d_pairs, void *d_rows, void *d_work,
                                   size_t work_bytes, void *hip_stream);
int gtop_certify_separation_batch(gtop_ctx *ctx, int B, const double *x, const gtop_sepcert_opts *opt, double *pairs,
                                  double *rows);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GTOP_SEPARATION_CERTIFICATE_H_ */
