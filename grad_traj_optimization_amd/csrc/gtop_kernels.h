// gtop_kernels.h — launch interface between the C-ABI layer (gtop_capi*.cpp)
// and the gfx950 kernels (the launchers of gtop_kernels.hip, gtop_esdf.hip, ...); the launch rule and its
// GtopEvalPlan are gtop_launch_rule.h's, included here.  Internal; the public boundary is include/gtop.h.
#ifndef GTOP_KERNELS_H_
#define GTOP_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gtop_launch_rule.h"

// Kernel arguments of gtop_eval_wave_kernel<R>, all in the arithmetic type R of the
// launch (double for GTOP_F64, float for GTOP_F32).
template <typename R>
struct GtopKernelArgs {
  // per-trajectory inputs/outputs (HBM)
  const R *x;    // [B][n]   free variables, axis-major
  const R *Df;   // [B][3][6]
  const R *T;    // [B][m] or [m]
  R *cost;       // [B]
  R *grad;       // [B][n]
  int B, m, t_stride;
  // shared distance field — SDFMap fields, sdf_map.h:13-23.  `sdf` is the resident CORNER-RECORD copy
  // (gtop_records.hip: record (ix+1, iy+1, level+1) = the four clamped (x,y) corners of base index (ix,iy) at one z
  // level, records z-fastest), not the boundary's z-fastest buffer; nx, ny, nz are the voxel grid's.
  const R *sdf;
  int nx, ny, nz;
  R origin[3];
  R lo[3], hi[3];   // min_range + 1e-4, max_range - 1e-4  (isInMap, sdf_map.cpp:55-69)
  float lo_f[3], hi_f[3];   // lo rounded up / hi rounded down to float: for a float p, p < lo <=> p < lo_f, p > hi <=> p > hi_f
  R res, res_inv;
  // posToIndex's constants in double whatever R is: the fp32 kernels decide which cell a sample reads as the reference
  // does, in double on the widened float position (gtop_wave_kernel.h IndexBox); the fp64 kernels do not read these
  double idx_origin[3], idx_half, idx_rinv;
  // parameters — grad_traj_optimizer.cpp:5-32
  R ws, wc, alpha, d0, alpha_v, r_v, v0, alpha_a, r_a, a0;
  R inv_r, alpha_over_r;   // 1/r, alpha/r  (:509, :514)
  R inv_r_v, inv_r_a, gv_scale, ga_scale;   // 1/r_v, 1/r_a, alpha_v/r_v, alpha_a/r_a  (:517-535, the DYN bodies)
  int step;
};

// ---- batched CCSA-MMA optimizer state (gtop_mma.hip), all fp64, [B][n] / [B] ----
struct GtopMmaState {
  double *x, *xcur, *xprev, *xprevprev, *dfdx, *sigma;   // [B][n]
  const double *lb, *ub;                                  // [B][n]
  double *rho, *minf, *gval, *wval, *fprev;               // [B]; fprev: f at the start of the outer iteration
  int *k, *state, *nevals;                                // [B]; state 0 first evaluation pending, 1 running,
                                                          //      >= 3 stopped with that nlopt_result code
  int iters;                                              // evaluations per launch of the fused kernel
  int max_evals;                                          // the optimisation's evaluation cap (all launches together)
  // stop rules beside the evaluation count (mma.hpp:35-39; nlopt set_ftol_rel / set_xtol_rel / set_maxtime,
  // grad_traj_optimizer.cpp:144-148); 0 = off.  max_ticks: wall clock in ticks of the 100 MHz device clock.
  double ftol_rel, xtol_rel;
  long long max_ticks;
  // The one-launch loop of gtop_eval_wave_kernel can do without the launches around it (all optional, NULL = off):
  // x0_init: start points [B][n] — the state is initialised in the kernel (mma_init_kernel's arithmetic) instead of
  // being loaded; out_*: where the results go when the loop ends (the best point, its cost, the nlopt_result-style
  // code and the evaluations used: what the copies and mma_finish_kernel deliver otherwise).
  const double *x0_init;
  double *out_x, *out_minf;
  int *out_code, *out_nevals;
};
enum { GTOP_MMA_FTOL_REACHED = 3, GTOP_MMA_XTOL_REACHED = 4, GTOP_MMA_MAXEVAL_REACHED = 5, GTOP_MMA_MAXTIME_REACHED = 6 };
// dyn: enable_dyn (the kernel applies it at step 2 only, as the commented-out block would)
template <typename R>
hipError_t gtop_launch_eval(const GtopKernelArgs<R> &args, const GtopEvalPlan &plan, bool dyn, hipStream_t stream);
// The consistent-gradient bodies live in an object of their own (gtop_kernels.hip compiled with -DGTOP_CONSISTENT_TU);
// the *_consistent launchers are that object's and are called by the launchers of the same name only.
template <typename R>
hipError_t gtop_launch_eval_consistent(const GtopKernelArgs<R> &args, const GtopEvalPlan &plan, bool dyn, hipStream_t stream);

// ---- the moving-obstacle term (gtop_set_moving_cost): the lookup of every collision sample becomes
// evaluateEDTWithGrad(pos, tau), the 8 corner values min'ed with the distance to the nearest box at the sample's
// absolute time (fp64 bodies only) ----
#define GTOP_MOVING_MAX_BOXES 32   // = GTOP_MOVING_COST_MAX_BOXES of include/gtop.h (checked in gtop_capi_boxes.cpp)
struct GtopMovingArgs {
  const double *rows;   // [nbox][9]: p0, vel, scale / 2 — wavefront-uniform, read through scalar loads
                        // (poly: [nbox][24], the rows of gtop_set_moving_box_polynomials, gtop_edt_lookup.h)
  int nbox;             // 1 .. GTOP_MOVING_MAX_BOXES
  const double *t0;     // start times on the boxes' clock; NULL = all zero
  int t0_stride;        // 0 = one shared value, 1 = one per trajectory
  int poly = 0;         // the list's kind (GTOP_BOXES_POLYNOMIAL): selects the body, so a captured launch keeps it
};
hipError_t gtop_launch_eval_moving(const GtopKernelArgs<double> &args, const GtopEvalPlan &plan, bool dyn,
                                   const GtopMovingArgs &mov, hipStream_t stream);
hipError_t gtop_launch_eval_mma_moving(const GtopKernelArgs<double> &args, const GtopMmaState &st, const GtopEvalPlan &plan,
                                       bool dyn, const GtopMovingArgs &mov, hipStream_t stream);
hipError_t gtop_launch_eval_moving_consistent(const GtopKernelArgs<double> &args, const GtopEvalPlan &plan, bool dyn,
                                              const GtopMovingArgs &mov, hipStream_t stream);
hipError_t gtop_launch_eval_mma_moving_consistent(const GtopKernelArgs<double> &args, const GtopMmaState &st,
                                                  const GtopEvalPlan &plan, bool dyn, const GtopMovingArgs &mov,
                                                  hipStream_t stream);

// `bytes` from src to each of the first n_dsts pointers of `dsts` (device memory of this or of a peer GPU mapped into
// this process; 16-byte aligned), one kernel: gtop_push.hip
#define GTOP_PUSH_MAX_DSTS 16
struct GtopPushDsts { void *p[GTOP_PUSH_MAX_DSTS]; };
hipError_t gtop_launch_push_rows(const void *src, size_t bytes, const GtopPushDsts &dsts, int n_dsts,
                                 unsigned long long *minmax /* optional clock stamp, NULL = none */, hipStream_t stream);

// minmax[0] = min(minmax[0], clock), minmax[1] = max(minmax[1], clock) of the device's constant-rate wall clock
hipError_t gtop_launch_clock_stamp(unsigned long long *minmax, hipStream_t stream);

// ---- ESDF construction (gtop_esdf.hip) -----------------------------------
struct GtopGrid {
  int nx, ny, nz;
  double origin[3], min_range[3], max_range[3];
  double res, res_inv;
};

// occupancy := 0, distance := 10000   (sdf_map.cpp:26-53)
hipError_t gtop_launch_esdf_reset(uint8_t *occ, double *dist, size_t nvox, hipStream_t stream);
// setOccupancy per point (sdf_map.cpp:80-99)
hipError_t gtop_launch_esdf_mark(const GtopGrid &g, const double *pts, int npts, uint8_t *occ,
                                 hipStream_t stream);
// updateESDF3d (sdf_map.cpp:310-368): the three sweeps z, y, x as exact integer minimisations,
// then res*sqrt(.) into dist, in fp64 only (the fp32 path reads fp32 corner records, which gtop_records.hip makes from
// dist).  tmp1/tmp2: nvox int32 each.
bool gtop_esdf_supported(const GtopGrid &g);
size_t gtop_esdf_rows_ints(const GtopGrid &g);   // ints of row workspace the builder needs
hipError_t gtop_launch_esdf_build(const GtopGrid &g, const uint8_t *occ, int *tmp1, int *tmp2, int *rows,
                                  double *dist, hipStream_t stream);
// The signed field (gtop_set_field_sign): the distance field above at free voxels; at occupied ones
// max(-max_depth, res - res*sqrt(n)), n the squared voxel distance to the nearest free voxel (-max_depth if none).
// Two transforms over the same workspaces.
hipError_t gtop_launch_esdf_build_signed(const GtopGrid &g, const uint8_t *occ, int *tmp1, int *tmp2, int *rows,
                                         double *dist, double max_depth, hipStream_t stream);

// the local update of compare2.cpp:147-152 (gtop_esdf_window.hip): resetBuffer(min, max) over the inclusive voxel box
// lo .. hi, and updateESDF3d over the same box (sdf_map.cpp:28-53, :310-368)
hipError_t gtop_launch_esdf_window_reset(const GtopGrid &g, const int lo[3], const int hi[3], uint8_t *occ, double *dist,
                                         hipStream_t stream);
hipError_t gtop_launch_esdf_window_build(const GtopGrid &g, const int lo[3], const int hi[3], const uint8_t *occ, int *tmp1,
                                         int *tmp2, double *dist, hipStream_t stream);
// the same, signed (gtop_launch_esdf_build_signed over the window taken alone)
hipError_t gtop_launch_esdf_window_build_signed(const GtopGrid &g, const int lo[3], const int hi[3], const uint8_t *occ,
                                                int *tmp1, int *tmp2, double *dist, double max_depth, hipStream_t stream);
// a compact grid's distances (z fastest) into the window
hipError_t gtop_launch_esdf_window_scatter(const GtopGrid &g, const int lo[3], const int hi[3], const double *sub,
                                           double *dist, hipStream_t stream);
// the compact path's reset + marking without a gather: clears the window's occupancy in the map and in `sub`, marks the
// points in the map and (inside the window) in `sub`; the distances are not reset (the scatter rewrites the window)
hipError_t gtop_launch_esdf_window_reset_mark_compact(const GtopGrid &g, const int lo[3], const int hi[3], const double *pts,
                                                      int npts, uint8_t *occ, uint8_t *sub, hipStream_t stream);

// ---- corner records (gtop_records.hip): the gather-friendly resident copy the lookups read ----
size_t gtop_record_count(const GtopGrid &g);   // (nx+1)(ny+1)(nz+2) records of 4 values
// S -> D in {double -> double, double -> float, float -> float}; rec32 (may be NULL): the fp32 records too, in the
// same pass; vlo / vhi: inclusive voxel box whose records are rebuilt (NULL = the whole field)
template <typename S, typename D>
hipError_t gtop_launch_build_records(const GtopGrid &g, const S *field, D *rec, float *rec32, const int *vlo,
                                     const int *vhi, hipStream_t stream);

// the optimizer loop: st.iters x {cost/gradient at st.xcur, CCSA-MMA update} per trajectory in one launch (fp64; a plan
// made with for_optimizer = true); honours st.x0_init / st.out_*
hipError_t gtop_launch_eval_mma(const GtopKernelArgs<double> &args, const GtopMmaState &st, const GtopEvalPlan &plan,
                                bool dyn, hipStream_t stream);
hipError_t gtop_launch_eval_mma(const GtopKernelArgs<float> &args, const GtopMmaState &st, const GtopEvalPlan &plan,
                                bool dyn, hipStream_t stream);
hipError_t gtop_launch_eval_mma_consistent(const GtopKernelArgs<double> &args, const GtopMmaState &st,
                                           const GtopEvalPlan &plan, bool dyn, hipStream_t stream);
hipError_t gtop_launch_eval_mma_consistent(const GtopKernelArgs<float> &args, const GtopMmaState &st,
                                           const GtopEvalPlan &plan, bool dyn, hipStream_t stream);
hipError_t gtop_launch_mma_init(const GtopMmaState &st, int B, int n, const double *x0, hipStream_t stream);
hipError_t gtop_launch_mma_update(const GtopMmaState &st, int B, int n, const double *fcur, const double *gcur,
                                  hipStream_t stream);
// code[b] = nlopt_result-style stop code, nevals[b] = evaluations used (either may be NULL)
hipError_t gtop_launch_mma_finish(const GtopMmaState &st, int B, int *code, int *nevals, hipStream_t stream);

// ---- setup + post-processing (gtop_setup.hip), fp64 ----
#define GTOP_TRAJ_STATS 9   // time_sum, length, jerk, mean_v, max_v, mean_a, max_a, acc_cost, n_samples
hipError_t gtop_launch_setup_paths(int B, int m, const double *wp, double mean_v, double init_time, double *T,
                                   double *Df, double *x0, hipStream_t stream);
hipError_t gtop_launch_coefficients(int B, int m, const double *x, const double *Df, const double *T, int t_stride,
                                    double *coeff, hipStream_t stream);
// samples (may be NULL): [B][max_samples][3] getTraj points
hipError_t gtop_launch_eval_trajectories(int B, int m, const double *coeff, const double *T, int t_stride,
                                         double dt_sample, double *out, double *samples, int max_samples,
                                         hipStream_t stream);

// ---- the minimum-jerk start point (gtop_minjerk.hip; its launch plan: gtop_minjerk_plan.h), fp64 ----
// Overwrites the velocity and acceleration entries of x [B][9 (m - 1)] with the minimiser of the smoothness term at the
// positions x holds; hipErrorInvalidValue where the plan refuses (m outside 2 .. 227, B < 0)
hipError_t gtop_launch_min_jerk_start(int B, int m, double *x, const double *Df, const double *T, int t_stride,
                                      hipStream_t stream);

// ---- static field + moving boxes (gtop_edt.hip) -----------------------------
// The box list the query and the report take: one of two kinds, with the pointers of that kind (the other kind's stay
// NULL); count 0 = no boxes, whatever the kind.
constexpr int kBoxRowPoly = 24;   // doubles per row of a polynomial list: device code (gtop_edt_lookup.h) and host alike
enum GtopBoxKind { GTOP_BOX_LIST_CONST_VEL = 0, GTOP_BOX_LIST_POLYNOMIAL = 1 };
struct GtopBoxList {
  GtopBoxKind kind;
  int count;
  const double *p0, *vel, *scale;   // constant velocity: count x 3 each
  const double *rows;               // polynomial (gtop_set_moving_box_polynomials): [count][kBoxRowPoly], gtop_edt_lookup.h
};
// field: the z-fastest fp64 buffer (the coarse query's voxel values); rec: its corner records (the interpolating query);
// grad NULL: the coarse query.
hipError_t gtop_launch_edt_query(const GtopGrid &g, const double *field, const double *rec, const GtopBoxList &boxes, int N,
                                 const double *pos, const double *time, double *dist, double *grad, hipStream_t stream);

// ---- trajectory report + selection (gtop_validate.hip), fp64 -----------------
#define GTOP_TRAJ_REPORT 12   // = include/gtop.h
// report[b] of the trajectories (coeff, T) as include/gtop.h lays it out: the getTraj samples looked up as
// edt_query_kernel<false> looks (pos, tau) up, tau = t0[b * t0_stride] + eval_t (t0 NULL = 0) — with no boxes static only
hipError_t gtop_launch_traj_report(const GtopGrid &g, const double *rec, const GtopBoxList &boxes, int B, int m,
                                   const double *coeff, const double *T, int t_stride, double dt_sample, const double *t0,
                                   int t0_stride, double margin, double *report,
                                   int simds /* of the device: sizes the launch */, hipStream_t stream);
// pass[b] (may be NULL) and best[2] = {passing row of least cost (lowest index on a tie, -1 if none), passing rows};
// two launches; workspace: GTOP_SELECT_PARTIALS x GTOP_SELECT_PARTIAL_BYTES bytes of device memory
#define GTOP_SELECT_PARTIALS 256
#define GTOP_SELECT_PARTIAL_BYTES 16
// cert (may be NULL: gtop_select_best_device): the certificates of the rows, [B][GTOP_CERT_REPORT]; a row then also
// needs verdict == +1 (require GTOP_CERT_REQUIRE_SAFE) or verdict != -1 (GTOP_CERT_REQUIRE_NOT_UNSAFE) to pass.
// kin (may be NULL: both selections of include/gtop.h): the kinematic certificates, [B][GTOP_KIN_REPORT], held to the
// same `require` (include/gtop_kinematics.h, gtop_select_best_kin_certified_device)
hipError_t gtop_launch_select_best(int B, const double *report, const double *cost, double max_vel, double max_acc,
                                   int per_axis, int allow_out_of_map, const double *cert, const double *kin,
                                   int require, unsigned char *pass, int *best, void *workspace, hipStream_t stream);

// ---- continuous-time clearance certificate (gtop_certify.hip), fp64: the static field, and the field with the boxes ----
#define GTOP_CERT_REPORT 8      // = include/gtop.h
#define GTOP_CERT_MAX_DEPTH 3   // = include/gtop.h: levels 0 .. 3
#define GTOP_CERT_REQUIRE_SAFE 1         // = include/gtop.h
#define GTOP_CERT_REQUIRE_NOT_UNSAFE 2   // = include/gtop.h
// The rounding allowances, DESIGN.md §5.13.  A box's radius r becomes r * INFLATE + SLACK * (P_k + coord), P_k =
// sum_j |c_j| T^j of the segment and axis, coord = the map's largest absolute face coordinate; a cell's vertex minimum
// is lowered by KAPPA * (8 + coord / res) * the largest |corner value| involved.
#define GTOP_CERT_INFLATE (1.0 + 0x1p-40)
#define GTOP_CERT_SLACK 0x1p-40
#define GTOP_CERT_KAPPA 0x1p-46
// cert[b] of the trajectories (coeff, T) as include/gtop.h lays it out; one wavefront per trajectory, one launch
hipError_t gtop_launch_traj_certify(const GtopGrid &g, const double *rec, int B, int m, const double *coeff,
                                    const double *T, int t_stride, double margin, int max_depth, int max_refine,
                                    double *cert, hipStream_t stream);
// The same against the static field and the boxes over whole ranges of box time (include/gtop.h,
// gtop_certify_moving_device): box time = t0[b * t0_stride] + trajectory time (t0 NULL = 0); both list kinds, any number
// of boxes; no boxes: the launch above
hipError_t gtop_launch_traj_certify_moving(const GtopGrid &g, const double *rec, const GtopBoxList &boxes, int B, int m,
                                           const double *coeff, const double *T, int t_stride, const double *t0,
                                           int t0_stride, double margin, int max_depth, int max_refine, double *cert,
                                           hipStream_t stream);

// ---- per-segment report (gtop_segments.hip) and segment-time reallocation (gtop_retime.hip), fp64 ------------
#define GTOP_SEG_REPORT 10   // = include/gtop.h
// seg_report[b][s] of the trajectories (coeff, T) as include/gtop.h lays it out: traj_report_kernel's samples, segments
// and distances, reduced per segment; one wavefront per trajectory, both list kinds, any number of boxes
hipError_t gtop_launch_traj_segments(const GtopGrid &g, const double *rec, const GtopBoxList &boxes, int B, int m,
                                     const double *coeff, const double *T, int t_stride, double dt_sample,
                                     const double *t0, int t0_stride, double margin, double *seg_report,
                                     hipStream_t stream);
// T_out [B][m] = length / mean_v of the waypoints as they stand in x and Df, init_time on the first and last segment
hipError_t gtop_launch_retime_length(int B, int m, const double *x, const double *Df, double mean_v, double init_time,
                                     double *T_out, hipStream_t stream);
// T_out [B][m] = ratio_s T[s] from the segment report's velocity / acceleration figures; scale_x: the interior
// velocities and accelerations of x divided by rho_k, rho_k^2 in place (x may be NULL otherwise)
hipError_t gtop_launch_retime_limits(int B, int m, double *x, const double *T, int t_stride, const double *seg_report,
                                     double max_vel, double max_acc, double max_ratio, int per_axis, int uniform,
                                     int scale_x, double *T_out, hipStream_t stream);

// ---- continuous-time kinematic certificate (gtop_kinematics.hip), fp64 -------------------------------------------
#define GTOP_KIN_REPORT 11   // = include/gtop_kinematics.h
#define GTOP_KIN_SEG 10      // = include/gtop_kinematics.h; == GTOP_SEG_REPORT (checked in gtop_kinematics.hip)
// kin[b] and (seg may be NULL) seg[b][s] of the trajectories (coeff, T) as include/gtop_kinematics.h lays them out:
// certified upper and attained lower bounds of ‖v‖, ‖a‖, max|v_k|, max|a_k| over whole time intervals on the interval
// tree of gtop_certify.hip, with its INFLATE and SLACK; one wavefront per trajectory, one launch
hipError_t gtop_launch_traj_kinematics(int B, int m, const double *coeff, const double *T, int t_stride, double max_vel,
                                       double max_acc, int per_axis, int max_depth, int max_refine, double *kin,
                                       double *seg, hipStream_t stream);

// ---- pairwise separation and distinct-candidate selection (gtop_separation.hip), fp64 ----------------------------
#define GTOP_SEP_ROW 6   // = include/gtop_separation.h
// the bytes of the workspace gtop_launch_separation needs for B rows on n_samples samples (its layout is the kernels')
size_t gtop_separation_work_bytes(int B, int n_samples);
// pair_min, pair_max [B][B] and rows [B][GTOP_SEP_ROW] of the trajectories (coeff, T) on the grid t_lo + k dt as
// include/gtop_separation.h lays them out; t0 (NULL: every start 0) with stride 0 or 1; three launches (sample, pairs,
// rows), work as sized above
hipError_t gtop_launch_separation(int B, int m, const double *coeff, const double *T, int t_stride, const double *t0,
                                  int t0_stride, double t_lo, double dt, int n_samples, int hold_ends, double radius,
                                  double *pair_min, double *pair_max, double *rows, void *work, hipStream_t stream);
// chosen [K] and count [1] (either may be NULL) by the greedy rule of include/gtop_separation.h; pass may be NULL;
// one launch of one workgroup, B = 0 included
hipError_t gtop_launch_select_distinct(int B, const unsigned char *pass, const double *cost, const double *pair_max,
                                       double min_gap, int K, int *chosen, int *count, hipStream_t stream);

// ---- continuous-time certificate of pairwise separation (gtop_separation_certificate.hip), fp64 ------------------
#define GTOP_SEPCERT_PAIR 8   // = include/gtop_separation_certificate.h
#define GTOP_SEPCERT_ROW 10   // = include/gtop_separation_certificate.h
// the bytes of the workspace gtop_launch_certify_separation needs for B rows (the rows' boxes)
size_t gtop_sepcert_work_bytes(int B);
// pairs [B][B][GTOP_SEPCERT_PAIR] and rows [B][GTOP_SEPCERT_ROW] of the trajectories (coeff, T) as
// include/gtop_separation_certificate.h lays them out, on the interval tree of gtop_certify.hip with its INFLATE and
// SLACK; t0 (NULL: every start 0) with stride 0 or 1; one wavefront per pair; two launches (pairs, rows), three with cull
hipError_t gtop_launch_certify_separation(int B, int m, const double *coeff, const double *T, int t_stride,
                                          const double *t0, int t0_stride, double min_sep, double t_lo, double t_hi,
                                          int max_depth, int max_refine, int hold_ends, int cull, double *pairs,
                                          double *rows, void *work, hipStream_t stream);

// ---- predictions fitted from observation histories (gtop_prediction.hip), fp64 -----------------------------------
struct GtopPredictArgs;   // gtop_prediction_fit.h: gtop_predict_opts as the kernel takes it
// coef [N][18], t_range [N][2], info [N][12] and local [N][20] (may be NULL) of the histories hist [N][H][4] (16-byte
// aligned), count [N], head [N] (may be NULL) as include/gtop_prediction.h lays them out; one wavefront per object, one
// launch, none for N = 0
hipError_t gtop_launch_fit_predictions(int mode, int N, int H, const double *hist, const int *count, const int *head,
                                       const GtopPredictArgs &o, double *coef, double *t_range, double *info,
                                       double *local, hipStream_t stream);
// the same fit written into rows [N][kBoxRowPoly] of a polynomial box list and, where given, into cost_rows (the rows
// the cost bodies read); scale [N][3] (NULL: the extents stay); one launch
hipError_t gtop_launch_refresh_predictions(int mode, int N, int H, const double *hist, const int *count, const int *head,
                                           const GtopPredictArgs &o, const double *scale, double *rows, double *cost_rows,
                                           double *info, hipStream_t stream);

// ---- waypoint insertion (gtop_insert.hip), fp64 ------------------------------------------------------------------
#define GTOP_INSERT_AT_TIME 0  // = include/gtop.h
#define GTOP_INSERT_LONGEST 1   // = include/gtop.h
#define GTOP_INSERT_INFO 6      // = include/gtop.h
// One segment of every row cut in two as include/gtop.h states it: x_out, lb_out, ub_out [B][9m], T_out [B][m + 1],
// info [B][GTOP_INSERT_INFO].  when is read under AT_TIME only; lb, ub, lb_out, ub_out all or none; info may be NULL;
// g and rec (the fp64 corner records) are read only when push > 0.  One wavefront per trajectory, one launch.
hipError_t gtop_launch_insert_waypoints(const GtopGrid &g, const double *rec, int mode, double min_fraction, double push,
                                        double push_below, double bos, double vos, double aos, int B, int m,
                                        const double *x, const double *coeff, const double *T, int t_stride,
                                        const double *when, int when_stride, const double *lb, const double *ub,
                                        double *x_out, double *T_out, double *lb_out, double *ub_out, double *info,
                                        hipStream_t stream);

// ---- segment-time gradient and segment-time optimizer (gtop_time.hip), fp64 --------------------------------------
#define GTOP_TIME_PARTS 4     // = include/gtop_time.h
#define GTOP_TIMEOPT_INFO 8   // = include/gtop_time.h
// the cost's parameters as gtop_set_params holds them (gtop_params of include/gtop.h, which this header does not see)
struct GtopTimeCost {
  double ws, wc, alpha, r, d0, alpha_v, r_v, v0, alpha_a, r_a, a0;
  int step, enable_dyn;
};
// cost [B], gT [B][m] and parts [B][m][GTOP_TIME_PARTS] (may be NULL) as include/gtop_time.h lays them out; rec: the
// fp64 corner records; one wavefront per trajectory, one launch
hipError_t gtop_launch_time_gradient(const GtopGrid &g, const double *rec, const GtopTimeCost &p, int B, int m,
                                     const double *x, const double *Df, const double *T, int t_stride, double *cost,
                                     double *gT, double *parts, hipStream_t stream);
// T_out [B][m] and info [B][GTOP_TIMEOPT_INFO] by the rule of include/gtop_time.h; T_lo [B][m] may be NULL; one launch
hipError_t gtop_launch_time_optimize(const GtopGrid &g, const double *rec, const GtopTimeCost &p, double rho,
                                     double t_min, double t_max, double first_move, double ftol_rel, double xtol_abs,
                                     int max_evals, int B, int m, const double *x, const double *Df, const double *T,
                                     int t_stride, const double *T_lo, double *T_out, double *info, hipStream_t stream);

// ---- the same under the moving-obstacle cost (gtop_time_moving.hip), fp64 -----------------------------------------
#define GTOP_TIME_MOVING_PARTS 6   // = include/gtop_time_moving.h
// cost [B], gT [B][m], gt0 [B] (may be NULL) and parts [B][m][GTOP_TIME_MOVING_PARTS] (may be NULL) as
// include/gtop_time_moving.h lays them out.  boxes: at most GTOP_MOVING_MAX_BOXES of either kind (more:
// hipErrorInvalidValue); count 0: the static lookup, the moving columns 0.  t0 (NULL: every start 0) with stride 0 or 1.
// One wavefront per trajectory, one launch
hipError_t gtop_launch_time_gradient_moving(const GtopGrid &g, const double *rec, const GtopTimeCost &p,
                                            const GtopBoxList &boxes, const double *t0, int t0_stride, int B, int m,
                                            const double *x, const double *Df, const double *T, int t_stride,
                                            double *cost, double *gT, double *gt0, double *parts, hipStream_t stream);
// gtop_launch_time_optimize with that pass as its evaluation; 1 .. GTOP_MOVING_MAX_BOXES boxes; one launch
hipError_t gtop_launch_time_optimize_moving(const GtopGrid &g, const double *rec, const GtopTimeCost &p,
                                            const GtopBoxList &boxes, const double *t0, int t0_stride, double rho,
                                            double t_min, double t_max, double first_move, double ftol_rel,
                                            double xtol_abs, int max_evals, int B, int m, const double *x,
                                            const double *Df, const double *T, int t_stride, const double *T_lo,
                                            double *T_out, double *info, hipStream_t stream);

// ---- swarm separation cost (gtop_swarm.hip), fp64 ----------------------------------------------------------------
// the common grid of include/gtop_swarm.h's options
struct GtopSwarmGrid {
  double t_lo, dt;
  int n_samples, hold_ends;
};
// the bytes of the workspace the launches below need for B rows of m segments on n_samples samples (its layout is the
// kernels'), and the two regions of it the optimizer's entry uses itself: the coefficient scratch [B][m][18] of a round
// and S [B] of the closing joint evaluation
size_t gtop_swarm_work_bytes(int B, int m, int n_samples);
double *gtop_swarm_coeff_scratch(void *work, int B, int m, int n_samples);
double *gtop_swarm_joint_scratch(void *work, int B, int m, int n_samples);
// the rows (coeff, T) sampled on the grid into side 0 (the trial rows) or 1 (the frozen rows) of the workspace; t0
// (NULL: every start 0) with stride 0 or 1; one launch
hipError_t gtop_launch_swarm_sample(const GtopSwarmGrid &g, int B, int m, const double *coeff, const double *T,
                                    int t_stride, const double *t0, int t0_stride, int side, void *work,
                                    hipStream_t stream);
// S [B], grad [B][9 (m - 1)] and active [B] (may be NULL) of the trial rows sampled in side 0 against the rows of
// partner_side (0: the batch itself) as include/gtop_swarm.h lays them out; add != 0: S and grad are ADDED to f and grad;
// two launches (pairs, rows)
hipError_t gtop_launch_swarm_terms(const GtopSwarmGrid &g, double w, double radius, int B, int m, const double *T,
                                   int t_stride, const double *t0, int t0_stride, int partner_side, int add, double *f,
                                   double *grad, double *active, void *work, hipStream_t stream);
// joint [B][2] = cost [B] | S [B] (NULL: +0); one launch
hipError_t gtop_launch_swarm_joint(int B, const double *cost, const double *S, double *joint, hipStream_t stream);

// ---- the joint pass over waypoint derivatives and segment times, and its optimizer's own launches (gtop_joint.hip),
// fp64 ----
#define GTOP_JOINT_INFO 8   // = include/gtop_joint.h
// One pass per row: f, d f / d x (9 (m - 1) entries at gx) and d f / d T (m entries at gT; parts as
// gtop_launch_time_gradient, may be NULL).  Every row pointer comes with its stride in doubles, so that the pass runs on
// separate buffers (the public gradient) and on a packed state z = [x | T] with f | g beside it (the optimizer).
// with_rho: f = cost + rho sum_s T_s and rho is added to every gT entry; else f = cost and gT is bare.
// aux (may be NULL): aux[b * aux_stride] = the cost without the rho term (aux_plain) or f.
struct GtopJointRows {
  const double *x; size_t x_stride;
  const double *T; size_t t_stride;   // 0: one row of times for all
  double *f; size_t f_stride;
  double *gx; size_t gx_stride;
  double *gT; size_t gt_stride;
  double *aux; size_t aux_stride;
  int aux_plain;
};
hipError_t gtop_launch_joint_pass(const GtopGrid &g, const double *rec, const GtopTimeCost &p, int B, int m,
                                  const GtopJointRows &rows, const double *Df, int with_rho, double rho, double *parts,
                                  hipStream_t stream);
// the packed start point z0 [B][10m - 9] = [x | T] and the packed bounds zlb, zub = [lb | lo] , [ub | hi]: lo_s =
// max(t_min, T_lo[b][s]) (T_lo NULL: t_min), hi_s = t_max, and lo_s > t_max pins the segment: lo_s = hi_s; one launch
hipError_t gtop_launch_joint_pack(int B, int m, const double *x, const double *T, int t_stride, const double *lb,
                                  const double *ub, const double *T_lo, double t_min, double t_max, double *z0,
                                  double *zlb, double *zub, hipStream_t stream);
// the results of a finished loop: x_out, T_out from the best point z [B][10m - 9], and info [B][GTOP_JOINT_INFO] but
// its entries [2] and [4] (written by the passes) from the gradient g at that point, the bounds, minf, code and nevals
hipError_t gtop_launch_joint_report(int B, int m, const double *z, const double *g, const double *zlb, const double *zub,
                                    const double *minf, const int *code, const int *nevals, double *x_out, double *T_out,
                                    double *info, hipStream_t stream);

#endif  // GTOP_KERNELS_H_
