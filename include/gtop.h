/*
 * gtop.h — C-ABI of the MI355X-native batched cost/gradient path of GTOP.
 *
 * This is the drop-in boundary.  Each entry point names the
 * reference interface it replaces as file:line into the reference tree
 * (EpicOne1/grad_traj_optimization).  Plain pointers and sizes only; no C++
 * or torch types; no exceptions cross this boundary (every entry point that can
 * allocate is a function-try-block, csrc/gtop_guard.h: whatever is thrown inside
 * comes back as GTOP_ERR_INTERNAL) — every function returns a gtop_status
 * (0 = OK) except gtop_cost_nlopt / gtop_cost_nlopt_shared, whose shape is fixed
 * by NLopt's `nlopt_func` (they return HUGE_VAL).
 *
 * Conventions
 *   m        number of polynomial segments (= #waypoints - 1), m >= 2
 *   n        free variables per trajectory = 9 (m - 1)
 *   x, grad  n values per trajectory, axis-major: x[i + axis*(3m-3)]
 *            (src/grad_traj_optimizer.cpp:182-187, :428-432)
 *   Df       3 x 6 per trajectory, row-major: per axis
 *            [p_start, v_start, a_start, p_end, v_end, a_end]
 *            (src/qp_generator.cpp:407-431)
 *   T        segment times, m per trajectory (src/grad_traj_optimizer.cpp:73-81)
 *   dist     voxel distance field, index x*ny*nz + y*nz + z
 *            (src/sdf_map.cpp:172-173)
 *
 * One gtop_ctx per host thread / HIP stream; a context is not thread-safe
 * (neither is the reference object it replaces: it mutates iter_num,
 * total_time and the cost curve on every call,
 * src/grad_traj_optimizer.cpp:284,436,439-447).
 */
#ifndef GTOP_H_
#define GTOP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gtop_ctx gtop_ctx;

typedef enum {
  GTOP_OK = 0,
  GTOP_ERR_INVALID = 1,   /* bad argument (NULL, m < 2, size mismatch ...) */
  GTOP_ERR_HIP = 2,       /* a HIP runtime call failed; see gtop_last_error */
  GTOP_ERR_NO_DEVICE = 3, /* no gfx950 device visible */
  GTOP_ERR_STATE = 4,     /* call order: SDF / problem / params not set */
  GTOP_ERR_INTERNAL = 5   /* a C++ exception (e.g. std::bad_alloc) was caught at this
                             boundary; see gtop_last_error.  The object stays usable. */
} gtop_status;

typedef enum { GTOP_F64 = 0, GTOP_F32 = 1 } gtop_dtype;

/* The ROS parameters the callback reads (ctor,
 * src/grad_traj_optimizer.cpp:5-32) plus `step` (:132, :413-415).
 * enable_dyn switches on the velocity/acceleration penalty block that is
 * commented out in the reference (:383-407); 0 = behave as shipped. */
typedef struct {
  double ws, wc;           /* w_smooth, w_collision  */
  double alpha, r, d0;     /* distance penalty       */
  double alpha_v, r_v, v0; /* velocity penalty       */
  double alpha_a, r_a, a0; /* acceleration penalty   */
  int32_t step;            /* OPT_INITIAL_TRY 0 / OPT_FIRST_STEP 1 / OPT_SECOND_STEP 2 */
  int32_t enable_dyn;
} gtop_params;

/* ---- lifetime ------------------------------------------------------- */

/* Replaces GradTrajOptimizer::GradTrajOptimizer()
 * (src/grad_traj_optimizer.cpp:3-33).  `device` is the HIP device ordinal.
 * Fails with GTOP_ERR_NO_DEVICE when no GPU is present: there is no CPU
 * fallback behind this ABI. */
int gtop_create(gtop_ctx **out, int device);
int gtop_destroy(gtop_ctx *ctx);
/* Text of the last error on this context ("" if none); with ctx == NULL,
 * the text of the calling thread's last failed gtop_create. */
const char *gtop_last_error(const gtop_ctx *ctx);
/* Library/ABI version, for the loader to check (2 since round 4: the windowed map
 * update, gtop_set_field_precisions, gtop_device_clock_*, gtop_group_gather_note,
 * GTOP_ERR_INTERNAL; 3: the signed field, gtop_set_field_sign / gtop_get_field_sign /
 * gtop_group_set_field_sign; 4: the moving-obstacle cost, gtop_set_moving_cost /
 * gtop_get_moving_cost / gtop_set_start_times / gtop_set_start_times_device; 5: the
 * trajectory report and selection, gtop_validate_trajectories_device /
 * gtop_select_best_device / gtop_validate_batch; 6: the gradient mode,
 * gtop_set_gradient_mode / gtop_get_gradient_mode / gtop_group_set_gradient_mode;
 * 7: the polynomial box list, gtop_set_moving_box_polynomials /
 * gtop_get_moving_box_kind / gtop_box_polynomial_centres; 8: the minimum-jerk
 * start point, gtop_min_jerk_start_device / gtop_min_jerk_start; 9: the
 * per-segment report and segment-time reallocation,
 * gtop_validate_segments[_device] / gtop_reallocate_times[_device]; 10: the
 * continuous-time clearance certificate, gtop_certify_trajectories_device /
 * gtop_certify_batch / gtop_select_best_certified_device; 11: the certificate
 * against the moving boxes, gtop_certify_moving_device / gtop_certify_moving_batch;
 * 12: waypoint insertion, gtop_insert_waypoints_device / gtop_insert_waypoints;
 * nothing of an earlier version changed meaning). */
int gtop_abi_version(void);

/* ---- configuration -------------------------------------------------- */

/* Replaces the 21 ros::param::get calls of the ctor
 * (src/grad_traj_optimizer.cpp:5-32) and `this->step = step` (:132). */
int gtop_set_params(gtop_ctx *ctx, const gtop_params *p);

/* Replaces GradTrajOptimizer::initSDFMap + the distance_buffer that
 * updateSDFMap leaves behind (src/grad_traj_optimizer.cpp:112-126,
 * src/sdf_map.cpp:3-24).  `dist_host` holds nx*ny*nz doubles; it is uploaded
 * to HBM; the corner records every lookup reads (csrc/gtop_records.hip: the
 * 8 corners of a cell as 64 contiguous bytes, border clamps applied, 4x the
 * field's bytes) are derived from it on the device, fp32 ones at the first
 * fp32 use.
 * `map_size` may be NULL (then max_range = origin + grid*res); when given,
 * max_range = origin + map_size as src/sdf_map.cpp:12 has it.
 * Requires nx, ny, nz >= 2 and nx*ny*nz < 2^31. */
int gtop_set_sdf(gtop_ctx *ctx, const double *dist_host, int nx, int ny, int nz,
                 const double origin[3], const double *map_size,
                 double resolution);

/* Same, from a distance field already resident in HBM (dtype says which; the
 * caller has synchronised whatever wrote it).  The buffer is borrowed as the
 * boundary copy — gtop_get_sdf and the coarse voxel query read it in place, so
 * it must outlive its use — and the gather-friendly corner records the lookups
 * read (csrc/gtop_records.hip) are derived from it AT THIS CALL: after writing
 * to the buffer, call again.  A GTOP_F64 field serves evaluations of both
 * precisions, a GTOP_F32 field fp32 evaluations only. */
int gtop_set_sdf_device(gtop_ctx *ctx, int dtype, const void *dist_dev, int nx,
                        int ny, int nz, const double origin[3],
                        const double *map_size, double resolution);

/* Replaces GradTrajOptimizer::updateSDFMap (src/grad_traj_optimizer.cpp:117-126
 * -> src/sdf_map.cpp:26-53, :80-99, :310-368): reset, mark the voxel under
 * each of the `npts` obstacle points (xyz triples), rebuild the Euclidean
 * distance field on the device and keep it resident.  Call after an SDF
 * geometry has been set with gtop_init_sdf_map. */
int gtop_init_sdf_map(gtop_ctx *ctx, const double map_size[3],
                      const double origin[3], double resolution);
int gtop_update_sdf_map(gtop_ctx *ctx, const double *obstacle_pts, int npts);
/* The same with the obstacle points (npts x 3 doubles, xyz-contiguous) already in
 * HBM: launches on `hip_stream` and returns without synchronising — the build is
 * five kernels, 0.08 ms for a 200^3 map, against 0.6 ms of PCIe for the points of
 * the host form.  The corner records of BOTH precisions are rebuilt behind the
 * sweeps on the same stream, so the call can be captured into a hipGraph and
 * replayed with fp64 or fp32 evaluations behind it. */
int gtop_update_sdf_map_device(gtop_ctx *ctx, const void *d_obstacle_pts, int npts, void *hip_stream);
/* The reference's LOCAL map update — what compare2.cpp:147-152 does per sensor frame:
 *   sdf_map.resetBuffer(min_pos, max_pos)     src/sdf_map.cpp:28-53
 *   sdf_map.setOccupancy(p) for every point   :80-99
 *   [setUpdateRange(min_pos, max_pos)]        :244-264
 *   sdf_map.updateESDF3d()                    :310-368, its loops over min_vec .. max_vec
 * with its semantics: the box is clamped to the map and turned into voxel indices as
 * the reference does (posToIndex(min_pos) .. posToIndex(max_pos - res/2)); inside
 * it occupancy is cleared and distances reset to 10000; the points are marked
 * wherever in the map they fall; the three sweeps run over the box only and see
 * only the box's part of every line (an obstacle outside casts no distance into
 * it); distances outside the box keep their values, inside they become
 * min(res*sqrt(val), 10000).  Only the corner records of the box are rebuilt, so
 * the cost follows the box, not the map.  A box that covers the whole map takes
 * the whole-grid builder (same results).  Occupancy persists between calls, as in
 * the reference.  The _device form takes the points in HBM and only enqueues;
 * the first window update after gtop_init_sdf_map allocates scratch for any
 * window of that map (make it outside a stream capture), later ones allocate
 * nothing and can be captured. */
int gtop_update_sdf_map_window(gtop_ctx *ctx, const double min_pos[3], const double max_pos[3],
                               const double *obstacle_pts, int npts);
int gtop_update_sdf_map_window_device(gtop_ctx *ctx, const double min_pos[3], const double max_pos[3],
                                      const void *d_obstacle_pts, int npts, void *hip_stream);
/* Copy the resident fp64 distance field back to the host (nx*ny*nz doubles). */
int gtop_get_sdf(gtop_ctx *ctx, double *dist_host, int grid_out[3]);

/* ---- signed field (not in the reference) ----------------------------- */
/* The field above is unsigned, as the reference's updateESDF3d
 * (src/sdf_map.cpp:310-368): every occupied voxel holds 0, so inside a thick
 * obstacle the lookup is a flat 0 with zero gradient and nothing pushes a
 * trajectory out sideways.  signed_mode = 1 makes the map builds produce a
 * SIGNED field instead.  With B the voxel box being built (the whole grid for
 * gtop_update_sdf_map*, the window for gtop_update_sdf_map_window*, taken alone
 * as always):
 *   free voxel (occupancy 0)  min(res*sqrt(n+), 10000), as unsigned; n+ = squared
 *                             voxel distance to the nearest occupied voxel of B
 *   occupied voxel            max(-D, res - res*sqrt(n-)) in fp64, each step
 *                             rounded (product, difference, max); n- = squared
 *                             voxel distance to the nearest FREE voxel of B;
 *                             -D when B holds no free voxel
 * D = max_depth, 0 meaning 10000 (the mirror of the reference's cap).  An
 * occupied voxel with a free face-neighbour gets exactly 0, the unsigned value:
 * the two fields differ only at occupied voxels without a free 6-neighbour in B,
 * and the signed one is continuous across the surface (distance + res inside).
 * Mode 0 (unsigned) is the default; max_depth must be finite and >= 0
 * (GTOP_ERR_INVALID otherwise).  The setting takes effect at the next WHOLE-MAP
 * build (gtop_update_sdf_map*, gtop_init_sdf_map — whose all-free field is the
 * same in both modes — or an upload); it does not rebuild the resident field.
 * A windowed update while the setting differs from the resident field's
 * (mode, or depth in signed mode) fails with GTOP_ERR_STATE and changes nothing.
 * gtop_get_field_sign reports the RESIDENT field's mode and max_depth (as given);
 * after gtop_set_sdf* that is the mode in force at the upload — the library
 * cannot tell what uploaded values mean.
 * Everything that reads the field (evaluations, the optimizer, the EDT queries)
 * takes negative values as they are.  One limit: the collision penalty
 * alpha*exp((d0 - d)/r) overflows once (d0 - d)/r passes about 88.7 in fp32
 * (GTOP_F32 evaluations, gtop_set_optimizer_precision(GTOP_F32)) and about 709
 * in fp64.  max_depth is the control: keep max_depth <= 80*r - d0 for fp32 use.
 * With the default D = 10000 a box without any free voxel holds -10000 and the
 * penalty there is inf even in fp64.
 * (Those thresholds are the COST's, which carries the exponential once.  The
 * reference's collision gradient carries it squared — see the gradient mode below —
 * and overflows at half the exponent; under GTOP_GRADIENT_CONSISTENT the gradient
 * carries it once and the thresholds above hold for it too.) */
int gtop_set_field_sign(gtop_ctx *ctx, int signed_mode, double max_depth);
int gtop_get_field_sign(const gtop_ctx *ctx, int *signed_mode, double *max_depth);

/* Replaces the problem state setPath/setKinoPath leave in the object
 * (segment_time, Df; L and R follow from segment_time and are formed on the
 * device: src/grad_traj_optimizer.cpp:67-110, src/qp_generator.cpp:357-405).
 * B trajectories of m segments each; time_stride = m (per-trajectory times)
 * or 0 (one shared time vector).  Host pointers; uploaded to HBM. */
int gtop_set_problem(gtop_ctx *ctx, int B, int m, const double *segment_time,
                     int time_stride, const double *Df);

/* Replaces GradTrajOptimizer::setPath for B waypoint lists at once
 * (src/grad_traj_optimizer.cpp:67-110): segment times (:73-81: length/mean_v,
 * + init_time on the first segment only), Df and the straight-line initial Dp
 * (src/qp_generator.cpp:199-221, :407-451), computed on the device.
 * waypoints: B x (m+1) x 3.  gtop_set_paths makes the result the context's
 * problem (as gtop_set_problem would) and returns the start point x0 (B*n, may
 * be NULL); gtop_setup_paths_device writes device buffers and touches no state.
 * gtop_get_problem reads segment_time (B*m, or m when shared) and Df (B*18) back.
 * gtop_set_paths rejects coincident consecutive waypoints (a segment time of 0:
 * GTOP_ERR_INVALID, the rule gtop_set_problem applies); gtop_setup_paths_device
 * cannot look at device memory without a synchronisation and behaves as the
 * reference does there (T_s = 0, a singular A_s: NaN cost and gradient). */
int gtop_set_paths(gtop_ctx *ctx, int B, int m, const double *waypoints,
                   double mean_v, double init_time, double *x0);
int gtop_setup_paths_device(gtop_ctx *ctx, int B, int m, const void *d_waypoints,
                            double mean_v, double init_time, void *d_T,
                            void *d_Df, void *d_x0, void *hip_stream);
int gtop_get_problem(gtop_ctx *ctx, double *segment_time, double *Df);

/* ---- the minimum-jerk start point -------------------------------------
 * The start point above is the reference's PolyQPGeneration(type = 2)
 * (src/qp_generator.cpp:317-345, :433-439): zero velocity and acceleration at
 * every interior waypoint, a stop-and-go trajectory.  This is the alternative of
 * the same function, type == 1 (:242-315), which setPath never selects
 * (src/grad_traj_optimizer.cpp:86): the waypoint positions stay fixed and the
 * interior (v_k, a_k), k = 1 .. m-1, become the minimiser of the smoothness term
 * the evaluations return, sum over the axes of d' R d (StackOptiDep, :357-403) —
 * generalised to any boundary velocity and acceleration (type == 1 has the end
 * pair at 0; Df carries all four).  R is never formed.  In the segment-local order
 * [p(0), p(T), v(0), v(T), a(0), a(T)] the jerk integral of one quintic segment of
 * duration T is d' M(T) d,
 *   M(1) = [  720 -720  360  360   60  -60 ]   M(T)(i,j) = M(1)(i,j) / T^(5 - o_i - o_j),
 *          [ -720  720 -360 -360  -60   60 ]   o = 0 for a position row / column,
 *          [  360 -360  192  168   36  -24 ]   1 for a velocity, 2 for an acceleration
 *          [  360 -360  168  192   24  -36 ]
 *          [   60  -60   36   24    9   -3 ]
 *          [  -60   60  -24  -36   -3    9 ]
 * and the normal equations are block tridiagonal with 2 x 2 blocks, symmetric
 * positive definite, one matrix for the three axes.  With u_k = (v_k, a_k),
 * Ta = T[k-1], Tb = T[k]:
 *   D_k = [ 192/Ta^3 + 192/Tb^3   -36/Ta^2 + 36/Tb^2 ]    U_k = [ 168/Tb^3  -24/Tb^2 ]
 *         [ -36/Ta^2 + 36/Tb^2      9/Ta   +  9/Tb   ]          [  24/Tb^2   -3/Tb   ]
 *   D_k u_k + U_{k-1}' u_{k-1} + U_k u_{k+1} = -g_k
 *   g_k(v) = 360 (p_{k-1} - p_k)/Ta^4 + 360 (p_k - p_{k+1})/Tb^4
 *   g_k(a) = -60 (p_{k-1} - p_k)/Ta^3 +  60 (p_k - p_{k+1})/Tb^3
 * u_0 is the start pair of Df, u_m the end pair; both move to the right-hand
 * side; m = 2 is a single 2 x 2 system.  Solved by block elimination, O(m) per
 * trajectory, one lane each (csrc/gtop_minjerk.hip).
 *
 * x: B*n, the free variables in the usual layout x[i + axis*(3m-3)],
 * i = 3(k-1) + {0: p, 1: v, 2: a}.  The call reads the position entries, Df and T,
 * OVERWRITES the velocity and acceleration entries with the minimiser and writes
 * nothing else — so it composes with everything that makes an x: the output of
 * gtop_setup_paths_device / gtop_set_paths (which stay what they are), or a
 * caller's own waypoints with gtop_set_problem.  The straight-line start and the
 * minimum-jerk start of one waypoint list are two natural candidates of one batch
 * for gtop_optimize_device_ex, gtop_validate_trajectories_device and
 * gtop_select_best_device.
 * The device form only enqueues on hip_stream: no allocation, no synchronisation,
 * capturable; it needs no distance field and no parameters.  fp64 only.
 * time_stride is m or 0; 2 <= m <= 227, the evaluation's own limit; B = 0 launches
 * nothing and returns GTOP_OK.  GTOP_ERR_INVALID, nothing launched: a NULL
 * pointer, B < 0, m out of range, another time_stride; in the host form B < 1 or B
 * above the problem's batch.  The host form serves the first B rows of the
 * context's problem (GTOP_ERR_STATE when none is set) and stages through the
 * context's buffers.
 * The device form cannot inspect T, as gtop_setup_paths_device cannot: a
 * trajectory with a zero segment time gets non-finite v, a in its own row — every
 * loop is bounded by m, nothing else is touched.
 * A row's result depends on that row's inputs only: not on its index, on B, or on
 * whether the times are shared.  Two rows with equal inputs get equal bits.
 * The minimiser knows no bounds: a velocity beyond +-vos (an acceleration beyond
 * +-aos) is legal input to the optimizer, which clamps its start point into the
 * box before the first evaluation (csrc/gtop_mma.hip, csrc/mma.hpp). */
int gtop_min_jerk_start_device(gtop_ctx *ctx, int B, int m, void *d_x, const void *d_Df,
                               const void *d_T, int time_stride, void *hip_stream);
int gtop_min_jerk_start(gtop_ctx *ctx, int B, double *x);

/* ---- evaluation ----------------------------------------------------- */

/* Batched form of GradTrajOptimizer::costFunc / getCostAndGradient
 * (src/grad_traj_optimizer.cpp:554-562, :281-448) for the problem set by
 * gtop_set_problem: x, grad are B*n host doubles, cost B host doubles.
 * fp64 on the device; includes the PCIe copies.  Small batches (up to 16384
 * outputs: the NLopt callback, a rendezvous generation) are read from and written to pinned host
 * memory by the kernel itself, and the call returns when the last output has
 * landed there (each is stored once; the slots are preset to a NaN pattern no
 * evaluation produces).  GTOP_POLL_COMPLETION=0 in the environment at
 * gtop_create, or 2 ms without completion, wait through the stream instead. */
int gtop_eval_batch(gtop_ctx *ctx, int B, const double *x, double *cost,
                    double *grad);

/* Exactly NLopt's `nlopt_func` (what nlopt::opt::set_min_objective's
 * trampoline calls; src/grad_traj_optimizer.cpp:140, :554-562): evaluates
 * trajectory 0 of the current problem.  `grad` may be NULL (the reference
 * always fills it, :426; NLopt passes NULL to derivative-free algorithms).
 * Returns the cost; on error returns HUGE_VAL and records gtop_last_error.
 * Also keeps iter_num / total_time / the best-so-far cost curve
 * (:284, :436, :439-447) — read them with gtop_get_stats/gtop_get_cost_curve. */
double gtop_cost_nlopt(unsigned n, const double *x, double *grad, void *ctx);

/* ---- rendezvous: N serial callers share one launch ------------------- */
/* The reference runs one NLopt instance per problem and each calls the callback
 * serially (src/grad_traj_optimizer.cpp:137-195, :554-562).  One trajectory per
 * launch is launch-bound on a GPU, so this layer lets N host threads — each
 * running its own serial optimizer on its own trajectory — meet in ONE
 * gtop_eval_batch of the shared context:
 *   gtop_set_problem(ctx, N, m, ...)           the N problems, row i = caller i
 *   gtop_rendezvous_create(&r, ctx, N, m)
 *   thread i:  nlopt_set_min_objective(opt_i, gtop_cost_nlopt_shared,
 *                                      gtop_rendezvous_get_slot(r, i));
 *              nlopt_optimize(opt_i, ...);  gtop_rendezvous_leave(slot_i);
 * gtop_cost_nlopt_shared has exactly NLopt's nlopt_func shape.  It blocks until
 * every slot that has not left has arrived; the last arriver runs the batch;
 * each caller gets the cost and gradient of its own row — bit for bit what
 * gtop_eval_batch gives that row.  A caller MUST call gtop_rendezvous_leave
 * when its optimizer returns, or the others wait for it: for ever by default,
 * or — after gtop_rendezvous_set_timeout(r, seconds) — until one of them has
 * waited that long FOR A CALLER THAT HAS NOT ARRIVED, which breaks the
 * rendezvous for everybody (every call, pending or later, returns HUGE_VAL).
 * Time spent waiting for the elected caller's launch (everybody has arrived:
 * a module load on the first call, a large batch) never counts against the
 * timeout.  gtop_rendezvous_abort breaks it at once, from any thread (an
 * error path that cannot make every caller leave).  After a break no slot
 * counts as waiting: gtop_rendezvous_leave on it returns GTOP_OK.
 * gtop_rendezvous_destroy breaks the rendezvous, waits until no thread is
 * inside a call on it (a launch in flight uses its buffers) and frees it.
 * gtop_rendezvous_leave on a slot whose caller is inside the call right now
 * (i.e. from another thread) is refused with GTOP_ERR_STATE.  Returns
 * HUGE_VAL on misuse (wrong n, a slot that has left) or when the evaluation
 * failed (gtop_last_error(ctx)).  The context must not be used by anything
 * else while callers are inside. */
typedef struct gtop_rendezvous gtop_rendezvous;
typedef struct gtop_rendezvous_slot gtop_rendezvous_slot;
int gtop_rendezvous_create(gtop_rendezvous **out, gtop_ctx *ctx, int n_slots, int m);
int gtop_rendezvous_destroy(gtop_rendezvous *r);
gtop_rendezvous_slot *gtop_rendezvous_get_slot(gtop_rendezvous *r, int i);
double gtop_cost_nlopt_shared(unsigned n, const double *x, double *grad, void *slot);
int gtop_rendezvous_leave(gtop_rendezvous_slot *slot);
int gtop_rendezvous_set_timeout(gtop_rendezvous *r, double seconds);   /* 0 = wait for ever (default) */
int gtop_rendezvous_abort(gtop_rendezvous *r);
/* launches so far, seconds spent inside them, callbacks served (all slots) */
int gtop_rendezvous_stats(gtop_rendezvous *r, int64_t *launches, double *launch_seconds,
                          int64_t *callbacks);

/* Device-resident form: every pointer is a HIP device pointer of `dtype`
 * elements; launches on `hip_stream` (a hipStream_t, NULL = default stream)
 * and returns without synchronising.  Does not touch the problem set by
 * gtop_set_problem.  d_T: B*m (time_stride = m) or m (time_stride = 0). */
int gtop_eval_device(gtop_ctx *ctx, int dtype, int B, int m, const void *d_x,
                     const void *d_Df, const void *d_T, int time_stride,
                     void *d_cost, void *d_grad, void *hip_stream);

/* ---- one batch over several GPUs from one process -------- */
/* Nothing in the reference is multi-device (one NLopt instance per problem,
 * src/grad_traj_optimizer.cpp:137-195); the batched callback shards trivially:
 * trajectories are independent and the field is read-only.  A group owns one
 * gtop_ctx and one HIP stream per listed device (a device may be listed more
 * than once), keeps the distance field REPLICATED (gtop_group_init_sdf_map /
 * _update_sdf_map / _set_sdf build it on every device), and cuts the batch of
 * gtop_group_set_problem into contiguous slices of ceil(B / n) rows
 * (gtop_group_shard).  Every slice is launched on its own device before any is
 * waited for; there is no reduction, so results are bit-identical to the
 * unsharded evaluation.
 *   gtop_group_eval_batch        host buffers in and out (fp64), like
 *                                gtop_eval_batch
 *   gtop_group_upload_x + gtop_group_eval_resident(gather, synchronize)
 *                                everything resident; gather = 1 all-gathers
 *                                the costs, 2 also the gradients, so that EVERY
 *                                device holds the whole batch's results
 *                                (gtop_group_read_gathered copies one device's
 *                                set to the host; gtop_group_device_buffers
 *                                hands out the device pointers and the stream)
 *   gtop_group_optimize_batch_ex the batched optimizer, one launch per device
 * The all-gather is RCCL's (ncclAllGather in a group call, one communicator per
 * device, librccl.so loaded on first use) when all listed devices differ, peer
 * copies otherwise — gtop_group_gather_backend says which ("rccl" / "copy");
 * GTOP_GROUP_GATHER=copy|rccl in the environment at gtop_group_create forces
 * one.  One host thread at a time per group. */
typedef struct gtop_group gtop_group;
int gtop_group_create(gtop_group **out, const int *devices, int n_devices);
int gtop_group_destroy(gtop_group *g);
int gtop_group_size(const gtop_group *g);
gtop_ctx *gtop_group_context(gtop_group *g, int member);
/* Text of the group's last error; with g == NULL, the text of the calling
 * thread's last failed gtop_group_create (which member, and why). */
const char *gtop_group_last_error(const gtop_group *g);
const char *gtop_group_gather_backend(const gtop_group *g);
/* The backend and the reason for it in words, e.g. "copy: peer copies, because
 * librccl.so not found: ..." — a fallback from RCCL to copies is never silent. */
const char *gtop_group_gather_note(const gtop_group *g);
int gtop_group_set_params(gtop_group *g, const gtop_params *p);
/* gtop_set_gradient_mode on every member */
int gtop_group_set_gradient_mode(gtop_group *g, int mode);
/* gtop_set_field_sign on every member */
int gtop_group_set_field_sign(gtop_group *g, int signed_mode, double max_depth);
int gtop_group_init_sdf_map(gtop_group *g, const double map_size[3], const double origin[3], double resolution);
int gtop_group_update_sdf_map(gtop_group *g, const double *pts, int npts);
int gtop_group_update_sdf_map_window(gtop_group *g, const double min_pos[3], const double max_pos[3], const double *pts,
                                     int npts);   /* gtop_update_sdf_map_window on every member */
int gtop_group_set_sdf(gtop_group *g, const double *dist_host, int nx, int ny, int nz, const double origin[3],
                       const double *map_size, double resolution);
int gtop_group_set_problem(gtop_group *g, int B, int m, const double *segment_time, int time_stride,
                           const double *Df);
int gtop_group_shard(const gtop_group *g, int member, int *first, int *count);
int gtop_group_eval_batch(gtop_group *g, int B, const double *x, double *cost, double *grad);
int gtop_group_upload_x(gtop_group *g, int B, const double *x);
int gtop_group_eval_resident(gtop_group *g, int gather, int synchronize);
int gtop_group_synchronize(gtop_group *g);
/* the gathered results as member `member` holds them: cost B, grad B*n host doubles (either may be NULL) */
int gtop_group_read_gathered(gtop_group *g, int member, double *cost, double *grad);
/* member's slice buffers (ceil(B/n) rows each), its gathered buffers (n*ceil(B/n) rows) and its hipStream_t */
int gtop_group_device_buffers(gtop_group *g, int member, void **d_x, void **d_cost, void **d_grad,
                              void **d_cost_all, void **d_grad_all, void **hip_stream);

/* ---- batched optimizer driver -------------------- */

/* Box bounds of GradTrajOptimizer::optimizeTrajectory
 * (src/grad_traj_optimizer.cpp:151-179): waypoint positions +-bos, velocities
 * +-vos, accelerations +-aos.  path: B x (m+1) x 3 waypoints; lb/ub: B x n.
 * Pure host helper (no context, no device). */
int gtop_default_bounds(int B, int m, const double *path, double bos,
                        double vos, double aos, double *lb, double *ub);

/* B independent bound-constrained CCSA-MMA solves on the device: what B calls
 * of nlopt::opt::optimize with algorithm 24 (LD_MMA) do one after another in
 * the reference (src/grad_traj_optimizer.cpp:137-195), here as max_evals
 * rounds of {cost/gradient, optimizer update} per trajectory — by default all
 * of them inside one kernel launch (gtop_set_optimizer_fusion).  The stop rule
 * is an evaluation count (the reference stops on wall-clock
 * maxtime, :144-148, which is not reproducible).  x: in = start point
 * (:182-187), out = best point found; min_cost: its cost.  fp64.
 * gtop_optimize_batch uses the problem of gtop_set_problem and host buffers;
 * gtop_optimize_device takes device pointers and only enqueues work.
 * What lb / ub may hold, per variable (lb <= ub; every entry point below, all three
 * launch forms and csrc/mma.hpp alike):
 *  - -inf as lb and/or +inf as ub: the side is open.  A variable with an infinite
 *    bound on either side starts with asymptote width sigma = 1 (a bounded one with
 *    (ub - lb) / 2) and its sigma is never clamped to [0.01, 10] (ub - lb).
 *  - lb == ub: the variable never moves and is returned as given (bit for bit); when
 *    every variable is fixed the run costs two evaluations under a tolerance (FTOL
 *    under ftol_rel, XTOL under xtol_rel or both) and max_evals without one.
 *  - a start point outside the box is clamped into it before the first evaluation
 *    (NLopt refuses it): the run is the run from the clamped point, bit for bit.
 * The returned point lies inside [lb, ub] exactly.  Up to 118 segments (one
 * wavefront's LDS with the optimizer's state); more: GTOP_ERR_INVALID, x untouched. */
int gtop_optimize_batch(gtop_ctx *ctx, int B, double *x, const double *lb,
                        const double *ub, int max_evals, double *min_cost);
int gtop_optimize_device(gtop_ctx *ctx, int B, int m, void *d_x,
                         const void *d_Df, const void *d_T, int time_stride,
                         const void *d_lb, const void *d_ub, int max_evals,
                         void *d_min_cost, void *hip_stream);

/* The same with NLopt's other stop rules (nlopt::opt::set_ftol_rel / set_xtol_rel /
 * set_maxtime; the reference sets maxtime only, src/grad_traj_optimizer.cpp:144-148;
 * host twin csrc/mma.hpp:35-39, :127-137).  A trajectory stops by itself — inside
 * the one-launch loop — when, at the end of an outer MMA iteration,
 *   |f - f_prev| < ftol_rel (|f| + |f_prev|)/2, or
 *   |x_j - xprev_j| < xtol_rel (|x_j| + |xprev_j|)/2 for every j,
 * or, after at least one evaluation, when `maxtime` seconds of device wall
 * clock have passed since the launch (whole-loop-in-one-launch mode only; not
 * reproducible, as in the reference).  0 switches a rule off.  A stopped
 * trajectory costs no further evaluations.  nevals[b]: evaluations trajectory b
 * used; code[b]: 3 FTOL, 4 XTOL, 5 MAXEVAL, 6 MAXTIME (nlopt_result values).
 * nevals / code may be NULL (device pointers in the _device form). */
typedef struct {
  int32_t max_evals;       /* >= 1 */
  double ftol_rel, xtol_rel;
  double maxtime;          /* seconds */
} gtop_stop;
int gtop_optimize_batch_ex(gtop_ctx *ctx, int B, double *x, const double *lb,
                           const double *ub, const gtop_stop *stop, double *min_cost,
                           int32_t *nevals, int32_t *code);
int gtop_optimize_device_ex(gtop_ctx *ctx, int B, int m, void *d_x, const void *d_Df,
                            const void *d_T, int time_stride, const void *d_lb,
                            const void *d_ub, const gtop_stop *stop, void *d_min_cost,
                            int32_t *d_nevals, int32_t *d_code, void *hip_stream);
/* the same over a group's devices (B = the batch of gtop_group_set_problem): one launch per device */
int gtop_group_optimize_batch_ex(gtop_group *g, int B, double *x, const double *lb, const double *ub,
                                 const gtop_stop *stop, double *min_cost, int32_t *nevals, int32_t *code);

/* ---- post-processing ------------------------------ */

/* Batched GradTrajOptimizer::getCoefficient / getCoefficientFromDerivative
 * (src/grad_traj_optimizer.cpp:245-279): coeff is B x m x 18, row s =
 * [cx0..5 | cy0..5 | cz0..5], ascending powers. */
int gtop_coefficients_device(gtop_ctx *ctx, int B, int m, const void *d_x,
                             const void *d_Df, const void *d_T, int time_stride,
                             void *d_coeff, void *hip_stream);

/* The evaluation src/opti_node.cpp:135-142 runs on the optimised polynomials
 * through PolynomialTraj (include/grad_traj_optimization/polynomial_traj.hpp):
 * stats is B x GTOP_TRAJ_STATS doubles per trajectory =
 *   [getTimeSum, getLength (samples every dt_sample; the reference uses 0.01),
 *    getJerk, mean_v, max_v (getMeanAndMaxVel), mean_a, max_a
 *    (getMeanAndMaxAcc), getAccCost, number of getTraj samples].
 * The functions' quirks are kept (mean/max velocity and acceleration are
 * evaluated at each segment's END time, weighted by its sample count, as
 * :158-159 / :189-190 compute them). */
#define GTOP_TRAJ_STATS 9
int gtop_eval_trajectories_device(gtop_ctx *ctx, int B, int m, const void *d_coeff,
                                  const void *d_T, int time_stride,
                                  double dt_sample, void *d_stats,
                                  void *hip_stream);
/* The same, also returning the points PolynomialTraj::getTraj produces
 * (polynomial_traj.hpp:69-78: one every dt_sample, the sample time ACCUMULATED
 * as the reference does, while eval_t <= time_sum): samples is
 * B x max_samples x 3; trajectory b has stats[b][8] points, of which the first
 * min(stats[b][8], max_samples) are stored.  src/opti_node.cpp:108-120 publishes
 * exactly these.  max_samples = 0 asks for the statistics alone (d_samples is
 * not read then); with max_samples > 0 a NULL d_samples is refused. */
int gtop_sample_trajectories_device(gtop_ctx *ctx, int B, int m, const void *d_coeff,
                                    const void *d_T, int time_stride, double dt_sample,
                                    void *d_stats, void *d_samples, int max_samples,
                                    void *hip_stream);
/* Host-buffer form for the context's problem: coefficients (may be NULL) and
 * stats (may be NULL) of the first B trajectories at free variables x. */
int gtop_trajectory_stats(gtop_ctx *ctx, int B, const double *x, double dt_sample,
                          double *coeff, double *stats);
int gtop_trajectory_samples(gtop_ctx *ctx, int B, const double *x, double dt_sample,
                            double *coeff, double *stats, double *samples, int max_samples);

/* Distance queries against the static field plus moving obstacles:
 * EDTEnvironment::evaluateEDTWithGrad / distToBox / minDistToAllBox
 * (src/edt_environment.cpp:26-122).  Boxes are {p0, vel, scale} (nbox x 3 each,
 * host arrays, copied): centre p0 + vel*t (obj_predictor.h:57-66), extent
 * +-scale/2.  A query is (pos[3], time): trilinear value and gradient over
 * the 8 corner voxels with corner value min(static, nearest box at `time`);
 * time < 0 = static only, and then equal to getDistWithGradTrilinear
 * (src/sdf_map.cpp:185-242).  Outside the map: dist = -1, grad = 0.  fp64,
 * needs the fp64 field.  pos is N x 3, grad is N x 3. */
int gtop_set_moving_boxes(gtop_ctx *ctx, int nbox, const double *p0,
                          const double *vel, const double *scale);
int gtop_edt_query_device(gtop_ctx *ctx, int N, const void *d_pos,
                          const void *d_time, void *d_dist, void *d_grad,
                          void *hip_stream);
int gtop_edt_query(gtop_ctx *ctx, int N, const double *pos, const double *time,
                   double *dist, double *grad);
/* EDTEnvironment::evaluateCoarseEDT (src/edt_environment.cpp:124-136): no
 * interpolation and no gradient — the distance stored in the voxel that holds
 * pos (SDFMap::getDistance(pos), src/sdf_map.cpp:155-164; -1 outside the map),
 * and for time >= 0 its minimum with the distance from pos to the nearest box. */
int gtop_edt_coarse_query_device(gtop_ctx *ctx, int N, const void *d_pos,
                                 const void *d_time, void *d_dist, void *hip_stream);
int gtop_edt_coarse_query(gtop_ctx *ctx, int N, const double *pos, const double *time,
                          double *dist);

/* ---- moving obstacles on polynomial predictions ------------------------
 * The other form of the ONE box list a context holds: each box's centre is a
 * quintic per axis on a validity interval — the reference's PolynomialPrediction
 * (polys, t1, t2, evaluate(t); include/grad_traj_optimization/obj_predictor.h:26-55),
 * the call distToBox carries in a comment above the constant-velocity one
 * (src/edt_environment.cpp:28-29).  For a turning or braking obstacle, or a peer
 * flying its own committed quintic segment.
 *   coef:    nbox x 3 x 6, axis-major per box, ascending powers (polys[k](i))
 *   t_range: nbox x 2 = {t1, t2} per box, or NULL = unbounded
 *   scale:   nbox x 3, the extent, as for gtop_set_moving_boxes
 * Box b at time tau, axis k (fp64; every consumer — the queries, the report, the
 * cost — computes exactly this, bit for bit):
 *   tc  = fmin(fmax(tau, t1[b]), t2[b])                    (no clamp without t_range)
 *   c_k = fma(fma(fma(fma(fma(c5, tc, c4), tc, c3), tc, c2), tc, c1), tc, c0)
 *   faces c_k +- 0.5 * scale_k; from there on as for a constant-velocity box
 *   (distToBox, the skip of far boxes, the min with the static corner values).
 * Outside its interval a box STANDS where its prediction ends (an extrapolated
 * quintic leaves the map within a second, and a box that vanished would make the
 * unknown look safe); +-inf bounds are allowed and clamp nothing on their side.
 * The rule "tau < 0: static only" is taken on tau itself, before the clamp.
 * gtop_set_moving_boxes and gtop_set_moving_box_polynomials each REPLACE whatever
 * list was set before, of either kind; nbox = 0 clears the list under either call
 * (the kind reads GTOP_BOXES_CONST_VEL then).  GTOP_ERR_INVALID at the call, the
 * list in force unchanged: t1 > t2, a NaN bound, a non-finite coefficient, a
 * negative or non-finite scale.  A list of more than GTOP_MOVING_COST_MAX_BOXES
 * boxes is accepted: it serves the queries and the report, and an evaluation in
 * moving mode refuses it (GTOP_ERR_INVALID there), exactly as a constant-velocity
 * list of that length.
 * Every limit of the moving-obstacle cost below holds for this form too: fp64 only,
 * at most GTOP_MOVING_COST_MAX_BOXES boxes, not forwarded by gtop_group_*, the same
 * launch-geometry refusals.
 * Capture: the list's KIND selects the kernel, so it is a launch argument — a
 * captured evaluation, optimizer run, query or report replays with the kind it was
 * captured with, and changing the kind needs a re-capture (a replay across a change
 * of kind would read rows of the other layout as its own; memory-safe, values
 * meaningless).  Changing the VALUES within a kind is followed at replay for the
 * evaluations and optimizer runs, as before: they read the one buffer that never
 * moves.
 * gtop_box_polynomial_centres: the same arithmetic on the host, no context and no
 * device (like gtop_default_bounds) — centres is ntimes x nbox x 3; the same
 * checks (GTOP_ERR_INVALID; NULL pointers too). */
#define GTOP_BOXES_CONST_VEL 0
#define GTOP_BOXES_POLYNOMIAL 1
int gtop_set_moving_box_polynomials(gtop_ctx *ctx, int nbox, const double *coef,
                                    const double *t_range, const double *scale);
int gtop_get_moving_box_kind(const gtop_ctx *ctx, int *kind, int *nbox);
int gtop_box_polynomial_centres(int nbox, const double *coef, const double *t_range,
                                int ntimes, const double *times, double *centres);

/* ---- moving-obstacle cost (not in the reference's callback) ---------- */
/* Off (the default), every evaluation looks the collision samples up in the static
 * field, as the reference's callback does (src/grad_traj_optimizer.cpp:363).  On,
 * and with at least one box set (gtop_set_moving_boxes, or
 * gtop_set_moving_box_polynomials above), the lookup of every
 * collision sample is the time-aware one the queries above answer: for
 * trajectory b, segment s, sample i, with local time t and position exactly as
 * before (:353, :457-465),
 *     tau = ((t0[b] + T[b][0]) + ... + T[b][s-1]) + t        (fp64, left to right)
 *     (dist, grad) = evaluateEDTWithGrad(pos, tau)
 * — the 8 corner values min'ed with the distance from each corner voxel's centre
 * to the nearest box at tau, then the unchanged trilinear value and gradient; out
 * of the map dist = -1, grad = 0, boxes ignored; a sample with tau < 0 is static
 * only.  Everything downstream (:365-381) is unchanged; segment times are not
 * variables, so nothing is differentiated through tau.  The resident field's
 * values are taken as they are (a signed field works as for the queries).  A box
 * over a sample drives its distance to 0, never below: the penalty's exponent is
 * bounded by d0 / r as on an unsigned field, so the mode opens no overflow road
 * beyond the one the signed field documents.  Inside a box all 8 corners are 0
 * and the gradient vanishes, as in any unsigned field.
 *
 * Context state, so it reaches every fp64 road: gtop_eval_batch, gtop_cost_nlopt
 * (trajectory 0's start time), gtop_cost_nlopt_shared (row i's),
 * gtop_eval_device(GTOP_F64), gtop_optimize_batch[_ex], gtop_optimize_device[_ex]
 * in all three fusion modes, with or without enable_dyn.  The device forms still
 * only enqueue (no allocation, no synchronisation; capturable).  On with NO boxes:
 * the static kernels run, results bit-identical to off.
 * Limits:
 *  - fp64 only: a GTOP_F32 evaluation, or an optimizer run under
 *    gtop_set_optimizer_precision(GTOP_F32), with the mode on and boxes set is
 *    GTOP_ERR_STATE.
 *  - at most GTOP_MOVING_COST_MAX_BOXES boxes, each finite with scale >= 0 (the
 *    queries take any list); otherwise GTOP_ERR_INVALID at the evaluation.
 *  - launch geometry (gtop_set_launch_geometry): samples_per_lane 0 (auto) serves
 *    every length the static evaluation serves (2 .. 227 segments; the optimizer
 *    118) and every batch; 3 serves up to 6 segments, 6 every length; 10 and 30,
 *    and 3 with more than 6 segments, have no moving-term body: GTOP_ERR_INVALID
 *    at the evaluation (the optimizer, which ignores 10 and 30, runs its own rule).
 *  - the gtop_group_* entry points do not forward the mode; a member context can
 *    be configured through gtop_group_context.
 *
 * Start times t0 on the boxes' clock: count = 0 (or NULL) all zero (the default);
 * count = 1 one shared value; otherwise one per trajectory, and count must equal
 * the batch of the evaluation it is used with (for gtop_eval_batch, gtop_cost_nlopt
 * and gtop_optimize_batch[_ex], which run the first B rows of the problem set, the
 * problem's batch serves too) — a mismatch is GTOP_ERR_INVALID at the evaluation,
 * nothing launched.  Host values must be finite and >= 0 (GTOP_ERR_INVALID at the
 * call).  The device form borrows an fp64 device buffer: no copy, no
 * synchronisation, values not inspected — it is read by every launch, so a
 * captured launch follows what the buffer holds at replay, and a sample whose
 * tau < 0 is static only, as in the query. */
#define GTOP_MOVING_COST_MAX_BOXES 32
int gtop_set_moving_cost(gtop_ctx *ctx, int enable);
int gtop_get_moving_cost(const gtop_ctx *ctx, int *enable);
int gtop_set_start_times(gtop_ctx *ctx, int count, const double *t0_host);
int gtop_set_start_times_device(gtop_ctx *ctx, int count, const void *d_t0);

/* ---- gradient mode (not in the reference) --------------------------------- */
/* The gradient the evaluations return by default is the reference's callback line
 * by line, and that is not the gradient of the cost they return:
 *  - collision term (src/grad_traj_optimizer.cpp:376-381): gd*grad(k)*cd*vel_norm,
 *    where the derivative of cd(dist)*vel_norm*dt is gd*grad(k)*vel_norm — a spurious
 *    factor cd = alpha*exp((d0 - dist)/r), 10 at dist = d0 and above 40 at dist = 0
 *    with the shipped parameters;
 *  - the enable_dyn block (:383-407): cv, ca in the gradient are the values the cost
 *    loop left behind (the last axis's), there is no sign(v) / sign(a) factor, and
 *    the d|v|/dx term carries one axis's penalty instead of the sum.
 * GTOP_GRADIENT_REFERENCE (the default) keeps all of that: a drop-in reproduces the
 * reference's iterates.  GTOP_GRADIENT_CONSISTENT changes the GRADIENT only; for a
 * live sample (inside the loop bound of :353), axis k:
 *
 *   g_colli.row(k) += ( gd*grad(k)*vel_norm * T*Ldp
 *                       + cd*(vel(k)/vel_norm) * T*V*Ldp ) * dt
 *   and, where the enable_dyn block is active (enable_dyn != 0 and step == 2):
 *   S = sum_j (cv_j + ca_j)                                    over the three axes
 *   g_vel.row(k) += ( gv_k*sgn(vel(k))*vel_norm + S*vel(k)/vel_norm ) * T*V*Ldp * dt
 *   g_acc.row(k) += ( ga_k*sgn(acc(k))*vel_norm ) * T*V*V*Ldp * dt
 *   sgn(+-0) = 0: an axis with exactly zero velocity (the two idle axes of an
 *   axis-aligned path) gets no push.
 *
 * Everything else is as in reference mode: the cost, bit for bit; position,
 * velocity and acceleration through `float`; vel_norm = |v| + 1e-5, also in the
 * quotient; out of the map dist = -1 and grad := 0; + 1e-5 on every gradient entry;
 * |wc| < 1e-4 skips the sample loop (the two modes are then the same function);
 * ws = 0 at step 1; with the moving-obstacle cost on, dist and grad come from the
 * time-aware lookup; a signed field is taken as it is.
 * "Consistent" means: the derivative of the returned cost with the float round
 * trips treated as the identity, the field as differentiable inside a cell, and
 * d vel_norm / d v = v / vel_norm (the 1e-5 of vel_norm in the quotient biases one
 * term by 1e-5/|v|).  It matches finite differences of the cost at the 1e-6 level,
 * not to rounding.
 *
 * Context state, read when a call is made (a captured gtop_eval_device replays
 * with the mode it was captured with): gtop_eval_batch, gtop_cost_nlopt,
 * gtop_cost_nlopt_shared, gtop_eval_device of both precisions,
 * gtop_optimize_batch[_ex] and gtop_optimize_device[_ex] in all three fusion modes
 * and both optimizer precisions, moving-obstacle cost on or off, enable_dyn on or
 * off, every launch geometry and length those serve — no limit of its own.  The
 * device forms still only enqueue.  Other values of `mode`: GTOP_ERR_INVALID. */
#define GTOP_GRADIENT_REFERENCE 0  /* default: the reference's callback, as shipped */
#define GTOP_GRADIENT_CONSISTENT 1
int gtop_set_gradient_mode(gtop_ctx *ctx, int mode);
int gtop_get_gradient_mode(const gtop_ctx *ctx, int *mode);

/* ---- trajectory safety report and best-candidate selection -------------- */
/* (Not a PolynomialTraj method.)  Replaces what a caller assembled by hand after
 * an optimisation: gtop_sample_trajectories_device (24 B per sample to HBM), then
 * gtop_edt_query_device (32 B per sample back, a gradient nobody wanted), then a
 * host or torch reduction; and the max_v / max_a of GTOP_TRAJ_STATS, which keep
 * the reference's end-of-segment quirk (polynomial_traj.hpp:144-204) and are not
 * the maxima along the curve.  The semantics are those of the reference's planner
 * front end, which tests every expanded motion primitive this way
 * (src/kinodynamic_astar.cpp:178-213): a per-axis velocity limit (:180) and
 * evaluateCoarseEDT(pos, time) <= margin_ along the primitive (:207) — here at
 * the samples of PolynomialTraj::getTraj (polynomial_traj.hpp:69-78: eval_t
 * accumulated from 0 by dt_sample while eval_t <= time_sum; count, times and
 * positions are bit for bit those of gtop_sample_trajectories_device), with the
 * interpolating lookup of gtop_edt_query_device: a sample's distance is the
 * `dist` that query returns for (pos, tau), bit for bit, tau = t0[b] + eval_t
 * (one fp64 addition; t0 = the start times of gtop_set_start_times[_device],
 * same count rules) with use_boxes set, static only (tau = -1) otherwise; out of
 * the map it is -1.  Any number of boxes, as for the queries; a signed field is
 * used as it is.  use_boxes is independent of gtop_set_moving_cost: validation
 * is a query, not the cost.  Velocity and acceleration are the polynomial's
 * first and second derivative at the sample's local time.
 * report is B x GTOP_TRAJ_REPORT doubles per trajectory:
 *   [0] number of samples
 *   [1] clearance: the least distance over the samples (an out-of-map sample
 *       contributes -1)        [2] eval_t of the first sample that attains it
 *   [3] that sample's index
 *   [4] number of samples with distance <= margin (out-of-map samples count
 *       whenever margin >= -1) [5] eval_t of the first such sample, -1 if none
 *   [6] number of samples out of the map
 *   [7] max ||v||_2   [8] max ||a||_2   over the samples
 *   [9] max |v_k|     [10] max |a_k|    over the samples and the three axes
 *   [11] time_sum
 * One wavefront per trajectory, nothing per sample goes to HBM.
 *
 * Selection: row b PASSES iff report[b][4] == 0, and report[b][6] == 0 unless
 * allow_out_of_map, and max_vel <= 0 or its velocity figure <= max_vel, and
 * max_acc <= 0 or its acceleration figure <= max_acc (per_axis: entries 9 and 10
 * instead of 7 and 8), and cost[b] is finite.  pass[b] (uint8, may be NULL) says
 * so; best[0] (int32) = the passing row of least cost, lowest index on a tie, -1
 * if none passes; best[1] = the number of passing rows.  Deterministic.
 *
 * The _device forms only enqueue (the report one launch, the selection two): no
 * allocation, no synchronisation, no host round trip; capturable — a captured
 * report reads the boxes, the start times and the field as they are at replay.
 * gtop_validate_batch serves the first B rows of the context's problem at free
 * variables x (coefficients as gtop_trajectory_stats forms them); with cost ==
 * NULL the selection is skipped and pass / best are left alone.
 * Errors, nothing launched: dt_sample <= 0, a non-finite margin, max_vel or
 * max_acc: GTOP_ERR_INVALID; a start-time count on the context that is neither
 * 0, 1 nor B (for gtop_validate_batch the problem's batch serves too), with or
 * without use_boxes: GTOP_ERR_INVALID; no fp64 field resident: GTOP_ERR_STATE.
 * B = 0 is accepted by both device forms: the report launches nothing, the
 * selection writes best = {-1, 0} (gtop_validate_batch needs B >= 1, as
 * gtop_trajectory_stats does).
 * The selection's first stage leaves its partial results in a small workspace
 * the context owns (allocated by gtop_create, which fails with GTOP_ERR_HIP if
 * that allocation fails): gtop_select_best_device calls on ONE context must be
 * ordered with each other — the same stream, or events / graph dependencies
 * between them; two of them in flight at once (two streams, parallel branches
 * of a graph) race on it.  Use one context per concurrent selection.
 * fp64 only.  The gtop_group_* entry points do not forward it; a member context
 * can be used through gtop_group_context. */
typedef struct {
  double margin;            /* a sample with distance <= margin is a violation */
  double max_vel, max_acc;  /* <= 0: that limit is off */
  int32_t per_axis;         /* limits apply to max |v_k|, |a_k| (kinodynamic_astar.cpp:180), not to the norms */
  int32_t allow_out_of_map; /* out-of-map samples alone do not fail a row */
  int32_t use_boxes;        /* distances against the moving boxes at tau = t0 + eval_t */
} gtop_limits;
#define GTOP_TRAJ_REPORT 12
int gtop_validate_trajectories_device(gtop_ctx *ctx, int B, int m, const void *d_coeff,
                                      const void *d_T, int time_stride, double dt_sample,
                                      const gtop_limits *limits, void *d_report, void *hip_stream);
int gtop_select_best_device(gtop_ctx *ctx, int B, const void *d_report, const void *d_cost,
                            const gtop_limits *limits, void *d_pass, void *d_best,
                            void *hip_stream);
int gtop_validate_batch(gtop_ctx *ctx, int B, const double *x, double dt_sample,
                        const gtop_limits *limits, const double *cost, double *report,
                        unsigned char *pass, int32_t best[2]);

/* ---- per-segment trajectory report ------------------------------------- */
/* (Not a PolynomialTraj method.)  The report above says THAT a row fails and names
 * its sample of least clearance; a row that is too fast or too close in several
 * places needs the figures per SEGMENT, the unit a caller can act on: insert a
 * waypoint, or stretch a time (below).  The samples, the segment each one belongs
 * to, positions, velocities, accelerations and distances are exactly those of
 * gtop_validate_trajectories_device: the accumulated eval_t, the walk
 * `while (idx < m-1 && ts[idx] <= t)` of PolynomialTraj::evaluate
 * (polynomial_traj.hpp:48-51) with the last segment extended, and the
 * interpolating lookup at tau = t0[b] + eval_t with use_boxes, -1 otherwise — both
 * kinds of box list, any number of boxes, a signed field as it is, the start-time
 * rules of gtop_set_start_times[_device].  Of `limits` only margin and use_boxes
 * are read (the others must still be finite).
 * seg_report is B x m x GTOP_SEG_REPORT doubles; row [b][s] covers the samples
 * whose walk ends at idx == s:
 *   [0] number of samples                        (a segment without samples:  0)
 *   [1] index of its first sample                                            -1
 *   [2] clearance: the least distance (an out-of-map sample gives -1)      +inf
 *   [3] eval_t of the first sample that attains it                           -1
 *   [4] samples with distance <= margin                                       0
 *   [5] samples out of the map                                                0
 *   [6] max ||v||_2   [7] max ||a||_2   over its samples                      0
 *   [8] max |v_k|     [9] max |a_k|     over its samples and the three axes   0
 * (a segment time below dt_sample can leave a segment without a sample).  Against
 * the whole report R of the same inputs, bit for bit: sum_s [0] = R[0]; the [1] of
 * consecutive non-empty segments advance by [0]; min_s [2] = R[1], and the first
 * segment attaining it has [3] = R[2] and holds sample R[3]; sum_s [4] = R[4];
 * sum_s [5] = R[6]; max_s [6..9] = R[7..10].
 * One wavefront per trajectory (csrc/gtop_segments.hip); every row is written
 * exactly once; nothing per sample goes to HBM.
 * The device form only enqueues one launch: no allocation, no synchronisation,
 * capturable; boxes, start times and the field are read at replay, the list's kind
 * and length are launch arguments, as for the report.  Errors are those of
 * gtop_validate_trajectories_device; B = 0 launches nothing.  gtop_validate_segments
 * serves the first B rows of the context's problem at free variables x
 * (1 <= B <= the problem's batch), staged as gtop_validate_batch stages.
 * fp64 only.  The gtop_group_* entry points do not forward it. */
#define GTOP_SEG_REPORT 10
int gtop_validate_segments_device(gtop_ctx *ctx, int B, int m, const void *d_coeff,
                                  const void *d_T, int time_stride, double dt_sample,
                                  const gtop_limits *limits, void *d_seg_report,
                                  void *hip_stream);
int gtop_validate_segments(gtop_ctx *ctx, int B, const double *x, double dt_sample,
                           const gtop_limits *limits, double *seg_report);

/* ---- segment-time reallocation ----------------------------------------- */
/* Segment times are length / mean_v of the straight-line path
 * (src/grad_traj_optimizer.cpp:73-81) and never change afterwards: a candidate the
 * optimizer has bent around an obstacle keeps the times of the path it no longer
 * follows, and one that breaks max_vel / max_acc can only be discarded.  The
 * reference has the remedy written down and switched off: the commented block
 * "reallocate segment time" behind the solve (src/grad_traj_optimizer.cpp:209-227).
 *
 * GTOP_RETIME_LENGTH is that block.  For i = 0 .. m-1, len = the distance between
 * waypoint positions i and i+1 AS THEY STAND IN x (position 0 is Df[k][0],
 * position m is Df[k][3], interior position j is x[3(j-1) + k(3m-3)]), formed as
 * sqrt(dx*dx + dy*dy + dz*dz) unfused, and T_out[i] = len / mean_v, plus init_time
 * for i == 0 AND i == m-1 — the block's rule (:226); setPath's own condition (:76)
 * only ever fires on the first segment, so on a straight-line start T_out equals
 * gtop_setup_paths_device's T but for init_time on the last segment.  Reads x and
 * Df, writes T_out; d_T and d_seg_report are not read (may be NULL).  mean_v must be
 * finite and > 0, init_time finite and >= 0.
 *
 * GTOP_RETIME_LIMITS stretches the segments that break a limit.  With V, A the
 * segment report's entries (6, 7), or (8, 9) under per_axis, each step one rounded
 * IEEE operation, nothing fused:
 *   rv = max_vel > 0 ? V / max_vel : 0      ra = max_acc > 0 ? sqrt(A / max_acc) : 0
 *   ratio_s = fmin(fmax(fmax(rv, ra), 1.0), max_ratio)
 *   uniform:  ratio_s := the largest ratio of the trajectory's segments
 *   T_out[s] = ratio_s * T[s]
 *   scale_x:  rho_k = fmax(ratio_{k-1}, ratio_k), k = 1 .. m-1;
 *             v_k := v_k / rho_k;  a_k := a_k / (rho_k * rho_k)     (in x, in place)
 * Times only grow; a segment within its limits keeps its bits, and so does a
 * junction with rho_k == 1.  Positions and Df are never written: the boundary
 * state is the caller's.  With uniform and scale_x on a rest-to-rest row (zero
 * boundary velocity and acceleration) the result is exactly the old curve flown
 * lambda times slower, p'(t) = p(t / lambda): velocities fall by lambda,
 * accelerations by lambda^2.  Otherwise the result is a new problem (x, T_out) to
 * re-optimise or to hand to gtop_min_jerk_start_device: a remedy, not a guarantee.
 * The loop is report -> reallocate -> optimise -> report:
 *   gtop_coefficients_device, gtop_validate_segments_device,
 *   gtop_reallocate_times_device, [gtop_min_jerk_start_device,]
 *   gtop_optimize_device_ex on (x, T_out), gtop_coefficients_device,
 *   gtop_validate_trajectories_device, gtop_select_best_device
 * — all on one stream, capturable as one graph.  max_ratio must be finite and >= 1;
 * a max_vel / max_acc <= 0 (or NaN) switches that limit off.
 *
 * One lane per trajectory, O(m) (csrc/gtop_retime.hip).  d_T_out is B x m.
 * d_T_out == d_T is allowed when time_stride == m (each lane reads a time before it
 * writes it); any other overlap of the buffers is not allowed.  time_stride == 0
 * gives per-trajectory output from a shared input.  The device form only enqueues
 * one launch and can be captured.  GTOP_ERR_INVALID, nothing launched: opt NULL, an
 * unknown mode, the parameter rules above, B < 0, m outside 2 .. 227, a time_stride
 * that is neither 0 nor m, and for B > 0 a NULL buffer that the mode reads or
 * writes (LENGTH: x, Df, T_out; LIMITS: T, seg_report, T_out, and x under scale_x).
 * B = 0 launches nothing.
 * gtop_reallocate_times serves the first B rows of the context's problem
 * (GTOP_ERR_STATE when none is set): LIMITS forms the coefficients and the segment
 * report itself from x, dt_sample and limits (errors as gtop_validate_segments);
 * LENGTH ignores both.  x is updated in place under scale_x.  The context's problem
 * is NOT changed: pass T_out to gtop_set_problem.  fp64 only; not forwarded by
 * groups. */
#define GTOP_RETIME_LENGTH 0 /* the reference's commented block, src/grad_traj_optimizer.cpp:209-227 */
#define GTOP_RETIME_LIMITS 1 /* stretch the segments that break max_vel / max_acc */
typedef struct {
  int32_t mode;
  double mean_v, init_time; /* LENGTH */
  double max_vel, max_acc;  /* LIMITS; <= 0: that limit is off */
  int32_t per_axis;         /* LIMITS: entries 8, 9 of the segment report instead of 6, 7 */
  int32_t uniform;          /* LIMITS: every segment takes the largest ratio of its trajectory */
  int32_t scale_x;          /* LIMITS: also rescale the interior velocities and accelerations of x, in place */
  double max_ratio;         /* LIMITS: cap of a segment's stretch, finite and >= 1 */
} gtop_retime;
int gtop_reallocate_times_device(gtop_ctx *ctx, const gtop_retime *opt, int B, int m, void *d_x,
                                 const void *d_Df, const void *d_T, int time_stride,
                                 const void *d_seg_report, void *d_T_out, void *hip_stream);
int gtop_reallocate_times(gtop_ctx *ctx, const gtop_retime *opt, int B, double *x,
                          double dt_sample, const gtop_limits *limits, double *T_out);

/* ---- continuous-time clearance certificate ------------------------------ */
/* (Not a PolynomialTraj method.)  Every figure of the reports above is SAMPLED: a
 * row passes when none of the getTraj samples is within the margin, and between
 * two samples nothing is known — at a coarse dt_sample a thin obstacle fits there.
 * The certificate bounds the interpolated distance over whole time intervals.  The
 * lookup is trilinear, so affine in each coordinate inside a cell: over an
 * axis-aligned box inside one cell its minimum is attained at a vertex of the box.
 * A box that contains the curve over an interval, cut along the cells it touches,
 * gives a lower bound of the distance over the interval from 8 trilinear values per
 * cell, for ANY field the library holds (an exact ESDF, a windowed one with its
 * 10000 sentinels, a signed one, arbitrary values of gtop_set_sdf): no Lipschitz
 * assumption is made.  These three entry points certify the STATIC field; the moving
 * boxes are certified, over whole time intervals too, by gtop_certify_moving_device
 * below (a sampled box figure has the same hole between two samples, and a wider
 * one: a thin box needs only to cross the curve there).
 *
 * Per segment (time T) and axis k: A_k = 2|c2| + 6|c3|T + 12|c4|T^2 + 20|c5|T^3
 * bounds the acceleration.  An interval is [a, a + w] in the segment's local time.
 * Level 0 cuts a segment into 64 intervals, w = T/64, a = j w, j = 0 .. 63;
 * refining an interval replaces it by 64 children, w' = w/64, a' = a + j w'.  With
 * h = w/2, tc = a + h: p = the position and v = the velocity at tc; the box is
 * p_k +- r_k, r_k = |v_k| h + A_k h^2 / 2, enlarged to r_k (1 + 2^-40) + 2^-40 (P_k
 * + C), P_k = sum_j |c_j| T^j, C = the largest absolute coordinate of a cell face of
 * the map: over a hundred times the rounding of the interval ends, the position and
 * the sub-box ends.
 *   d_mid = the `dist` gtop_edt_query_device returns for (p, -1), bit for bit (-1
 *     out of the map).
 *   lb = -inf if p - r or p + r fails the in-map test of the lookup, or if the box
 *     spans more than 2 of the lookup's cells (floor((x - res/2 - origin) / res)
 *     at both ends) on an axis; else the least, over the at most 8 cells the box
 *     touches, of that cell's trilinear form (its 8 corners with the lookup's
 *     clamps) at the 8 vertices of the box cut to the cell (local coordinates
 *     against that cell, clamped to [0, 1]), minus 2^-46 (8 + C / res) times the
 *     largest |corner value| involved (the rounding of the forms and coordinates).
 *   VIOLATION if d_mid <= margin (the report's comparison), else CERTIFIED if
 *   lb > margin, else OPEN.
 * An OPEN interval is refined while its level is below max_depth and fewer than
 * max_refine refinements have been done for this trajectory; after that it is an
 * undecided leaf.  A VIOLATION is never refined.  Segments in order, within a
 * segment depth-first in ascending time; level 0 of every segment is always
 * evaluated.  cert is B x GTOP_CERT_REPORT doubles per trajectory:
 *   [0] verdict: -1 UNSAFE (an evaluated midpoint has d_mid <= margin), +1 SAFE (no
 *       violation and no undecided leaf), 0 UNDECIDED
 *   [1] lo: the least lb over all leaves — a certified lower bound of the
 *       interpolated distance over [0, time_sum]; -inf if the curve leaves the map
 *   [2] hi: the least d_mid over every evaluated midpoint of every level
 *   [3] the trajectory time of the earliest midpoint that attains hi
 *   [4] the trajectory time of the earliest evaluated midpoint with d_mid <=
 *       margin, -1 if none
 *   [5] the number of undecided leaves   [6] the number of refinements done
 *   [7] time_sum
 * SAFE implies lo > margin.  A row's result depends neither on B nor on the row's
 * place in the batch; results are deterministic.  One wavefront per trajectory
 * (csrc/gtop_certify.hip), nothing per interval goes to HBM.
 *
 * gtop_certify_trajectories_device only enqueues one launch: no allocation, no
 * synchronisation, capturable; the field is read at replay.  gtop_certify_batch
 * serves the first B rows of the context's problem at free variables x (1 <= B <=
 * the problem's batch; GTOP_ERR_STATE when none is set), staged as
 * gtop_validate_batch stages.  gtop_select_best_certified_device is
 * gtop_select_best_device's rule plus one condition on cert[b][0]:
 * GTOP_CERT_REQUIRE_SAFE verdict == +1, GTOP_CERT_REQUIRE_NOT_UNSAFE verdict != -1
 * — the same two launches and the same workspace, so its calls are ordered with
 * gtop_select_best_device's as those are with each other.
 * GTOP_ERR_INVALID, nothing launched: opt NULL, a non-finite margin, max_depth
 * outside 0 .. GTOP_CERT_MAX_DEPTH, max_refine < 0, B < 0, m outside 2 .. 227, a
 * time_stride that is neither 0 nor m, a NULL buffer with B > 0, a `require` that
 * is neither value, the limits rules of gtop_select_best_device.  No fp64 field
 * resident: GTOP_ERR_STATE.  B = 0 launches nothing (the selection writes best =
 * {-1, 0}).  fp64 only.  The gtop_group_* entry points do not forward it. */
typedef struct {
  double margin;      /* a midpoint with distance <= margin is a violation; lb > margin certifies */
  int32_t max_depth;  /* 0 .. GTOP_CERT_MAX_DEPTH: levels of refinement below the 64 intervals of a segment */
  int32_t max_refine; /* >= 0: refinements per trajectory */
} gtop_certify_opts;
#define GTOP_CERT_REPORT 8
#define GTOP_CERT_MAX_DEPTH 3
#define GTOP_CERT_REQUIRE_SAFE 1
#define GTOP_CERT_REQUIRE_NOT_UNSAFE 2
int gtop_certify_trajectories_device(gtop_ctx *ctx, int B, int m, const void *d_coeff,
                                     const void *d_T, int time_stride,
                                     const gtop_certify_opts *opt, void *d_cert, void *hip_stream);
int gtop_certify_batch(gtop_ctx *ctx, int B, const double *x, const gtop_certify_opts *opt,
                       double *cert);
int gtop_select_best_certified_device(gtop_ctx *ctx, int B, const void *d_report,
                                      const void *d_cert, const void *d_cost,
                                      const gtop_limits *limits, int require, void *d_pass,
                                      void *d_best, void *hip_stream);

/* ---- the certificate against the moving boxes (ABI version 11) ----------- */
/* For a row b the certified quantity is the `dist` gtop_edt_query_device returns for
 * (x(t), tau = start + t): the trilinear form over corner values min(static, distance
 * from the corner voxel's centre to the nearest box at tau), for either kind of box
 * list (gtop_set_moving_boxes, gtop_set_moving_box_polynomials) and any number of
 * boxes.  `start` is the row's start time under the rules of
 * gtop_set_start_times[_device] (none: 0; one: shared; else one per row).  Two
 * monotonicities of the lookup carry the bound: the trilinear weights lie in [0, 1]
 * on the clamped local coordinates, so the form is non-decreasing in every corner
 * value; and a corner's distance to a box does not grow when the box's faces move
 * outwards (the subtraction, the squares, their sum and the sqrt round
 * monotonically).  With each box replaced by an axis-aligned box that contains it at
 * every tau of an interval, the vertex minimum per touched cell of the static
 * certificate is a lower bound for every point and time of the interval — for any
 * field, as before.
 *
 * The interval tree, the curve box, its cells and sub-boxes, the VIOLATION /
 * CERTIFIED / OPEN rule, the budget, the order and the 8 columns of cert are those of
 * gtop_certify_trajectories_device above.  New, per interval [a, a + w] of a segment
 * with time Ts that starts at trajectory time t_off, all in plain fp64 operations:
 *   d_mid = the `dist` the query returns for (p, start + t), t = t_off + tc as entry
 *     3 has it, bit for bit; out of the map -1 and the boxes ignored, as the query.
 *   ta = start + (t_off + a), tb = start + (t_off + (a + w)),
 *   delta = 2^-40 (|start| + (t_off + Ts)), tau_a = ta - delta, tau_b = tb + delta.
 *   The boxes are applied iff tau_b >= 0 (a wholly negative interval is static only,
 *   as the query; one that straddles 0 takes the boxes over all of [tau_a, tau_b]).
 *   Constant-velocity box: the query's faces at tau_a and at tau_b; per axis the
 *     smaller lower and the larger upper face (the centre is a monotone function of
 *     tau in floating point: no slack).
 *   Polynomial box: tca, tcb = tau_a, tau_b clamped into the box's [t1, t2];
 *     hh = 0.5 (tcb - tca), tm = tca + hh, M = max(|tca|, |tcb|); per axis
 *     cm = the centre at tm (the fma Horner of gtop_box_polynomial_centres),
 *     vq = ((((5 c5) tm + 4 c4) tm + 3 c3) tm + 2 c2) tm + c1,
 *     Aq = 2|c2| + 6|c3| M + 12|c4| M^2 + 20|c5| M^3,
 *     Qk = ((((|c5| M + |c4|) M + |c3|) M + |c2|) M + |c1|) M + |c0|,
 *     rq = |vq| hh + 0.5 Aq hh hh, then rq (1 + 2^-40) + 2^-40 Qk;
 *     faces (cm - rq) - half extent and (cm + rq) + half extent.  A cm or rq that is
 *     not finite: the box covers everything (distance 0 at every corner).
 *   lb: for each of the at most 8 cells the curve box touches, the static corner
 *     values; V = the largest |static corner value| of the touched cells (taken
 *     before any min: the query's form at any tau holds values between the lowered
 *     and the static ones); then every corner lowered to its distance to every swept
 *     box (with the query's exact skip, per cell); the 8 vertex values as in the
 *     static certificate; lb = their least - 2^-46 (8 + C / res) V.
 * DESIGN.md 5.15 bounds the roundings delta and 2^-40 Qk cover.
 *
 * cert is the same B x GTOP_CERT_REPORT row, so gtop_select_best_certified_device
 * takes it unchanged.  With use_boxes == 0 or an empty box list the call launches the
 * static kernel: the result is gtop_certify_trajectories_device's, bit for bit.
 * use_boxes is independent of gtop_set_moving_cost.  gtop_certify_moving_device only
 * enqueues one launch: no allocation, no synchronisation, capturable; the boxes, the
 * start times and the field are read at replay (a captured launch keeps the list's
 * kind and length).  gtop_certify_moving_batch stages as gtop_certify_batch does.
 * Errors: those of gtop_certify_trajectories_device / gtop_certify_batch, and
 * GTOP_ERR_INVALID for reserved != 0 and for a start-time count that is neither 0, 1
 * nor B (for the batch form the problem's batch serves too, as for
 * gtop_validate_batch).  fp64 only.  The gtop_group_* entry points do not forward
 * it. */
typedef struct {
  double margin;
  int32_t max_depth, max_refine; /* as gtop_certify_opts */
  int32_t use_boxes;             /* 0: the static certificate, bit for bit */
  int32_t reserved;              /* must be 0 */
} gtop_certify_moving_opts;
int gtop_certify_moving_device(gtop_ctx *ctx, int B, int m, const void *d_coeff, const void *d_T,
                               int time_stride, const gtop_certify_moving_opts *opt, void *d_cert,
                               void *hip_stream);
int gtop_certify_moving_batch(gtop_ctx *ctx, int B, const double *x,
                              const gtop_certify_moving_opts *opt, double *cert);

/* ---- waypoint insertion (ABI version 12) --------------------------------- */
/* (Not in the reference: the number of segments m is fixed by setPath.)  The
 * per-segment report names two remedies for a row that fails; stretching a time is
 * gtop_reallocate_times, this is the other.  A row whose curve runs through an
 * obstacle has no free variable where the collision is: the call cuts ONE segment s
 * of each of the B rows at a local time tl, which gives a problem of m + 1 segments
 * for every row (the batch stays rectangular).  The new junction carries the old
 * curve's position, velocity and acceleration at the cut.  A quintic is fixed by its
 * six end conditions, so in exact arithmetic the two new segments are the old one
 * restricted to [0, tl] and [tl, Ts]: the trajectory is unchanged, and the optimizer
 * gains nine free variables where they are needed.  Optionally the new waypoint is
 * pushed up the static field's gradient.  Df is not touched.
 *
 * d_x is B x 9(m-1) and d_coeff B x m x 18 (gtop_coefficients_device of the same x,
 * Df and T), d_T B x m or m (time_stride m or 0).  d_x_out, d_lb_out and d_ub_out are
 * B x 9m in the layout x[i + axis * 3m]; d_T_out is B x (m+1), per trajectory also
 * when time_stride == 0.  Under GTOP_INSERT_AT_TIME the trajectory time of row b's
 * cut is the double d_when[b * when_stride], when_stride >= 1: a caller points at a
 * column of a device report — report + 2 with stride GTOP_TRAJ_REPORT (the time of
 * the least clearance), cert + 3 or cert + 4 with stride GTOP_CERT_REPORT.  d_when is
 * not read under GTOP_INSERT_LONGEST.  d_lb and d_ub (the bounds of x): both or
 * neither; d_lb_out and d_ub_out are required exactly when they are given.  d_info
 * (B x GTOP_INSERT_INFO) is optional.
 *
 * The rule per row, every step ONE rounded fp64 operation in the order written,
 * nothing fused (csrc/gtop_insert.hip):
 *   1. AT_TIME: t = when.  If !(t >= 0 && t < inf) — NaN, inf, the -1 of "no
 *      violation" in cert[4] — the row falls back to LONGEST and info[2] = 1.
 *   2. AT_TIME: s = the segment the walk `while (idx < m-1 && ts[idx] <= t)
 *      t -= ts[idx++]` of the reports ends in (the last segment extended), tl = the
 *      remaining t, Ts = T[s].
 *   3. LONGEST: s = the FIRST index of the largest T[s] (a later segment replaces
 *      the current one only on strict >), tl = 0.5 * Ts.
 *   4. lo = min_fraction * Ts, hi = Ts - lo, tl = fmin(fmax(tl, lo), hi); info[3] = 1
 *      if that changed tl.
 *   5. T_out[s] = tl, T_out[s+1] = Ts - tl; the other times are copied, shifted by
 *      one behind s.
 *   6. Per axis, c the coefficients of segment s: p = the getTraj point, ((((0 +
 *      t5 c5) + t4 c4) + t3 c3) + t2 c2) + tl c1) + c0 with t2 = tl tl, t3 = t2 tl,
 *      t4 = t2 t2, t5 = t4 tl.  When `when` is a report's entry 2 and the clamp is
 *      idle, the new waypoint IS that sample, bit for bit.
 *   7. v = ((((5 c5) tl + 4 c4) tl + 3 c3) tl + 2 c2) tl + c1,
 *      a = (((20 c5) tl + 12 c4) tl + 6 c3) tl + 2 c2, the integer factor applied to
 *      the coefficient first.
 *   8. push > 0 only (otherwise no field is needed): (d, g) = what
 *      gtop_edt_query_device returns for (p, -1), bit for bit.  n = sqrt(gx gx +
 *      gy gy + gz gz), summed left to right.  Unless the point is out of the map, or
 *      d >= push_below, or n == 0: p_k = p_k + (push * g_k) / n.  v and a stay.
 *      info[4] = d (0 when push is off), info[5] = pushed, 0 or 1.  The pushed point
 *      is NOT tested against the map or the field: push is a start for the
 *      optimizer, which the next report judges.
 *   9. Junction k' = 1 .. m of the output: k' <= s is old junction k'; k' == s + 1
 *      is the new (p, v, a); k' > s + 1 is old junction k' - 1.
 *  10. Bounds: old entries are copied by the same map; the new waypoint takes
 *      gtop_default_bounds' rule around the FINAL p: p -+ bos, -+vos, -+aos.  The new
 *      v and a are the old curve's and may lie beyond vos / aos: that is legal
 *      input, gtop_optimize_device_ex clamps its start point into the bounds.
 *  11. info[0] = s, info[1] = tl.
 * A row's bits depend on that row's inputs only: not on B, on its index, or on
 * time_stride.  A NaN or zero segment time gives garbage in that row only; the call
 * stays memory-safe.
 *
 * The loop is coefficients -> report / certify -> insert -> optimise on m + 1:
 *   gtop_coefficients_device, gtop_validate_trajectories_device or
 *   gtop_certify_trajectories_device, gtop_insert_waypoints_device,
 *   [gtop_min_jerk_start_device,] gtop_optimize_device_ex on (x_out, T_out, m + 1),
 *   gtop_coefficients_device, gtop_validate_trajectories_device,
 *   gtop_select_best_device
 * — all on one stream, capturable as one graph.
 *
 * One wavefront per trajectory; every output entry is written exactly once.  The
 * device form only enqueues one launch: no allocation, no synchronisation,
 * capturable; the field is read at replay.  Outputs must not overlap inputs or each
 * other.  GTOP_ERR_INVALID, nothing launched: opt NULL, an unknown mode, reserved
 * != 0, min_fraction outside (0, 0.5] or NaN, a non-finite push or push_below, with
 * bounds a bos, vos or aos that is negative or not finite, lb without ub (or ub
 * without lb), bounds without their outputs (or outputs without bounds), B < 0, m
 * outside 2 .. 226 (m + 1 must be servable), a time_stride that is neither 0 nor m,
 * when_stride < 1 under AT_TIME, and for B > 0 a NULL x, coeff, T, x_out or T_out,
 * or a NULL when under AT_TIME.  push > 0 without a resident fp64 field:
 * GTOP_ERR_STATE.  B = 0 launches nothing.
 * gtop_insert_waypoints serves the first B rows of the context's problem at free
 * variables x (1 <= B <= the problem's batch; GTOP_ERR_STATE when none is set), the
 * coefficients staged as gtop_validate_batch stages them; when may be NULL under
 * LONGEST (one entry per row otherwise), lb / ub / lb_out / ub_out and info as above.
 * The context's problem is NOT changed: pass T_out to gtop_set_problem(B, m + 1,
 * T_out, m + 1, Df).  fp64 only; not forwarded by groups. */
#define GTOP_INSERT_AT_TIME 0 /* cut at the trajectory time d_when gives */
#define GTOP_INSERT_LONGEST 1 /* cut the longest segment in the middle */
typedef struct {
  int32_t mode;
  double min_fraction;     /* in (0, 0.5]: the cut keeps this share of the segment on either side */
  double push, push_below; /* push <= 0: off; else the step up the gradient where the distance is below push_below */
  double bos, vos, aos;    /* bounds of the new waypoint, read only when lb / ub are given */
  int32_t reserved;        /* must be 0 */
} gtop_insert;
#define GTOP_INSERT_INFO 6
int gtop_insert_waypoints_device(gtop_ctx *ctx, const gtop_insert *opt, int B, int m, const void *d_x,
                                 const void *d_coeff, const void *d_T, int time_stride,
                                 const void *d_when, int when_stride, const void *d_lb,
                                 const void *d_ub, void *d_x_out, void *d_T_out, void *d_lb_out,
                                 void *d_ub_out, void *d_info, void *hip_stream);
int gtop_insert_waypoints(gtop_ctx *ctx, const gtop_insert *opt, int B, const double *x,
                          const double *when, const double *lb, const double *ub, double *x_out,
                          double *T_out, double *lb_out, double *ub_out, double *info);

/* ---- bookkeeping the reference keeps inside the callback ------------ */

/* iter_num and total_time (src/grad_traj_optimizer.cpp:284, :436); reset as
 * optimizeTrajectory does after a step-2 solve (:236-239). */
int gtop_get_stats(const gtop_ctx *ctx, int64_t *iter_num, double *total_time);
int gtop_reset_stats(gtop_ctx *ctx);
/* Best-so-far cost curve (src/grad_traj_optimizer.cpp:439-447,
 * include/grad_traj_optimization/grad_traj_optimizer.h:127-130).  Copies up
 * to `cap` entries; *count receives the number available. */
int gtop_get_cost_curve(const gtop_ctx *ctx, double *cost, double *time,
                        int cap, int *count);
int gtop_clear_cost_curve(gtop_ctx *ctx);

/* ---- tuning knobs (not in the reference) ---------------------------- */

/* Launch geometry of the evaluation kernel (csrc/gtop_launch_rule.cpp,
 * gtop_eval_plan).  A wavefront always holds whole segments; `waves` must be 0
 * or 1 (the number of wavefronts per workgroup follows from the rule below and
 * is not a knob).  samples_per_lane:
 *   3   ten lanes per polynomial segment.  Up to 6 segments: one trajectory per
 *       wavefront.  7 .. 12 segments: one trajectory over TWO wavefronts (a
 *       128-thread workgroup, wavefront w holds segments 6w .. 6w+5).  More
 *       than 12 segments (and the batched optimizer past 6): GTOP_ERR_INVALID
 *       at the evaluation.
 *   6   five lanes per segment: two trajectories of up to 6 segments per
 *       wavefront, one of up to 12, or 12 segments at a time beyond that.
 *   10  three lanes per segment, 21 / m whole trajectories per wavefront; up to
 *       10 segments, plain evaluations; more: GTOP_ERR_INVALID at the
 *       evaluation.  Five lanes per segment leave most of a wavefront idle for
 *       every length but 6, 11 and 12 segments: the rule takes three for
 *       2 .. 5 segments from 8 192 trajectories and for 7 .. 10 from 4 096.
 *   30  ONE lane per segment (a lane walks all 30 samples), 64 / m whole
 *       trajectories per wavefront; up to 64 segments, plain evaluations (the
 *       batched optimizer keeps its own rule); more segments: GTOP_ERR_INVALID
 *       at the evaluation.  Fewest instructions per trajectory, most distinct
 *       cache lines per load: the rule takes it for fp32 batches of 65 536
 *       six-segment trajectories and more, and past 12 segments wherever the
 *       12-segments-at-a-time body would end on a mostly idle chunk.
 *   0   choose from B, m and dtype (measured rule).
 * Other values are GTOP_ERR_INVALID at the call.  Results do not depend on the
 * geometry beyond fp summation order. */
int gtop_set_launch_geometry(gtop_ctx *ctx, int waves, int samples_per_lane);
/* The corner records every lookup reads exist in fp64 and fp32; the capturable
 * map-update entries (gtop_update_sdf_map_device, _window_device) rebuild both
 * so that a replayed graph leaves both current — a third of their record pass
 * (200^3: 98 us for both against 57 us for fp64 alone).  keep_fp32 = 0 tells the
 * context that it will never run fp32 evaluations: only fp64 records are kept,
 * and GTOP_F32 evaluations (and gtop_set_optimizer_precision(GTOP_F32) runs) fail
 * with GTOP_ERR_STATE.  1 (default) switches them back on; they are rebuilt from
 * the fp64 field at the next fp32 use. */
int gtop_set_field_precisions(gtop_ctx *ctx, int keep_fp32);
/* Batched optimizer: 2 (default) = one launch runs the whole loop (evaluate,
 * MMA update, evaluate, ... max_evals times) for every trajectory — they are
 * independent, so nothing has to return to the host or to HBM in between;
 * 1 = the MMA update runs as the epilogue of the evaluation kernel, one launch
 * per iteration; 0 = separate update launch.  Same arithmetic in all three. */
int gtop_set_optimizer_fusion(gtop_ctx *ctx, int fused);
/* Batched optimizer: the arithmetic of its EVALUATIONS.  GTOP_F64 (default) is
 * the reference's; GTOP_F32 runs them on the fp32 corner records in the
 * packed-fp32 bodies of gtop_eval_device(GTOP_F32) — the trial point, bounds,
 * Df, T, the CCSA-MMA update and every result stay fp64, so the interface of
 * gtop_optimize_* does not change.  Measured: 9 % less time for 1 024
 * trajectories of 6 segments, 17 % for 16 384, 20 % for 65 536.  The iterates
 * are those of an fp32 objective: an accept / reject decision within fp32's
 * noise (1e-5 relative) can fall the other way.  Needs a fused launch form
 * (fusion 1 or 2). */
int gtop_set_optimizer_precision(gtop_ctx *ctx, int dtype);

/* ---- collecting the shards' results (not in the reference) -- */

/* The all-gather of a rank's result rows as point-to-point stores: ONE kernel on
 * `hip_stream` copies `bytes` from d_src to each of the n_dsts (<= 16) device
 * pointers of d_dsts — this rank's slot in its own gathered buffer and in every
 * peer's, the peers' buffers mapped into this process (hipIpcOpenMemHandle
 * between the one-process-per-GPU ranks, peer access inside one process), each
 * destination over its own xGMI link.  Every rank's slot is written by that rank
 * alone, so no protocol is needed; an owner may read its buffer after any
 * synchronisation that orders the read behind the writers' kernels (the closing
 * barrier of a timed region).  All pointers 16-byte aligned.  Asynchronous,
 * capturable.  d_clock_minmax != NULL: the kernel also takes the device-clock
 * stamp of gtop_device_clock_stamp as it starts (behind the last evaluation, in
 * front of the stores) — a node of a graph saved.  bench.py's N > 1 runs gather their costs this way, with RCCL's
 * all-gather as the fallback when the peers' buffers cannot be mapped. */
int gtop_push_rows(gtop_ctx *ctx, const void *d_src, size_t bytes, void *const *d_dsts, int n_dsts,
                   void *d_clock_minmax, void *hip_stream);
/* Buffers for it that another process can map.  gtop_shared_alloc: a zeroed
 * device allocation of its own (an IPC handle names a whole allocation) on the
 * context's device and its 64-byte handle, to be sent to the peers by any means;
 * gtop_shared_open maps a PEER's buffer (a handle made in another process) for
 * the context's device — the device whose kernels will store into it; with
 * owner_device >= 0 (the owner's device ordinal as THIS process counts devices)
 * the call first checks hipDeviceCanAccessPeer and enables peer access, and
 * refuses (GTOP_ERR_STATE) where the owner's device cannot be reached, instead of
 * leaving a mapping a kernel would fault on; -1 = unknown: the lazy flag alone.
 * gtop_shared_close unmaps it; gtop_shared_free releases an
 * allocation of gtop_shared_alloc (after the peers have closed it). */
#define GTOP_IPC_HANDLE_BYTES 64
int gtop_shared_alloc(gtop_ctx *ctx, size_t bytes, void **d_ptr, unsigned char handle[GTOP_IPC_HANDLE_BYTES]);
int gtop_shared_open(gtop_ctx *ctx, const unsigned char handle[GTOP_IPC_HANDLE_BYTES], int owner_device,
                     void **d_ptr);
int gtop_shared_close(gtop_ctx *ctx, void *d_ptr);
int gtop_shared_free(gtop_ctx *ctx, void *d_ptr);

/* ---- measurement aid (not in the reference) --------------------------- */

/* Enqueues a one-lane kernel on `hip_stream` that reads the device's constant-
 * rate wall clock (the counter gtop_stop.maxtime is measured with) and folds it
 * into d_minmax[0] = min(d_minmax[0], t), d_minmax[1] = max(d_minmax[1], t)
 * (two uint64 in HBM; preset them to UINT64_MAX and 0).  Put one in front of and
 * one behind a run of launches — e.g. as first and last node of a captured
 * hipGraph — and (max - min) / gtop_device_clock_hz is the GPU's own time for
 * them: no host clock and no profiler instrumentation inside the interval.
 * bench.py times its region this way (`ms_per_step_gpu`). */
int gtop_device_clock_stamp(gtop_ctx *ctx, void *d_minmax, void *hip_stream);
/* Rate of that clock in Hz (hipDeviceAttributeWallClockRate; 100 MHz on MI355X). */
int gtop_device_clock_hz(gtop_ctx *ctx, double *hz);

#ifdef __cplusplus
}
#endif
#endif /* GTOP_H_ */
