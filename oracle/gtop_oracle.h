/*
 * gtop_oracle.h — interface of the CPU restatement (TEST INFRASTRUCTURE ONLY;
 * see the header of gtop_oracle.c: parity unpinned, never used by the product
 * path).  Citations are file:line into /root/reference/.
 */
#ifndef GTOP_ORACLE_H_
#define GTOP_ORACLE_H_

#ifdef __cplusplus
extern "C" {
#endif

/* ROS parameters read by the ctor (grad_traj_optimizer.cpp:5-32) that the
 * callback uses, plus `step` (:132) and the dyn-feasibility switch for the
 * commented-out block (:383-407). */
typedef struct {
  double ws, wc;          /* w_smooth, w_collision          :10-11 */
  double alpha, r, d0;    /* distance penalty               :13-15 */
  double alpha_v, r_v, v0; /* velocity penalty (dead code)  :17-19 */
  double alpha_a, r_a, a0; /* acceleration penalty (dead)   :21-23 */
  int step;               /* 0,1,2; 1 zeroes ws             :413-415 */
  int enable_dyn;         /* 0 = as shipped (block commented out) */
} oracle_params;

/* SDFMap fields the query reads (sdf_map.h:13-23) */
typedef struct {
  double origin[3], min_range[3], max_range[3];
  double resolution, resolution_inv;
  int grid[3];
  double *dist; /* x*ny*nz + y*nz + z, sdf_map.cpp:172-173 */
} oracle_sdf;

void oracle_segment_time(int npts, const double *path, double mean_v,
                         double init_time, double *T);
int oracle_generator(int m, const double *T, double *A, double *Q, double *Ct,
                     double *L, double *R);
void oracle_initial_d(int npts, const double *path, const double *vel,
                      const double *acc, double *Df, double *Dp);

void oracle_sdf_init(oracle_sdf *S, const double origin[3], double resolution,
                     const int grid[3], double *distance_buffer);
void oracle_sdf_init_size(oracle_sdf *S, const double origin[3],
                          double resolution, const double map_size[3],
                          int grid_out[3]);
double oracle_sdf_query(const oracle_sdf *S, const double pos[3],
                        double grad[3]);

/* EDTEnvironment::evaluateEDTWithGrad (src/edt_environment.cpp:75-122): trilinear
 * over min(static, moving boxes at `time`); time < 0: static only.  Boxes:
 * p0/vel/scale, nbox x 3 each.  See the .c file for the conventions taken. */
double oracle_edt_query(const oracle_sdf *S, int nbox, const double *box_p0, const double *box_vel,
                        const double *box_scale, const double pos[3], double time, double grad[3]);
int oracle_set_occupancy(const oracle_sdf *S, double *occupancy,
                         const double pos[3], int occ);
void oracle_esdf_build(const oracle_sdf *S, const double *occupancy,
                       double *distance);
/* the windowed update (sdf_map.cpp:28-53 resetBuffer(min, max), :244-264 setUpdateRange, :310-368 updateESDF3d over
 * min_vec .. max_vec) */
void oracle_window_ids(const oracle_sdf *S, const double min_pos[3], const double max_pos[3], int min_id[3],
                       int max_id[3]);
void oracle_reset_window(const oracle_sdf *S, double *occupancy, double *distance, const double min_pos[3],
                         const double max_pos[3]);
void oracle_esdf_build_window(const oracle_sdf *S, const double *occupancy, double *distance, const int lo[3],
                              const int hi[3]);

double oracle_cost_grad(int m, const double *L, const double *R,
                        const double *Df, const double *T,
                        const oracle_params *prm, const oracle_sdf *S,
                        const double *x, double *grad_out);
double oracle_eval_batch(int B, int m, const double *T, int t_stride,
                         const double *Df, const oracle_params *prm,
                         const oracle_sdf *S, const double *x, double *cost,
                         double *grad, int reps, int nthreads);

/* oracle_cost_grad plus, in mag[0 .. 2n + 5] (n = 9(m-1)), the callback re-evaluated as an a-priori rounding-error
 * magnitude — absolute values of the inputs, additions for subtractions, sums of products of magnitudes — and the
 * narrowest margin of each discrete decision:
 *   mag[0]        Cmag, mag[1 + k] Gmag[k] (same layout as grad): an implementation that rounds differently but
 *                 takes the same decisions differs from the exact callback by a small multiple of u * magnitude;
 *   mag[n + 1]    float rounding of a sample's position / velocity (/ acceleration with the dyn block): distance
 *                 of the double to the nearest float rounding boundary, relative to its magnitude;
 *   mag[n + 2]    cell choice (sdf_map.cpp:201-204): distance of the cell coordinate to an integer, relative;
 *   mag[n + 3]    in-map test (:55-69): distance to min_range + 1e-4 / max_range - 1e-4, relative;
 *   mag[n + 4]    sample count (grad_traj_optimizer.cpp:353): distance of the last tested t to T, relative to T;
 *   mag[n + 5]    Cflip, mag[n + 6 + k] Gflip[k]: absolute allowance for the sample positions / velocities whose
 *                 float rounding can go either way (pre-rounding double within 2^-44 of its magnitude from a
 *                 rounding boundary) — twice the first-order effect of one float step of each such coordinate.
 * Margins with no sample to test are +inf. */
double oracle_cost_grad_mag(int m, const double *L, const double *R,
                            const double *Df, const double *T,
                            const oracle_params *prm, const oracle_sdf *S,
                            const double *x, double *grad_out, double *mag);
/* the batch driver with mag: B x (2n + 6), one row per trajectory as above */
double oracle_eval_batch_mag(int B, int m, const double *T, int t_stride,
                             const double *Df, const oracle_params *prm,
                             const oracle_sdf *S, const double *x, double *cost,
                             double *grad, double *mag, int nthreads);

/* The callback with the two later semantics of include/gtop.h, everything else as oracle_cost_grad_mag.
 *   mode    0: the reference's gradient.  1 (gtop_set_gradient_mode, GTOP_GRADIENT_CONSISTENT, tests/consistent_twin.py):
 *           the collision weight gd*grad(k)*vn without cd; in the enable_dyn block S = sum_j (cv_j + ca_j) on the
 *           v/|v| term, sgn(vel_k) / sgn(acc_k) on the penalties' own derivatives, sgn(+-0) = 0.  The cost statements
 *           are the same in both modes.
 *   boxes   nbox > 0 (gtop_set_moving_cost): every collision sample's lookup is oracle_edt_query's arithmetic at
 *           tau = ((t0 + T[0]) + ... + T[s-1]) + t (tests/moving_twin.py).  poly == 0: p0, vel, scale (nbox x 3 each).
 *           poly != 0 (gtop_set_moving_box_polynomials): coef nbox x 3 x 6 (ascending powers), scale, t_range nbox x 2
 *           or NULL; the centre is the time clamped into [t1, t2], then Horner in explicit fma.
 * The magnitudes (same layout as oracle_cost_grad_mag's mag[]) carry, for a corner lowered by a box, the rounding of
 * the box centre (|p0| + |vel| |tau|, or the Horner magnitude sum |c_j| |tc|^j plus the derivative magnitude
 * sum j |c_j| |tc|^(j-1) times |tau| for the sample time's own error), of the half extent and of the corner centre;
 * in mode 1 Gflip also holds, twice, the gv*vn / ga*vn term of every sample whose pre-rounding velocity /
 * acceleration lies within 2^-44 of its magnitude from zero (its sgn may differ in a correct implementation). */
typedef struct {
  int mode;
  int nbox, poly;
  const double *p0, *vel, *scale; /* poly == 0: p0, vel; both: scale */
  const double *coef, *t_range;   /* poly != 0 */
} oracle_ext;

/* mag may be NULL (no magnitudes); ext may be NULL (mode 0, no boxes). */
double oracle_cost_grad_ext(int m, const double *L, const double *R, const double *Df, const double *T,
                            const oracle_params *prm, const oracle_sdf *S, const double *x, const oracle_ext *ext,
                            double t0, double *grad_out, double *mag);
/* the batch driver: t0 NULL (all zero), t0_stride 0 (one shared value) or 1; lowered (B, or NULL): the number of
 * collision samples of each row with at least one corner value lowered by a box. */
double oracle_eval_batch_ext(int B, int m, const double *T, int t_stride, const double *Df, const oracle_params *prm,
                             const oracle_sdf *S, const double *x, const oracle_ext *ext, const double *t0,
                             int t0_stride, double *cost, double *grad, double *mag, int *lowered, int nthreads);

void oracle_traj_stats(int m, const double *coeff, const double *T, double dt_sample, double *out);
/* PolynomialTraj::getTraj (polynomial_traj.hpp:69-78): returns the number of points, stores the first max_samples */
int oracle_traj_samples(int m, const double *coeff, const double *T, double dt_sample, int max_samples,
                        double *samples);
/* EDTEnvironment::evaluateCoarseEDT (src/edt_environment.cpp:124-136) */
double oracle_edt_coarse(const oracle_sdf *S, int nbox, const double *box_p0, const double *box_vel,
                         const double *box_scale, const double pos[3], double time);
void oracle_coefficients(int m, const double *L, const double *Df, const double *x, double *coe);

#ifdef __cplusplus
}
#endif
#endif
