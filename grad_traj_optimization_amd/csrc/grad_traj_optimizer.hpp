// grad_traj_optimizer.hpp — C++ host shim with the public interface of the
// reference's GradTrajOptimizer
// (include/grad_traj_optimization/grad_traj_optimizer.h:20-39, :127-130 of
// EpicOne1/grad_traj_optimization), implemented on the C-ABI of include/gtop.h.
//
// Same method names, argument meaning and (absence of) error behaviour:
// optimizeTrajectory always returns true (src/grad_traj_optimizer.cpp:242),
// nothing throws.  Differences forced by the image (no Eigen, no ROS, no
// NLopt headers): Eigen::Vector3d -> gtop_amd::Vec3, Eigen::MatrixXd ->
// gtop_amd::Matrix (row-major), the ROS parameter server -> the Config struct
// (same 21 names, src/grad_traj_optimizer.cpp:5-32), nlopt::opt -> the CCSA-MMA
// driver in mma.hpp (NLopt algorithm 24 = LD_MMA is what opti_node.launch
// selects; its algorithm is restated from Svanberg 2002 / NLopt 2.5.0's
// published mma.c, see mma.hpp).
#ifndef GTOP_AMD_GRAD_TRAJ_OPTIMIZER_HPP_
#define GTOP_AMD_GRAD_TRAJ_OPTIMIZER_HPP_

#include <array>
#include <string>
#include <vector>

#include "gtop.h"
#include "gtop_kinematics.h"
#include "gtop_prediction.h"
#include "gtop_swarm.h"
#include "gtop_joint.h"
#include "gtop_time.h"
#include "gtop_time_moving.h"

#define OPT_INITIAL_TRY 0
#define OPT_FIRST_STEP 1
#define OPT_SECOND_STEP 2

namespace gtop_amd {

using Vec3 = std::array<double, 3>;

// Minimal dense row-major matrix (stands in for Eigen::MatrixXd at the API).
struct Matrix {
  int rows = 0, cols = 0;
  std::vector<double> a;
  Matrix() = default;
  Matrix(int r, int c) : rows(r), cols(c), a((size_t)r * c, 0.0) {}
  void resize(int r, int c) { rows = r; cols = c; a.assign((size_t)r * c, 0.0); }
  double &operator()(int r, int c) { return a[(size_t)r * cols + c]; }
  double operator()(int r, int c) const { return a[(size_t)r * cols + c]; }
};

class GradTrajOptimizer {
 public:
  // The parameters the reference's ctor reads from the ROS parameter server
  // under /traj_opti_node1/* (src/grad_traj_optimizer.cpp:5-32); defaults are
  // launch/opti_node.launch:3-28.
  struct Config {
    int alg = 24;                 // NLopt id; 24 = LD_MMA
    double time_limit_1 = 0.4, time_limit_2 = 0.1;
    double dt = 0.2;              // read but unused by the cost (:8, :351)
    double ws = 1.0, wc = 5.0;
    double alpha = 10.0, r = 0.5, d0 = 0.8;
    double alpha_v = 0.0, r_v = 1.5, v0 = 2.5;
    double alpha_a = 0.0, r_a = 1.5, a0 = 3.5;
    double bos = 3.0, vos = 8.0, aos = 10.0;
    double mean_v = 1.8, mean_a = 0.0, init_time = 0.3;
    // not in the reference: which GPU, whether to run the dyn-feasibility
    // block the reference has commented out (:383-407), and an evaluation cap
    // for reproducible runs (0 = stop on maxtime only, as the reference does).
    int device = 0;
    int enable_dyn = 0;
    int max_evals = 0;
    // 0: the optimizer (csrc/mma.hpp standing in for NLopt's LD_MMA) runs on the host and calls the cost function
    // once per evaluation, as the reference does (:195) — iter_num, total_time and the cost curve are kept per call.
    // 1: the whole optimisation is ONE launch of the batched device optimizer (gtop_optimize_batch_ex, same
    // algorithm, same stop rules); only the evaluation count is reported, the cost curve stays empty.
    int optimize_on_device = 0;
    // the device optimizer's evaluations in fp32 (gtop_set_optimizer_precision; its state and results stay fp64):
    // for large batches through GradTrajBatch; needs the device optimizer (optimize_on_device, or GradTrajBatch)
    int optimizer_fp32 = 0;
    // which gradient the cost function and the device optimizer use (include/gtop.h, gtop_set_gradient_mode):
    // 0 = GTOP_GRADIENT_REFERENCE, the reference's callback line by line (its iterates); 1 = GTOP_GRADIENT_CONSISTENT,
    // the gradient of the cost as returned — the one to optimise with
    int gradient_mode = 0;
    // the start point setPath / setKinoPath leave in Dp (GradTrajBatch::setPaths too): 0 = the reference's — the
    // straight line of PolyQPGeneration(type = 2) in setPath (zero velocity and acceleration at every waypoint), the
    // given derivatives in setKinoPath; 1 = positions, Df and segment times as they are, the interior velocities and
    // accelerations replaced by the minimiser of the smoothness term (include/gtop.h, gtop_min_jerk_start: the
    // reference's type == 1, src/qp_generator.cpp:242-315), the coefficients refreshed from it
    int initial_guess = 0;
    // 1: optimizeTrajectory reallocates the segment times behind the solve, where the reference carries the block
    // commented out (:209-227): segment_time(i) = the distance between waypoints i and i + 1 as the optimizer left
    // them / mean_v, plus init_time on the first and the last segment (include/gtop.h, GTOP_RETIME_LENGTH).  The
    // coefficients getCoefficient returns afterwards are those of the NEW times (the block sits in front of :230), and
    // the next optimizeTrajectory runs on them.  0 (default): the times of setPath / setKinoPath stand, as shipped.
    int reallocate_time = 0;
  };

  GradTrajOptimizer();
  explicit GradTrajOptimizer(const Config &cfg);
  ~GradTrajOptimizer();
  GradTrajOptimizer(const GradTrajOptimizer &) = delete;
  GradTrajOptimizer &operator=(const GradTrajOptimizer &) = delete;

  void setPath(const std::vector<Vec3> &way_points);                      // :67-110
  void setKinoPath(const Matrix &Pos, const Matrix &Vel, const Matrix &Acc,
                   const std::vector<double> &Time);                      // :35-65
  bool optimizeTrajectory(int step);                                      // :128-243
  void getCoefficient(Matrix &coeff);                                     // :245-247
  void getSegmentTime(std::vector<double> &seg_time);                     // :249-251
  void initSDFMap(Vec3 map_size_3d, Vec3 origin, double resolution);      // :112-115
  void updateSDFMap(const std::vector<Vec3> &obs);                        // :117-126
  void getCostCurve(std::vector<double> &cost, std::vector<double> &time);  // header :127-130

  // NLopt-format cost function (:554-562).  Private in the reference; public
  // here so that an external NLopt (or a test) can take its address.
  static double costFunc(const std::vector<double> &x, std::vector<double> &grad, void *func_data);

  // The moving-obstacle cost (include/gtop.h, gtop_set_moving_cost; not in the reference's callback): boxes
  // {p0, vel, scale} — centre p0 + vel t, extent +-scale/2 — and the trajectory's start time on their clock.  A
  // non-empty list switches the mode on for costFunc and optimizeTrajectory (both roads), an empty one off.
  void setMovingObstacles(const std::vector<Vec3> &p0, const std::vector<Vec3> &vel, const std::vector<Vec3> &scale);
  // The same with polynomial predictions (gtop_set_moving_box_polynomials; the reference's PolynomialPrediction,
  // obj_predictor.h:26-55): coef[b] = axis-major 3 x 6 coefficients in ascending powers, t_range[b] = {t1, t2} (empty
  // vector = unbounded; outside its interval a box stands where its prediction ends), scale[b] the extent.
  using Poly3 = std::array<double, 18>;
  void setMovingObstaclePredictions(const std::vector<Poly3> &coef, const std::vector<std::array<double, 2>> &t_range,
                                    const std::vector<Vec3> &scale);
  // The predictions FITTED from observation histories (include/gtop_prediction.h; the reference's ObjPredictor,
  // src/obj_predictor.cpp): the host fit gtop_fit_predictions of histories[b] — samples {x, y, z, t}, oldest first —
  // followed by setMovingObstaclePredictions with the fitted rows and the extents scales[b] + 2 inflate resmax (the
  // half extent gtop_refresh_box_predictions_device writes).  Returns one info row per object (GTOP_PRED_INFO doubles:
  // status, count, degree used, the interval's start, t_last, the interval's end, resmax per axis, rms, two pads).  An
  // object that cannot be fitted (no samples, a non-finite one, times that do not advance) refuses the whole list
  // (ok() is false, the list in force stays); its status in the rows returned tells which.
  struct PredictOptions {
    int mode = 0;            // GTOP_PREDICT_POLYFIT; 1: GTOP_PREDICT_CONST_VEL
    int degree = 5;
    double lambda = 1.0, horizon = 0.0, inflate = 0.0;
    bool regularise_horizon = false;
  };
  using History = std::vector<std::array<double, 4>>;
  using PredictInfo = std::array<double, 12>;
  std::vector<PredictInfo> fitObstaclePredictions(const std::vector<History> &histories, const std::vector<Vec3> &scales,
                                                  const PredictOptions &options);
  void setStartTime(double t0);

  // The safety report of the trajectory at the current Dp (include/gtop.h, gtop_validate_batch; not a method of the
  // reference's class — its planner front end tests motion primitives this way, src/kinodynamic_astar.cpp:178-213):
  // true iff no getTraj sample lies within `margin` of an obstacle (of the boxes of setMovingObstacles too, at
  // start time + sample time, with use_boxes), none lies out of the map unless allowed, and the velocity /
  // acceleration maxima keep to max_vel / max_acc (<= 0: off; per_axis: the largest component, not the norm).
  // false also when the call itself fails (ok() tells the two apart).
  struct Limits {
    double margin = 0.0, max_vel = 0.0, max_acc = 0.0;
    bool per_axis = false, allow_out_of_map = false, use_boxes = false;
    double dt_sample = 0.01;
  };
  struct Report {
    int n_samples = 0;
    double clearance = 0.0, clearance_time = 0.0;
    int clearance_index = -1, n_below_margin = 0;
    double first_below_time = -1.0;
    int n_out_of_map = 0;
    double max_vel_norm = 0.0, max_acc_norm = 0.0, max_vel_axis = 0.0, max_acc_axis = 0.0, time_sum = 0.0;
  };
  bool validateTrajectory(const Limits &limits, Report *report = nullptr);

  // The continuous-time clearance certificate of the trajectory at the current Dp (include/gtop.h,
  // gtop_certify_batch): where validateTrajectory speaks about the getTraj samples, this speaks about every point of
  // the curve — true iff the verdict is SAFE: the interpolated distance of the static field is above `margin` over
  // the whole of [0, time_sum].  The static field alone: certifyTrajectoryMoving below takes the moving obstacles in.
  // false also when the call fails (ok() tells).
  struct CertifyOptions {
    double margin = 0.0;
    int max_depth = 2, max_refine = 256;
  };
  struct CertifyReport {
    int verdict = 0;                                  // -1 UNSAFE, 0 UNDECIDED, +1 SAFE
    double lo = 0.0, hi = 0.0, hi_time = 0.0;         // certified lower bound; least midpoint distance and its time
    double first_violation_time = -1.0;
    int n_undecided = 0, n_refinements = 0;
    double time_sum = 0.0;
  };
  bool certifyTrajectory(const CertifyOptions &options, CertifyReport &report);
  // The same against the static field AND the boxes of setMovingObstacles / setMovingObstaclePredictions at
  // setStartTime's clock (include/gtop.h, gtop_certify_moving_batch): true iff SAFE — every point of the curve keeps
  // `margin` from the field and from every box at the time the curve is there.  Without boxes: certifyTrajectory.
  bool certifyTrajectoryMoving(const CertifyOptions &options, CertifyReport &report);
  // The continuous-time KINEMATIC certificate of the trajectory at the current Dp (include/gtop_kinematics.h,
  // gtop_certify_kinematics_batch): where Report's max_vel_* / max_acc_* are maxima over the getTraj samples, ub_* here
  // bound the figure over the whole of [0, time_sum] — true iff the verdict is WITHIN: the chosen figures (the norms, or
  // under per_axis the largest |component|) keep max_vel / max_acc at every time.  A limit <= 0 is off.  false also
  // when the call fails (ok() tells).
  struct KinematicOptions {
    double max_vel = 0.0, max_acc = 0.0;
    bool per_axis = false;
    int max_depth = 2, max_refine = 256;
  };
  struct KinematicReport {
    int verdict = 0;                                   // -1 EXCEEDS, 0 UNDECIDED, +1 WITHIN
    double ub_vel = 0.0, lo_vel = 0.0, lo_vel_time = 0.0;   // certified upper bound; largest midpoint figure and its time
    double ub_acc = 0.0, lo_acc = 0.0, lo_acc_time = 0.0;
    double first_violation_time = -1.0;
    int n_undecided = 0, n_refinements = 0;
    double time_sum = 0.0;
  };
  bool certifyKinematics(const KinematicOptions &options, KinematicReport &report);

  // The same figures per SEGMENT (include/gtop.h, gtop_validate_segments): rows->at(s) covers the getTraj samples that
  // fall into segment s; of `limits` margin, use_boxes and dt_sample are read.  false when the call fails.
  struct SegmentReport {
    int n_samples = 0, first_sample = -1;         // a segment without samples: 0, -1, clearance +inf, time -1, zeros
    double clearance = 0.0, clearance_time = -1.0;
    int n_below_margin = 0, n_out_of_map = 0;
    double max_vel_norm = 0.0, max_acc_norm = 0.0, max_vel_axis = 0.0, max_acc_axis = 0.0;
  };
  bool segmentReport(const Limits &limits, std::vector<SegmentReport> *rows);
  // New segment times from the trajectory at the current Dp (include/gtop.h, gtop_reallocate_times): by waypoint
  // distance (GTOP_RETIME_LENGTH, the reference's commented block :209-227; mean_v / init_time < 0: the Config's) or by
  // stretching the segments whose velocity / acceleration breaks max_vel / max_acc (GTOP_RETIME_LIMITS; the report
  // is formed with `report`'s margin, use_boxes and dt_sample).  The new times become the object's segment_time — what
  // getSegmentTime returns and the next optimizeTrajectory runs on —, Dp is rescaled under scale_x, the coefficients
  // are refreshed.  false, and nothing changed, when the call fails.
  struct RetimeOptions {
    int mode = GTOP_RETIME_LIMITS;
    double mean_v = -1.0, init_time = -1.0;
    double max_vel = 0.0, max_acc = 0.0;
    bool per_axis = false, uniform = false, scale_x = false;
    double max_ratio = 4.0;
    Limits report;
  };
  bool reallocateSegmentTime(const RetimeOptions &options);
  // One more waypoint on the trajectory at the current Dp (include/gtop.h, gtop_insert_waypoints): the segment that
  // holds trajectory time `when` (GTOP_INSERT_AT_TIME — a Report's clearance_time, a CertifyReport's hi_time or
  // first_violation_time; a time that is not in [0, inf) falls back to LONGEST) or the longest segment
  // (GTOP_INSERT_LONGEST) is cut in two, the new junction takes the curve's position, velocity and acceleration there
  // and, with push > 0 where the static distance is below push_below, is moved `push` up the field's gradient.  The
  // object's path, Dp, segment_time and segment count become the new problem of one segment more — what
  // optimizeTrajectory runs on next, its bounds around the new waypoint as around the others — and the coefficients
  // are refreshed: without a push the curve is the old one.  false, and nothing changed, when the call fails.
  struct InsertOptions {
    int mode = GTOP_INSERT_LONGEST;
    double when = -1.0;
    double min_fraction = 0.1;          // the cut keeps this share of the segment on either side
    double push = 0.0, push_below = 0.0;
  };
  struct InsertInfo {
    int segment = -1;                   // the segment that was cut
    double local_time = 0.0;            // where, in its own time
    bool fell_back = false, clamped = false, pushed = false;
    double distance = 0.0;              // the static distance at the new waypoint before the push (0 when push is off)
  };
  bool insertWaypoint(const InsertOptions &options, InsertInfo *info = nullptr);
  // The derivative of the cost with respect to every segment time at the current Dp and segment_time
  // (include/gtop_time.h, gtop_time_gradient_batch): the callback's cost at the parameters the last optimizeTrajectory
  // left in force, gT[s] = d cost / d T_s, and (given) per segment the smoothness and collision + dyn cost and their
  // two derivatives.  false when the call fails.
  bool timeGradient(double *cost, std::vector<double> *gT, std::vector<std::array<double, 4>> *parts = nullptr);
  // New segment times by minimising cost + rho sum(T) over them at the current Dp (include/gtop_time.h,
  // gtop_optimize_times): a projected gradient descent with backtracking on the device.  keep_limits: the times of
  // reallocateSegmentTime(limits) at the current trajectory are the lower bounds — never faster than max_vel / max_acc
  // allow.  The new times become the object's segment_time — what getSegmentTime returns and the next
  // optimizeTrajectory runs on —, the coefficients are refreshed.  false, and nothing changed, when the call fails.
  struct TimeOptConfig {
    double rho = 1.0;
    double t_min = 0.05, t_max = 60.0;
    double first_move = 0.05;
    double ftol_rel = 1e-6, xtol_abs = 1e-9;
    int max_evals = 40;
    bool keep_limits = false;
    RetimeOptions limits;
  };
  struct TimeOptInfo {
    int code = 0, accepted = 0, evaluations = 0;   // 3 FTOL, 4 XTOL, 5 MAXEVAL
    double f_start = 0.0, f = 0.0, cost = 0.0, free_gradient = 0.0, time_sum = 0.0;
  };
  bool optimizeSegmentTimes(const TimeOptConfig &config, TimeOptInfo *info = nullptr);
  // The two calls above under the moving-obstacle cost (include/gtop_time_moving.h, gtop_time_gradient_moving_batch
  // and gtop_optimize_times_moving), which the two above refuse while setMovingObstacles / setMovingObstaclePredictions
  // have the mode on: the cost and its derivative see the boxes at setStartTime's clock, where a segment time moves
  // the lookups of every later segment.  gt0 (given): d cost / d start time.  parts: the four columns of timeGradient,
  // then q_s (what the segment's cost gains per second of delay of its start) and the sum of q over the later
  // segments.  Without boxes they give what the two above give.
  bool timeGradientMoving(double *cost, std::vector<double> *gT, double *gt0 = nullptr,
                          std::vector<std::array<double, 6>> *parts = nullptr);
  bool optimizeSegmentTimesMoving(const TimeOptConfig &config, TimeOptInfo *info = nullptr);
  // The cost with its derivative with respect to every free waypoint value (gx, laid out as Dp, axis-major) and every
  // segment time (gT) from one pass (include/gtop_joint.h, gtop_joint_gradient_batch), at the current Dp and
  // segment_time and the parameters the last optimizeTrajectory left in force.  false when the call fails.
  bool jointGradient(double *cost, std::vector<double> *gx, std::vector<double> *gT,
                     std::vector<std::array<double, 4>> *parts = nullptr);
  // Dp and the segment times optimised TOGETHER: cost + rho sum(T) minimised over both by the batched MMA loop
  // (include/gtop_joint.h, gtop_optimize_joint) inside optimizeTrajectory's bounds on Dp and t_min .. t_max on the times;
  // keep_limits as in TimeOptConfig.  Dp, segment_time and the coefficients are replaced.  false, and nothing changed,
  // when the call fails.
  struct JointOptConfig {
    double rho = 1.0;
    double t_min = 0.05, t_max = 60.0;
    double ftol_rel = 0.0, xtol_rel = 0.0;
    int max_evals = 40;
    bool keep_limits = false;
    RetimeOptions limits;
  };
  struct JointOptInfo {
    int code = 0, evaluations = 0;   // 3 FTOL, 4 XTOL, 5 MAXEVAL
    double f_start = 0.0, f = 0.0, cost = 0.0, time_sum = 0.0, free_gradient_x = 0.0, free_gradient_t = 0.0;
  };
  bool optimizeJoint(const JointOptConfig &config, JointOptInfo *info = nullptr);
  // The robots of a swarm, one object each, planned against each other (include/gtop_swarm.h).  Their paths must have
  // the same number of segments.  Both calls run on the FIRST object's context: its map, and the parameters its last
  // optimizeTrajectory left in force; that context's problem is the swarm for the length of the call and the object's
  // own again afterwards.  The start times are that context's.
  struct SwarmOptions {
    double t_lo = 0.0, dt = 0.05;   // the common grid tau_k = t_lo + k dt
    int n_samples = 256;
    double w = 1.0, radius = 1.0;   // the weight of the term and the radius of interaction
    bool hold_ends = true;          // a robot stands at its start before and at its end after its flight
    int sweeps = 4, evals_per_sweep = 25;   // optimizeSwarm's stop rules
  };
  // gtop_swarm_gradient_batch at every robot's current Dp: S[b], the penalty of robot b against the others, grad[b], its
  // derivative with respect to robot b's Dp (axis-major), and (given) active[b], the number of active terms.  The swarm's
  // total is sum(S) / 2.  false when the call fails.
  static bool swarmGradient(const std::vector<GradTrajOptimizer *> &robots, const SwarmOptions &options,
                            std::vector<double> *S, std::vector<std::vector<double>> *grad,
                            std::vector<double> *active = nullptr);
  // gtop_optimize_swarm from every robot's current Dp inside the bounds optimizeTrajectory uses: in every sweep each
  // robot minimises its own cost plus its penalty against the plans the others had at the sweep's start.  The results
  // become the objects' Dp and coefficients.  min_cost[b] (given): the last sweep's least cost + penalty; joint[b]
  // (given): {the robot's own cost, its penalty with the others unfrozen} at the result.  false, and nothing changed,
  // when the call fails.
  static bool optimizeSwarm(const std::vector<GradTrajOptimizer *> &robots, const SwarmOptions &options,
                            std::vector<double> *min_cost = nullptr, std::vector<std::array<double, 2>> *joint = nullptr);

  // extras (not in the reference)
  bool ok() const { return ctx_ != nullptr && last_status_ == GTOP_OK; }
  const char *lastError() const;
  gtop_ctx *context() { return ctx_; }
  const std::vector<double> &freeDerivatives() const { return dp_; }      // Dp, axis-major
  int iterations() const { return last_evals_; }

 private:
  void setupProblem(const std::vector<double> &path_flat, int npts, const std::vector<double> &seg_time,
                    const std::vector<double> &Dx, const std::vector<double> &Dy, const std::vector<double> &Dz);
  void pushParams();
  void coefficientsFromDerivatives(const std::vector<double> &dp);        // :253-279
  // the swarm as the first object's problem: the call's status (the first object's last_status_)
  static bool swarmProblem(const std::vector<GradTrajOptimizer *> &robots, const SwarmOptions &options,
                           gtop_swarm_opts *opt, std::vector<double> *x);
  void ownProblem();   // this object's problem back on its context
  // optimizeSegmentTimes (gtop_optimize_times) or, moving, optimizeSegmentTimesMoving (gtop_optimize_times_moving)
  bool optimizeSegmentTimesWith(const TimeOptConfig &config, TimeOptInfo *info, bool moving);

  Config cfg_;
  gtop_ctx *ctx_ = nullptr;
  int last_status_ = GTOP_OK;
  std::string create_error_;

  int m_ = 0, num_dp_ = 0;
  int step_ = 1;
  std::vector<double> path_;          // npts x 3
  std::vector<double> segment_time_;  // m
  std::vector<double> df_;            // 3 x 6
  std::vector<double> dp_;            // 3 x num_dp, axis-major == NLopt x
  Matrix coeff_;                      // m x 18
  int last_evals_ = 0;
};

// ---------------------------------------------------------------------------
// GradTrajBatch — the same public steps for MANY trajectories at once, on one or several GPUs (not in the reference,
// which optimises one trajectory per object: a planner that holds N candidate paths runs N objects one after the other).
// initSDFMap / updateSDFMap / setPaths / optimizeTrajectories / getCoefficient mirror GradTrajOptimizer's methods with a
// batch index; underneath is a gtop_group (include/gtop.h): the distance field replicated on every listed device, the
// batch in contiguous slices, the whole optimisation of a slice ONE launch on its device.
// ---------------------------------------------------------------------------
class GradTrajBatch {
 public:
  // devices: HIP ordinals, one slice of the batch each (an ordinal may repeat); cfg as for GradTrajOptimizer
  explicit GradTrajBatch(const std::vector<int> &devices, const GradTrajOptimizer::Config &cfg = GradTrajOptimizer::Config());
  ~GradTrajBatch();
  GradTrajBatch(const GradTrajBatch &) = delete;
  GradTrajBatch &operator=(const GradTrajBatch &) = delete;

  void initSDFMap(Vec3 map_size_3d, Vec3 origin, double resolution);
  void updateSDFMap(const std::vector<Vec3> &obs);
  // B waypoint lists of m_b + 1 >= 3 points each — the lengths may differ (candidate paths of a planner seldom have the
  // same number of waypoints): segment times, Df and the straight-line start as GradTrajOptimizer::setPath makes
  // them (src/grad_traj_optimizer.cpp:67-110); trajectories of equal segment count form one device problem
  void setPaths(const std::vector<std::vector<Vec3>> &way_points);
  // every trajectory's LD_MMA run (:128-243), all at once; stop rules: cfg.max_evals and the step's time limit
  bool optimizeTrajectories(int step);
  void getCoefficient(int b, Matrix &coeff) const;               // trajectory b, m_b x 18
  int segments(int b) const { return (b >= 0 && b < B_) ? m_of_[b] : 0; }
  const std::vector<double> &costs() const { return min_cost_; }  // the minimum each trajectory reached
  const std::vector<int> &evaluations() const { return nevals_; }
  int size() const { return B_; }
  int devices() const;
  const char *gatherBackend() const;                              // "rccl" / "copy" (gtop_group_gather_backend)
  bool ok() const { return grp_ != nullptr && last_status_ == GTOP_OK; }
  const char *lastError() const;

 private:
  GradTrajOptimizer::Config cfg_;
  gtop_group *grp_ = nullptr;
  int last_status_ = GTOP_OK;
  int B_ = 0;
  // per trajectory: segment count and where its rows start in the flat arrays (waypoints x 3, times, free variables)
  std::vector<int> m_of_;
  std::vector<size_t> path_at_, T_at_, x_at_;
  std::vector<double> path_, T_, Df_, x_, min_cost_;
  std::vector<int> nevals_;
};

}  // namespace gtop_amd

#endif  // GTOP_AMD_GRAD_TRAJ_OPTIMIZER_HPP_
