// grad_traj_optimizer.cpp — host shim over the C-ABI (see the header).
// file:line citations are into EpicOne1/grad_traj_optimization.
#include "grad_traj_optimizer.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "mma.hpp"

namespace gtop_amd {

namespace {

// Coefficients of one quintic segment from its boundary derivatives
// [p0, pT, v0, vT, a0, aT] and duration T: the closed form of A_s^-1 d
// (A_s: src/qp_generator.cpp:185-195; the reference forms A.inverse(), :334-336, :390).
void quintic_from_boundary(const double d[6], double T, double c[6]) {
  const double p0 = d[0], pT = d[1], v0 = d[2], vT = d[3], a0 = d[4], aT = d[5];
  const double T2 = T * T, iT = 1.0 / T, iT3 = iT * iT * iT;
  const double P = pT - p0 - v0 * T - 0.5 * a0 * T2;
  const double V = (vT - v0 - a0 * T) * T;
  const double A = (aT - a0) * T2;
  c[0] = p0;
  c[1] = v0;
  c[2] = 0.5 * a0;
  c[3] = (10 * P - 4 * V + 0.5 * A) * iT3;
  c[4] = (-15 * P + 7 * V - A) * (iT3 * iT);
  c[5] = (6 * P - 3 * V + 0.5 * A) * (iT3 * iT * iT);
}

double nlopt_trampoline(unsigned n, const double *x, double *grad, void *data) {
  return gtop_cost_nlopt(n, x, grad, data);
}

}  // namespace

GradTrajOptimizer::GradTrajOptimizer() : GradTrajOptimizer(Config()) {}

GradTrajOptimizer::GradTrajOptimizer(const Config &cfg) : cfg_(cfg) {
  last_status_ = gtop_create(&ctx_, cfg_.device);
  if (last_status_ != GTOP_OK) {
    create_error_ = gtop_last_error(nullptr);
    ctx_ = nullptr;
    return;
  }
  pushParams();
}

GradTrajOptimizer::~GradTrajOptimizer() {
  if (ctx_) gtop_destroy(ctx_);
}

const char *GradTrajOptimizer::lastError() const {
  return ctx_ ? gtop_last_error(ctx_) : create_error_.c_str();
}

void GradTrajOptimizer::pushParams() {
  if (!ctx_) return;
  gtop_params p;
  p.ws = cfg_.ws; p.wc = cfg_.wc;
  p.alpha = cfg_.alpha; p.r = cfg_.r; p.d0 = cfg_.d0;
  p.alpha_v = cfg_.alpha_v; p.r_v = cfg_.r_v; p.v0 = cfg_.v0;
  p.alpha_a = cfg_.alpha_a; p.r_a = cfg_.r_a; p.a0 = cfg_.a0;
  p.step = step_;
  p.enable_dyn = cfg_.enable_dyn;
  last_status_ = gtop_set_params(ctx_, &p);
  if (last_status_ == GTOP_OK) last_status_ = gtop_set_gradient_mode(ctx_, cfg_.gradient_mode);
}

void GradTrajOptimizer::initSDFMap(Vec3 map_size_3d, Vec3 origin, double resolution) {
  if (!ctx_) return;
  last_status_ = gtop_init_sdf_map(ctx_, map_size_3d.data(), origin.data(), resolution);
}

void GradTrajOptimizer::updateSDFMap(const std::vector<Vec3> &obs) {
  if (!ctx_) return;
  // std::array<double,3> is layout-compatible with xyz triples
  last_status_ = gtop_update_sdf_map(ctx_, obs.empty() ? nullptr : obs[0].data(), (int)obs.size());
}

void GradTrajOptimizer::setMovingObstacles(const std::vector<Vec3> &p0, const std::vector<Vec3> &vel,
                                           const std::vector<Vec3> &scale) {
  if (!ctx_) return;
  if (p0.size() != vel.size() || p0.size() != scale.size()) {
    last_status_ = GTOP_ERR_INVALID;
    return;
  }
  const int nbox = (int)p0.size();
  last_status_ = gtop_set_moving_boxes(ctx_, nbox, nbox ? p0[0].data() : nullptr, nbox ? vel[0].data() : nullptr,
                                       nbox ? scale[0].data() : nullptr);
  if (last_status_ == GTOP_OK) last_status_ = gtop_set_moving_cost(ctx_, nbox > 0);
}

void GradTrajOptimizer::setMovingObstaclePredictions(const std::vector<Poly3> &coef,
                                                     const std::vector<std::array<double, 2>> &t_range,
                                                     const std::vector<Vec3> &scale) {
  if (!ctx_) return;
  if (coef.size() != scale.size() || (!t_range.empty() && t_range.size() != coef.size())) {
    last_status_ = GTOP_ERR_INVALID;
    return;
  }
  const int nbox = (int)coef.size();
  last_status_ = gtop_set_moving_box_polynomials(ctx_, nbox, nbox ? coef[0].data() : nullptr,
                                                 t_range.empty() ? nullptr : t_range[0].data(),
                                                 nbox ? scale[0].data() : nullptr);
  if (last_status_ == GTOP_OK) last_status_ = gtop_set_moving_cost(ctx_, nbox > 0);
}

std::vector<GradTrajOptimizer::PredictInfo> GradTrajOptimizer::fitObstaclePredictions(
    const std::vector<History> &histories, const std::vector<Vec3> &scales, const PredictOptions &options) {
  static_assert(GTOP_PRED_INFO == 12, "PredictInfo is one info row");
  const int N = (int)histories.size();
  std::vector<PredictInfo> info((size_t)N);
  if (!ctx_) return info;
  if (scales.size() != histories.size()) {
    last_status_ = GTOP_ERR_INVALID;
    return info;
  }
  size_t H = 1;
  for (const History &h : histories) H = std::max(H, h.size());
  std::vector<double> hist((size_t)N * H * 4, 0.0);
  std::vector<int32_t> count((size_t)N);
  for (int b = 0; b < N; ++b) {
    count[b] = (int32_t)histories[b].size();
    for (size_t i = 0; i < histories[b].size(); ++i)
      std::copy(histories[b][i].begin(), histories[b][i].end(), hist.begin() + ((size_t)b * H + i) * 4);
  }
  gtop_predict_opts o{};
  o.mode = options.mode;
  o.degree = options.degree;
  o.lambda = options.lambda;
  o.horizon = options.horizon;
  o.inflate = options.inflate;
  o.regularise_horizon = options.regularise_horizon;
  std::vector<Poly3> coef((size_t)N);
  std::vector<std::array<double, 2>> t_range((size_t)N);
  last_status_ = gtop_fit_predictions(N, (int)H, hist.data(), count.data(), nullptr, &o, N ? coef[0].data() : nullptr,
                                      N ? t_range[0].data() : nullptr, N ? info[0].data() : nullptr, nullptr);
  if (last_status_ != GTOP_OK) return info;
  std::vector<Vec3> scale(scales);
  for (int b = 0; b < N; ++b) {
    if (info[b][0] != GTOP_PRED_OK && info[b][0] != GTOP_PRED_LOWERED) {
      last_status_ = GTOP_ERR_INVALID;
      return info;
    }
    for (int k = 0; k < 3; ++k) {
      const double grow = options.inflate * info[b][6 + k];   // (its own statement: rounded before it is added)
      scale[b][k] = 2.0 * (0.5 * scales[b][k] + grow);
    }
  }
  setMovingObstaclePredictions(coef, t_range, scale);
  return info;
}

void GradTrajOptimizer::setStartTime(double t0) {
  if (!ctx_) return;
  last_status_ = gtop_set_start_times(ctx_, 1, &t0);
}

bool GradTrajOptimizer::validateTrajectory(const Limits &limits, Report *report) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_limits lim{};
  lim.margin = limits.margin;
  lim.max_vel = limits.max_vel;
  lim.max_acc = limits.max_acc;
  lim.per_axis = limits.per_axis;
  lim.allow_out_of_map = limits.allow_out_of_map;
  lim.use_boxes = limits.use_boxes;
  double r[GTOP_TRAJ_REPORT];
  const double cost = 0.0;   // one candidate: the selection is the pass test alone
  unsigned char pass = 0;
  int32_t best[2] = {-1, 0};
  last_status_ = gtop_validate_batch(ctx_, 1, dp_.data(), limits.dt_sample, &lim, &cost, r, &pass, best);
  if (last_status_ != GTOP_OK) return false;
  if (report) {
    report->n_samples = (int)r[0];
    report->clearance = r[1];
    report->clearance_time = r[2];
    report->clearance_index = (int)r[3];
    report->n_below_margin = (int)r[4];
    report->first_below_time = r[5];
    report->n_out_of_map = (int)r[6];
    report->max_vel_norm = r[7];
    report->max_acc_norm = r[8];
    report->max_vel_axis = r[9];
    report->max_acc_axis = r[10];
    report->time_sum = r[11];
  }
  return pass != 0;
}

// a row of GTOP_CERT_REPORT doubles as a CertifyReport
static void fill_certify_report(const double *r, GradTrajOptimizer::CertifyReport &report) {
  report.verdict = (int)r[0];
  report.lo = r[1];
  report.hi = r[2];
  report.hi_time = r[3];
  report.first_violation_time = r[4];
  report.n_undecided = (int)r[5];
  report.n_refinements = (int)r[6];
  report.time_sum = r[7];
}

bool GradTrajOptimizer::certifyTrajectory(const CertifyOptions &options, CertifyReport &report) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_certify_opts opt{};
  opt.margin = options.margin;
  opt.max_depth = options.max_depth;
  opt.max_refine = options.max_refine;
  double r[GTOP_CERT_REPORT];
  last_status_ = gtop_certify_batch(ctx_, 1, dp_.data(), &opt, r);
  if (last_status_ != GTOP_OK) return false;
  fill_certify_report(r, report);
  return report.verdict == 1;
}

bool GradTrajOptimizer::certifyTrajectoryMoving(const CertifyOptions &options, CertifyReport &report) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_certify_moving_opts opt{};
  opt.margin = options.margin;
  opt.max_depth = options.max_depth;
  opt.max_refine = options.max_refine;
  opt.use_boxes = 1;
  double r[GTOP_CERT_REPORT];
  last_status_ = gtop_certify_moving_batch(ctx_, 1, dp_.data(), &opt, r);
  if (last_status_ != GTOP_OK) return false;
  fill_certify_report(r, report);
  return report.verdict == 1;
}

bool GradTrajOptimizer::certifyKinematics(const KinematicOptions &options, KinematicReport &report) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_kin_opts opt{};
  opt.max_vel = options.max_vel;
  opt.max_acc = options.max_acc;
  opt.per_axis = options.per_axis ? 1 : 0;
  opt.max_depth = options.max_depth;
  opt.max_refine = options.max_refine;
  double r[GTOP_KIN_REPORT];
  last_status_ = gtop_certify_kinematics_batch(ctx_, 1, dp_.data(), &opt, r, nullptr);
  if (last_status_ != GTOP_OK) return false;
  report.verdict = (int)r[0];
  report.ub_vel = r[1];
  report.lo_vel = r[2];
  report.lo_vel_time = r[3];
  report.ub_acc = r[4];
  report.lo_acc = r[5];
  report.lo_acc_time = r[6];
  report.first_violation_time = r[7];
  report.n_undecided = (int)r[8];
  report.n_refinements = (int)r[9];
  report.time_sum = r[10];
  return report.verdict == 1;
}

bool GradTrajOptimizer::segmentReport(const Limits &limits, std::vector<SegmentReport> *rows) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_limits lim{};
  lim.margin = limits.margin;
  lim.use_boxes = limits.use_boxes;
  std::vector<double> r((size_t)m_ * GTOP_SEG_REPORT);
  last_status_ = gtop_validate_segments(ctx_, 1, dp_.data(), limits.dt_sample, &lim, r.data());
  if (last_status_ != GTOP_OK) return false;
  if (rows) {
    rows->resize(m_);
    for (int s = 0; s < m_; ++s) {
      const double *q = &r[(size_t)s * GTOP_SEG_REPORT];
      SegmentReport &o = (*rows)[s];
      o.n_samples = (int)q[0];
      o.first_sample = (int)q[1];
      o.clearance = q[2];
      o.clearance_time = q[3];
      o.n_below_margin = (int)q[4];
      o.n_out_of_map = (int)q[5];
      o.max_vel_norm = q[6];
      o.max_acc_norm = q[7];
      o.max_vel_axis = q[8];
      o.max_acc_axis = q[9];
    }
  }
  return true;
}

bool GradTrajOptimizer::reallocateSegmentTime(const RetimeOptions &options) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_retime opt{};
  opt.mode = options.mode;
  opt.mean_v = options.mean_v < 0.0 ? cfg_.mean_v : options.mean_v;
  opt.init_time = options.init_time < 0.0 ? cfg_.init_time : options.init_time;
  opt.max_vel = options.max_vel;
  opt.max_acc = options.max_acc;
  opt.per_axis = options.per_axis;
  opt.uniform = options.uniform;
  opt.scale_x = options.scale_x;
  opt.max_ratio = options.max_ratio;
  gtop_limits lim{};
  lim.margin = options.report.margin;
  lim.use_boxes = options.report.use_boxes;
  std::vector<double> T(m_), x = dp_;
  last_status_ = gtop_reallocate_times(ctx_, &opt, 1, x.data(), options.report.dt_sample, &lim, T.data());
  if (last_status_ != GTOP_OK) return false;
  last_status_ = gtop_set_problem(ctx_, 1, m_, T.data(), m_, df_.data());   // (refuses a time that is not > 0)
  if (last_status_ != GTOP_OK) return false;
  segment_time_ = T;
  dp_ = x;
  coefficientsFromDerivatives(dp_);
  return true;
}

bool GradTrajOptimizer::timeGradient(double *cost, std::vector<double> *gT, std::vector<std::array<double, 4>> *parts) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  double c = 0.0;
  std::vector<double> g(m_), p(parts ? (size_t)m_ * GTOP_TIME_PARTS : 0);
  last_status_ = gtop_time_gradient_batch(ctx_, 1, dp_.data(), &c, g.data(), parts ? p.data() : nullptr);
  if (last_status_ != GTOP_OK) return false;
  if (cost) *cost = c;
  if (gT) *gT = g;
  if (parts) {
    parts->resize(m_);
    for (int s = 0; s < m_; ++s)
      for (int k = 0; k < GTOP_TIME_PARTS; ++k) (*parts)[s][k] = p[(size_t)s * GTOP_TIME_PARTS + k];
  }
  return true;
}

bool GradTrajOptimizer::timeGradientMoving(double *cost, std::vector<double> *gT, double *gt0,
                                           std::vector<std::array<double, 6>> *parts) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  double c = 0.0, g0 = 0.0;
  std::vector<double> g(m_), p(parts ? (size_t)m_ * GTOP_TIME_MOVING_PARTS : 0);
  last_status_ = gtop_time_gradient_moving_batch(ctx_, 1, dp_.data(), &c, g.data(), &g0, parts ? p.data() : nullptr);
  if (last_status_ != GTOP_OK) return false;
  if (cost) *cost = c;
  if (gT) *gT = g;
  if (gt0) *gt0 = g0;
  if (parts) {
    parts->resize(m_);
    for (int s = 0; s < m_; ++s)
      for (int k = 0; k < GTOP_TIME_MOVING_PARTS; ++k) (*parts)[s][k] = p[(size_t)s * GTOP_TIME_MOVING_PARTS + k];
  }
  return true;
}

bool GradTrajOptimizer::optimizeSegmentTimes(const TimeOptConfig &config, TimeOptInfo *info) {
  return optimizeSegmentTimesWith(config, info, false);
}

bool GradTrajOptimizer::optimizeSegmentTimesMoving(const TimeOptConfig &config, TimeOptInfo *info) {
  return optimizeSegmentTimesWith(config, info, true);
}

bool GradTrajOptimizer::optimizeSegmentTimesWith(const TimeOptConfig &config, TimeOptInfo *info, bool moving) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_timeopt opt{};
  opt.rho = config.rho;
  opt.t_min = config.t_min;
  opt.t_max = config.t_max;
  opt.first_move = config.first_move;
  opt.ftol_rel = config.ftol_rel;
  opt.xtol_abs = config.xtol_abs;
  opt.max_evals = config.max_evals;
  std::vector<double> lo;
  if (config.keep_limits) {   // the LIMITS reallocation of the trajectory as it stands, Dp untouched
    gtop_retime rt{};
    rt.mode = GTOP_RETIME_LIMITS;
    rt.max_vel = config.limits.max_vel;
    rt.max_acc = config.limits.max_acc;
    rt.per_axis = config.limits.per_axis;
    rt.uniform = config.limits.uniform;
    rt.max_ratio = config.limits.max_ratio;
    gtop_limits lim{};
    lim.margin = config.limits.report.margin;
    lim.use_boxes = config.limits.report.use_boxes;
    lo.resize(m_);
    std::vector<double> x = dp_;
    last_status_ = gtop_reallocate_times(ctx_, &rt, 1, x.data(), config.limits.report.dt_sample, &lim, lo.data());
    if (last_status_ != GTOP_OK) return false;
  }
  std::vector<double> T(m_);
  double r[GTOP_TIMEOPT_INFO];
  last_status_ = (moving ? gtop_optimize_times_moving : gtop_optimize_times)(ctx_, &opt, 1, dp_.data(),
                                                                             lo.empty() ? nullptr : lo.data(), T.data(), r);
  if (last_status_ != GTOP_OK) return false;
  last_status_ = gtop_set_problem(ctx_, 1, m_, T.data(), m_, df_.data());   // (refuses a time that is not > 0)
  if (last_status_ != GTOP_OK) return false;
  segment_time_ = T;
  coefficientsFromDerivatives(dp_);
  if (info) {
    info->code = (int)r[0];
    info->accepted = (int)r[1];
    info->evaluations = (int)r[2];
    info->f_start = r[3];
    info->f = r[4];
    info->cost = r[5];
    info->free_gradient = r[6];
    info->time_sum = r[7];
  }
  return true;
}

bool GradTrajOptimizer::jointGradient(double *cost, std::vector<double> *gx, std::vector<double> *gT,
                                      std::vector<std::array<double, 4>> *parts) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  double c = 0.0;
  std::vector<double> g(dp_.size()), t(m_), p(parts ? (size_t)m_ * GTOP_TIME_PARTS : 0);
  last_status_ = gtop_joint_gradient_batch(ctx_, 1, dp_.data(), &c, g.data(), t.data(), parts ? p.data() : nullptr);
  if (last_status_ != GTOP_OK) return false;
  if (cost) *cost = c;
  if (gx) *gx = g;
  if (gT) *gT = t;
  if (parts) {
    parts->resize(m_);
    for (int s = 0; s < m_; ++s)
      for (int k = 0; k < GTOP_TIME_PARTS; ++k) (*parts)[s][k] = p[(size_t)s * GTOP_TIME_PARTS + k];
  }
  return true;
}

bool GradTrajOptimizer::optimizeJoint(const JointOptConfig &config, JointOptInfo *info) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_jointopt opt{};
  opt.rho = config.rho;
  opt.t_min = config.t_min;
  opt.t_max = config.t_max;
  opt.ftol_rel = config.ftol_rel;
  opt.xtol_rel = config.xtol_rel;
  opt.max_evals = config.max_evals;
  std::vector<double> lo;
  if (config.keep_limits) {   // the LIMITS reallocation of the trajectory as it stands, Dp untouched
    gtop_retime rt{};
    rt.mode = GTOP_RETIME_LIMITS;
    rt.max_vel = config.limits.max_vel;
    rt.max_acc = config.limits.max_acc;
    rt.per_axis = config.limits.per_axis;
    rt.uniform = config.limits.uniform;
    rt.max_ratio = config.limits.max_ratio;
    gtop_limits lim{};
    lim.margin = config.limits.report.margin;
    lim.use_boxes = config.limits.report.use_boxes;
    lo.resize(m_);
    std::vector<double> x = dp_;
    last_status_ = gtop_reallocate_times(ctx_, &rt, 1, x.data(), config.limits.report.dt_sample, &lim, lo.data());
    if (last_status_ != GTOP_OK) return false;
  }
  const size_t n = dp_.size();
  std::vector<double> x = dp_, lb(n), ub(n), T(m_);   // the bounds of optimizeTrajectory, :151-179
  for (int i = 0; i < num_dp_; ++i)
    for (int a = 0; a < 3; ++a) {
      const size_t j = (size_t)i + (size_t)a * num_dp_;
      const double centre = i % 3 == 0 ? path_[(i / 3 + 1) * 3 + a] : 0.0;
      const double half = i % 3 == 0 ? cfg_.bos : (i % 3 == 1 ? cfg_.vos : cfg_.aos);
      lb[j] = centre - half;
      ub[j] = centre + half;
    }
  double r[GTOP_JOINT_INFO];
  gtop_set_optimizer_precision(ctx_, GTOP_F64);
  last_status_ = gtop_optimize_joint(ctx_, &opt, 1, x.data(), lb.data(), ub.data(), lo.empty() ? nullptr : lo.data(),
                                     T.data(), r);
  if (last_status_ != GTOP_OK) return false;
  last_status_ = gtop_set_problem(ctx_, 1, m_, T.data(), m_, df_.data());   // (refuses a time that is not > 0)
  if (last_status_ != GTOP_OK) return false;
  segment_time_ = T;
  dp_ = x;
  coefficientsFromDerivatives(dp_);
  if (info) {
    info->code = (int)r[0];
    info->evaluations = (int)r[1];
    info->f_start = r[2];
    info->f = r[3];
    info->cost = r[4];
    info->time_sum = r[5];
    info->free_gradient_x = r[6];
    info->free_gradient_t = r[7];
  }
  return true;
}

bool GradTrajOptimizer::swarmProblem(const std::vector<GradTrajOptimizer *> &robots, const SwarmOptions &options,
                                     gtop_swarm_opts *opt, std::vector<double> *x) {
  if (robots.empty() || !robots[0]) return false;
  GradTrajOptimizer &lead = *robots[0];
  const int m = lead.m_;
  for (const GradTrajOptimizer *r : robots)
    if (!r || !r->ctx_ || r->m_ < 2 || r->m_ != m || r->dp_.empty()) {
      lead.last_status_ = GTOP_ERR_STATE;
      return false;
    }
  *opt = gtop_swarm_opts{};
  opt->t_lo = options.t_lo;
  opt->dt = options.dt;
  opt->w = options.w;
  opt->radius = options.radius;
  opt->n_samples = options.n_samples;
  opt->hold_ends = options.hold_ends ? 1 : 0;
  std::vector<double> T, Df;
  x->clear();
  for (const GradTrajOptimizer *r : robots) {
    T.insert(T.end(), r->segment_time_.begin(), r->segment_time_.end());
    Df.insert(Df.end(), r->df_.begin(), r->df_.end());
    x->insert(x->end(), r->dp_.begin(), r->dp_.end());
  }
  lead.last_status_ = gtop_set_problem(lead.ctx_, (int)robots.size(), m, T.data(), m, Df.data());
  return lead.last_status_ == GTOP_OK;
}

void GradTrajOptimizer::ownProblem() {
  const int rc = gtop_set_problem(ctx_, 1, m_, segment_time_.data(), m_, df_.data());
  if (last_status_ == GTOP_OK) last_status_ = rc;
}

bool GradTrajOptimizer::swarmGradient(const std::vector<GradTrajOptimizer *> &robots, const SwarmOptions &options,
                                      std::vector<double> *S, std::vector<std::vector<double>> *grad,
                                      std::vector<double> *active) {
  gtop_swarm_opts opt;
  std::vector<double> x;
  if (!swarmProblem(robots, options, &opt, &x)) return false;
  GradTrajOptimizer &lead = *robots[0];
  const size_t B = robots.size(), n = lead.dp_.size();
  std::vector<double> s(B), g(B * n), a(B);
  lead.last_status_ = gtop_swarm_gradient_batch(lead.ctx_, &opt, (int)B, x.data(), nullptr, s.data(), g.data(), a.data());
  lead.ownProblem();
  if (lead.last_status_ != GTOP_OK) return false;
  if (S) *S = s;
  if (active) *active = a;
  if (grad) {
    grad->resize(B);
    for (size_t b = 0; b < B; ++b) (*grad)[b].assign(g.begin() + b * n, g.begin() + (b + 1) * n);
  }
  return true;
}

bool GradTrajOptimizer::optimizeSwarm(const std::vector<GradTrajOptimizer *> &robots, const SwarmOptions &options,
                                      std::vector<double> *min_cost, std::vector<std::array<double, 2>> *joint) {
  gtop_swarm_opts opt;
  std::vector<double> x;
  if (!swarmProblem(robots, options, &opt, &x)) return false;
  GradTrajOptimizer &lead = *robots[0];
  const size_t B = robots.size(), n = lead.dp_.size();
  gtop_swarm_stop stop{};
  stop.sweeps = options.sweeps;
  stop.evals_per_sweep = options.evals_per_sweep;
  std::vector<double> lb(B * n), ub(B * n), mc(B), jt(2 * B);   // the bounds of optimizeTrajectory, :151-179
  for (size_t b = 0; b < B; ++b) {
    const GradTrajOptimizer &r = *robots[b];
    for (int i = 0; i < r.num_dp_; ++i)
      for (int a = 0; a < 3; ++a) {
        const size_t j = b * n + (size_t)i + (size_t)a * r.num_dp_;
        const double centre = i % 3 == 0 ? r.path_[(i / 3 + 1) * 3 + a] : 0.0;
        const double half = i % 3 == 0 ? r.cfg_.bos : (i % 3 == 1 ? r.cfg_.vos : r.cfg_.aos);
        lb[j] = centre - half;
        ub[j] = centre + half;
      }
  }
  gtop_set_optimizer_precision(lead.ctx_, GTOP_F64);
  lead.last_status_ = gtop_optimize_swarm(lead.ctx_, &opt, &stop, (int)B, x.data(), lb.data(), ub.data(), mc.data(), jt.data());
  lead.ownProblem();
  if (lead.last_status_ != GTOP_OK) return false;
  for (size_t b = 0; b < B; ++b) {
    GradTrajOptimizer &r = *robots[b];
    r.dp_.assign(x.begin() + b * n, x.begin() + (b + 1) * n);
    r.coefficientsFromDerivatives(r.dp_);
  }
  if (min_cost) *min_cost = mc;
  if (joint) {
    joint->resize(B);
    for (size_t b = 0; b < B; ++b) (*joint)[b] = {jt[2 * b], jt[2 * b + 1]};
  }
  return true;
}

bool GradTrajOptimizer::insertWaypoint(const InsertOptions &options, InsertInfo *info) {
  if (!ctx_ || m_ < 2 || dp_.empty()) {
    last_status_ = GTOP_ERR_STATE;
    return false;
  }
  gtop_insert opt{};
  opt.mode = options.mode;
  opt.min_fraction = options.min_fraction;
  opt.push = options.push;
  opt.push_below = options.push_below;
  const int m = m_ + 1, num_dp = 3 * m - 3;
  std::vector<double> x((size_t)3 * num_dp), T(m);
  double row[GTOP_INSERT_INFO];
  last_status_ = gtop_insert_waypoints(ctx_, &opt, 1, dp_.data(), &options.when, nullptr, nullptr, x.data(), T.data(),
                                       nullptr, nullptr, row);
  if (last_status_ != GTOP_OK) return false;
  last_status_ = gtop_set_problem(ctx_, 1, m, T.data(), m, df_.data());   // (refuses a time that is not > 0)
  if (last_status_ != GTOP_OK) return false;
  const int s = (int)row[0];
  double p[3];
  for (int a = 0; a < 3; ++a) p[a] = x[(size_t)a * num_dp + 3 * s];   // junction s + 1 of the new row
  path_.insert(path_.begin() + 3 * (s + 1), p, p + 3);
  m_ = m;
  num_dp_ = num_dp;
  segment_time_ = T;
  dp_ = x;
  coefficientsFromDerivatives(dp_);
  if (info) {
    info->segment = s;
    info->local_time = row[1];
    info->fell_back = row[2] != 0.0;
    info->clamped = row[3] != 0.0;
    info->distance = row[4];
    info->pushed = row[5] != 0.0;
  }
  return true;
}

// Common tail of setPath / setKinoPath: Df, Dp (getInitialD,
// src/qp_generator.cpp:407-451), initial coefficients (Px = A^-1 Dx,
// :334-336 / :134-136), then the problem goes to the device.
void GradTrajOptimizer::setupProblem(const std::vector<double> &path_flat, int npts,
                                     const std::vector<double> &seg_time, const std::vector<double> &Dx,
                                     const std::vector<double> &Dy, const std::vector<double> &Dz) {
  path_ = path_flat;
  segment_time_ = seg_time;
  m_ = npts - 1;
  num_dp_ = 3 * m_ - 3;
  const std::vector<double> *D[3] = {&Dx, &Dy, &Dz};
  df_.assign(18, 0.0);
  dp_.assign((size_t)3 * num_dp_, 0.0);
  coeff_.resize(m_, 18);
  for (int a = 0; a < 3; ++a) {
    const std::vector<double> &d = *D[a];
    df_[a * 6 + 0] = d[0];                  // :418-423
    df_[a * 6 + 3] = d[d.size() - 5];
    df_[a * 6 + 1] = 0.0;                   // startVel / startAcc (:425-431): file-scope globals that
    df_[a * 6 + 2] = 0.0;                   // every caller leaves at zero (setPath passes 0, :83-85)
    for (int k = 1; k < m_; k++)            // :433-439
      for (int i = 0; i < 3; i++) dp_[(size_t)a * num_dp_ + (k - 1) * 3 + i] = d[(k - 1) * 6 + 2 * i + 1];
    for (int s = 0; s < m_; ++s) {
      double c[6];
      quintic_from_boundary(&d[s * 6], segment_time_[s], c);
      for (int j = 0; j < 6; ++j) coeff_(s, 6 * a + j) = c[j];
    }
  }
  if (!ctx_) return;
  last_status_ = gtop_set_problem(ctx_, 1, m_, segment_time_.data(), m_, df_.data());
  if (cfg_.initial_guess == 1 && last_status_ == GTOP_OK) {
    last_status_ = gtop_min_jerk_start(ctx_, 1, dp_.data());
    if (last_status_ == GTOP_OK) coefficientsFromDerivatives(dp_);
  }
}

void GradTrajOptimizer::setPath(const std::vector<Vec3> &way_points) {
  const int npts = (int)way_points.size();
  if (npts < 3) {   // m >= 2: StackOptiDep indexes out of bounds otherwise (src/qp_generator.cpp:365-378)
    last_status_ = GTOP_ERR_INVALID;
    return;
  }
  const int m = npts - 1;
  std::vector<double> path((size_t)npts * 3);
  for (int i = 0; i < npts; ++i)
    for (int a = 0; a < 3; ++a) path[i * 3 + a] = way_points[i][a];
  // :73-81 — `i == segment_time.size()` never holds, so only segment 0 gets init_time
  std::vector<double> T(m);
  for (int i = 0; i < m; ++i) {
    const double dx = path[i * 3] - path[(i + 1) * 3], dy = path[i * 3 + 1] - path[(i + 1) * 3 + 1],
                 dz = path[i * 3 + 2] - path[(i + 1) * 3 + 2];
    const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
    if (i == 0 || i == m) T[i] = len / cfg_.mean_v + cfg_.init_time;
    else T[i] = len / cfg_.mean_v;
  }
  // PolyQPGeneration(type = 2), src/qp_generator.cpp:199-221: positions at both
  // ends of each segment, start vel = acc = 0 (:83-85), everything else 0.
  std::vector<double> D[3];
  for (int a = 0; a < 3; ++a) {
    D[a].assign((size_t)6 * m, 0.0);
    for (int k = 1; k < m + 1; k++) {
      D[a][(k - 1) * 6] = path[(k - 1) * 3 + a];
      D[a][(k - 1) * 6 + 1] = path[k * 3 + a];
    }
  }
  setupProblem(path, npts, T, D[0], D[1], D[2]);
}

void GradTrajOptimizer::setKinoPath(const Matrix &Pos, const Matrix &Vel, const Matrix &Acc,
                                    const std::vector<double> &Time) {
  const int m = (int)Time.size();
  if (m < 2 || Pos.rows != m + 1 || Vel.rows != m + 1 || Acc.rows != m + 1 || Pos.cols != 3 ||
      Vel.cols != 3 || Acc.cols != 3) {
    last_status_ = GTOP_ERR_INVALID;
    return;
  }
  std::vector<double> path((size_t)(m + 1) * 3);
  for (int i = 0; i < m + 1; ++i)
    for (int a = 0; a < 3; ++a) path[i * 3 + a] = Pos(i, a);
  // PolyKinoGeneration, src/qp_generator.cpp:63-86
  std::vector<double> D[3];
  for (int a = 0; a < 3; ++a) {
    D[a].assign((size_t)6 * m, 0.0);
    for (int k = 0; k < m; k++) {
      D[a][k * 6] = Pos(k, a);
      D[a][k * 6 + 1] = Pos(k + 1, a);
      D[a][k * 6 + 2] = Vel(k, a);
      D[a][k * 6 + 3] = Vel(k + 1, a);
      D[a][k * 6 + 4] = Acc(k, a);
      D[a][k * 6 + 5] = Acc(k + 1, a);
    }
  }
  setupProblem(path, m + 1, Time, D[0], D[1], D[2]);
}

// getCoefficientFromDerivative, :253-279: coe = L d, which per segment is
// A_s^-1 applied to the derivatives of its two waypoints.
void GradTrajOptimizer::coefficientsFromDerivatives(const std::vector<double> &dp) {
  coeff_.resize(m_, 18);
  for (int a = 0; a < 3; ++a) {
    auto wp = [&](int j, int der) -> double {   // derivative `der` of waypoint j on axis a
      if (j == 0) return df_[a * 6 + der];
      if (j == m_) return df_[a * 6 + 3 + der];
      return dp[(size_t)a * num_dp_ + 3 * (j - 1) + der];
    };
    for (int s = 0; s < m_; ++s) {
      const double d[6] = {wp(s, 0), wp(s + 1, 0), wp(s, 1), wp(s + 1, 1), wp(s, 2), wp(s + 1, 2)};
      double c[6];
      quintic_from_boundary(d, segment_time_[s], c);
      for (int j = 0; j < 6; ++j) coeff_(s, 6 * a + j) = c[j];
    }
  }
}

bool GradTrajOptimizer::optimizeTrajectory(int step) {
  if (step != 0 && step != 1 && step != 2) {   // :129-131 (the reference prints and carries on)
    std::printf("step number error, step should be 0, 1 or 2\n");
  }
  if (!ctx_ || m_ < 2) return true;   // :242 — always true
  step_ = step;
  if (step == 0 || step == 1 || step == 2) pushParams();

  const unsigned n = 3u * (unsigned)num_dp_;
  MmaOptions opt;
  if (step == OPT_FIRST_STEP) opt.maxtime = cfg_.time_limit_1;        // :144-148
  else if (step == OPT_SECOND_STEP) opt.maxtime = cfg_.time_limit_2;
  opt.maxeval = cfg_.max_evals;

  // bounds, :151-179
  std::vector<double> lb(n), ub(n);
  for (int i = 0; i < num_dp_; ++i) {
    for (int a = 0; a < 3; ++a) {
      const size_t j = (size_t)i + (size_t)a * num_dp_;
      if (i % 3 == 0) {
        lb[j] = path_[(i / 3 + 1) * 3 + a] - cfg_.bos;
        ub[j] = path_[(i / 3 + 1) * 3 + a] + cfg_.bos;
      } else if (i % 3 == 1) {
        lb[j] = -cfg_.vos;
        ub[j] = cfg_.vos;
      } else {
        lb[j] = -cfg_.aos;
        ub[j] = cfg_.aos;
      }
    }
  }
  std::vector<double> x = dp_;   // :182-187
  gtop_clear_cost_curve(ctx_);   // :192-194
  if (cfg_.optimize_on_device) {
    // (maxtime alone bounds the reference's run: an evaluation cap far past what it can reach stands in for "none")
    const gtop_stop stop = {opt.maxeval > 0 ? opt.maxeval : (1 << 24), 0.0, 0.0, opt.maxtime};
    double minf = 0.0;
    int32_t nev = 0, code = 0;
    gtop_set_optimizer_precision(ctx_, cfg_.optimizer_fp32 ? GTOP_F32 : GTOP_F64);
    last_status_ = gtop_optimize_batch_ex(ctx_, 1, x.data(), lb.data(), ub.data(), &stop, &minf, &nev, &code);
    last_evals_ = nev;
  } else {
    MmaResult r = mma_minimize(n, nlopt_trampoline, ctx_, lb.data(), ub.data(), x.data(), opt);
    last_evals_ = r.nevals;
  }
  dp_ = x;                        // :202-207
  if (cfg_.reallocate_time == 1) {   // :209-227, the block the reference carries commented out
    RetimeOptions length;
    length.mode = GTOP_RETIME_LENGTH;
    if (!reallocateSegmentTime(length)) return true;   // (:242 — always true; ok() tells)
  }
  coefficientsFromDerivatives(x);  // :230 — with the new times where they were reallocated
  if (step == 1 || step == 2) {   // :233-240
    int64_t it = 0;
    double tt = 0;
    gtop_get_stats(ctx_, &it, &tt);
    std::printf("total time:%g\niterative num:%lld\n", tt, (long long)it);
    if (step == 2) gtop_reset_stats(ctx_);
  }
  return true;
}

void GradTrajOptimizer::getCoefficient(Matrix &coeff) { coeff = coeff_; }

void GradTrajOptimizer::getSegmentTime(std::vector<double> &seg_time) { seg_time = segment_time_; }

void GradTrajOptimizer::getCostCurve(std::vector<double> &cost, std::vector<double> &time) {
  cost.clear();
  time.clear();
  if (!ctx_) return;
  int count = 0;
  gtop_get_cost_curve(ctx_, nullptr, nullptr, 0, &count);
  cost.resize(count);
  time.resize(count);
  if (count) gtop_get_cost_curve(ctx_, cost.data(), time.data(), count, &count);
}

// :554-562
double GradTrajOptimizer::costFunc(const std::vector<double> &x, std::vector<double> &grad, void *func_data) {
  GradTrajOptimizer *gtop = reinterpret_cast<GradTrajOptimizer *>(func_data);
  grad.resize(x.size());   // the reference resizes grad itself (:426)
  return gtop_cost_nlopt((unsigned)x.size(), x.data(), grad.data(), gtop->ctx_);
}

// ---- GradTrajBatch ----------------------------------------------------------------------------------------------

GradTrajBatch::GradTrajBatch(const std::vector<int> &devices, const GradTrajOptimizer::Config &cfg) : cfg_(cfg) {
  last_status_ = gtop_group_create(&grp_, devices.data(), (int)devices.size());
  if (last_status_ != GTOP_OK) grp_ = nullptr;
}

GradTrajBatch::~GradTrajBatch() {
  if (grp_) gtop_group_destroy(grp_);
}

int GradTrajBatch::devices() const { return grp_ ? gtop_group_size(grp_) : 0; }
const char *GradTrajBatch::gatherBackend() const { return grp_ ? gtop_group_gather_backend(grp_) : ""; }
const char *GradTrajBatch::lastError() const { return grp_ ? gtop_group_last_error(grp_) : "gtop_group_create failed"; }

void GradTrajBatch::initSDFMap(Vec3 map_size_3d, Vec3 origin, double resolution) {
  if (grp_) last_status_ = gtop_group_init_sdf_map(grp_, map_size_3d.data(), origin.data(), resolution);
}

void GradTrajBatch::updateSDFMap(const std::vector<Vec3> &obs) {
  if (grp_) last_status_ = gtop_group_update_sdf_map(grp_, obs.empty() ? nullptr : obs[0].data(), (int)obs.size());
}

void GradTrajBatch::setPaths(const std::vector<std::vector<Vec3>> &way_points) {
  const int B = (int)way_points.size();
  bool valid = B > 0;
  for (const auto &w : way_points) valid = valid && w.size() >= 3;
  if (!grp_ || !valid) {
    last_status_ = GTOP_ERR_INVALID;
    return;
  }
  B_ = B;
  m_of_.assign(B, 0);
  path_at_.assign(B, 0);
  T_at_.assign(B, 0);
  x_at_.assign(B, 0);
  size_t np = 0, nt = 0, nx = 0;
  for (int b = 0; b < B; ++b) {
    const int m = (int)way_points[b].size() - 1;
    m_of_[b] = m;
    path_at_[b] = np; T_at_[b] = nt; x_at_[b] = nx;
    np += (size_t)(m + 1) * 3; nt += (size_t)m; nx += 9 * (size_t)(m - 1);
  }
  path_.assign(np, 0.0);
  T_.assign(nt, 0.0);
  Df_.assign((size_t)B * 18, 0.0);
  x_.assign(nx, 0.0);
  for (int b = 0; b < B; ++b) {
    const int m = m_of_[b], num_dp = 3 * m - 3;
    double *p = &path_[path_at_[b]], *T = &T_[T_at_[b]], *x = &x_[x_at_[b]];
    for (int i = 0; i <= m; ++i)
      for (int a = 0; a < 3; ++a) p[i * 3 + a] = way_points[b][i][a];
    for (int i = 0; i < m; ++i) {   // :73-81 (only segment 0 gets init_time: the `i == size()` clause never holds)
      const double dx = p[i * 3] - p[(i + 1) * 3], dy = p[i * 3 + 1] - p[(i + 1) * 3 + 1], dz = p[i * 3 + 2] - p[(i + 1) * 3 + 2];
      T[i] = std::sqrt(dx * dx + dy * dy + dz * dz) / cfg_.mean_v + (i == 0 ? cfg_.init_time : 0.0);
    }
    for (int a = 0; a < 3; ++a) {   // getInitialD (src/qp_generator.cpp:407-451): positions only, zero velocity / acceleration
      Df_[(size_t)b * 18 + a * 6 + 0] = p[a];
      Df_[(size_t)b * 18 + a * 6 + 3] = p[m * 3 + a];
      for (int k = 1; k < m; ++k) x[(size_t)a * num_dp + (k - 1) * 3] = p[k * 3 + a];
    }
  }
  min_cost_.assign(B, 0.0);
  nevals_.assign(B, 0);
  last_status_ = GTOP_OK;
  if (cfg_.initial_guess != 1) return;
  // the minimum-jerk start: one call per distinct segment count on the first member's context (its problem is set anew
  // by every optimizeTrajectories)
  gtop_ctx *ctx = gtop_group_context(grp_, 0);
  std::vector<int> order(B);
  for (int b = 0; b < B; ++b) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return m_of_[a] < m_of_[b]; });
  std::vector<double> T, Df, x;
  for (int lo = 0; lo < B;) {
    const int m = m_of_[order[lo]];
    int hi = lo;
    while (hi < B && m_of_[order[hi]] == m) ++hi;
    const int nb = hi - lo;
    const size_t n = 9 * (size_t)(m - 1);
    T.resize((size_t)nb * m); Df.resize((size_t)nb * 18); x.resize(nb * n);
    for (int k = 0; k < nb; ++k) {
      const int b = order[lo + k];
      std::copy_n(&T_[T_at_[b]], m, &T[(size_t)k * m]);
      std::copy_n(&Df_[(size_t)b * 18], 18, &Df[(size_t)k * 18]);
      std::copy_n(&x_[x_at_[b]], n, &x[k * n]);
    }
    if ((last_status_ = gtop_set_problem(ctx, nb, m, T.data(), m, Df.data())) != GTOP_OK) return;
    if ((last_status_ = gtop_min_jerk_start(ctx, nb, x.data())) != GTOP_OK) return;
    for (int k = 0; k < nb; ++k) std::copy_n(&x[k * n], n, &x_[x_at_[order[lo + k]]]);
    lo = hi;
  }
}

bool GradTrajBatch::optimizeTrajectories(int step) {
  if (!grp_ || B_ == 0) return true;   // (:242 — always true)
  gtop_params p;
  p.ws = cfg_.ws; p.wc = cfg_.wc;
  p.alpha = cfg_.alpha; p.r = cfg_.r; p.d0 = cfg_.d0;
  p.alpha_v = cfg_.alpha_v; p.r_v = cfg_.r_v; p.v0 = cfg_.v0;
  p.alpha_a = cfg_.alpha_a; p.r_a = cfg_.r_a; p.a0 = cfg_.a0;
  p.step = step;
  p.enable_dyn = cfg_.enable_dyn;
  if ((last_status_ = gtop_group_set_params(grp_, &p)) != GTOP_OK) return true;
  if ((last_status_ = gtop_group_set_gradient_mode(grp_, cfg_.gradient_mode)) != GTOP_OK) return true;
  for (int i = 0; i < gtop_group_size(grp_); ++i)
    gtop_set_optimizer_precision(gtop_group_context(grp_, i), cfg_.optimizer_fp32 ? GTOP_F32 : GTOP_F64);
  const double maxtime = step == OPT_FIRST_STEP ? cfg_.time_limit_1 : (step == OPT_SECOND_STEP ? cfg_.time_limit_2 : 0.0);
  const gtop_stop stop = {cfg_.max_evals > 0 ? cfg_.max_evals : (1 << 24), 0.0, 0.0, maxtime};   // :144-148
  // one device problem per distinct segment count, in rising order; each is the whole optimisation of its
  // trajectories in one launch per device (the wall-clock limit is each problem's own, as it is each object's in the
  // reference)
  std::vector<int> order(B_);
  for (int b = 0; b < B_; ++b) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return m_of_[a] < m_of_[b]; });
  std::vector<double> T, Df, x, path, lb, ub, cost;
  std::vector<int32_t> nev, code;
  for (int lo = 0; lo < B_;) {
    const int m = m_of_[order[lo]];
    int hi = lo;
    while (hi < B_ && m_of_[order[hi]] == m) ++hi;
    const int nb = hi - lo;
    const size_t n = 9 * (size_t)(m - 1), np = (size_t)(m + 1) * 3;
    T.resize((size_t)nb * m); Df.resize((size_t)nb * 18); x.resize(nb * n); path.resize(nb * np);
    lb.resize(nb * n); ub.resize(nb * n); cost.resize(nb); nev.resize(nb); code.resize(nb);
    for (int k = 0; k < nb; ++k) {
      const int b = order[lo + k];
      std::copy_n(&T_[T_at_[b]], m, &T[(size_t)k * m]);
      std::copy_n(&Df_[(size_t)b * 18], 18, &Df[(size_t)k * 18]);
      std::copy_n(&x_[x_at_[b]], n, &x[k * n]);
      std::copy_n(&path_[path_at_[b]], np, &path[k * np]);
    }
    gtop_default_bounds(nb, m, path.data(), cfg_.bos, cfg_.vos, cfg_.aos, lb.data(), ub.data());   // :151-179
    if ((last_status_ = gtop_group_set_problem(grp_, nb, m, T.data(), m, Df.data())) != GTOP_OK) return true;
    last_status_ = gtop_group_optimize_batch_ex(grp_, nb, x.data(), lb.data(), ub.data(), &stop, cost.data(), nev.data(),
                                                code.data());
    if (last_status_ != GTOP_OK) return true;
    for (int k = 0; k < nb; ++k) {
      const int b = order[lo + k];
      std::copy_n(&x[k * n], n, &x_[x_at_[b]]);
      min_cost_[b] = cost[k];
      nevals_[b] = nev[k];
    }
    lo = hi;
  }
  return true;
}

void GradTrajBatch::getCoefficient(int b, Matrix &coeff) const {
  if (b < 0 || b >= B_) {
    coeff.resize(0, 18);
    return;
  }
  const int m = m_of_[b], num_dp = 3 * m - 3;
  coeff.resize(m, 18);
  const double *df = &Df_[(size_t)b * 18], *x = &x_[x_at_[b]], *T = &T_[T_at_[b]];
  for (int a = 0; a < 3; ++a) {
    auto wp = [&](int j, int der) -> double {
      if (j == 0) return df[a * 6 + der];
      if (j == m) return df[a * 6 + 3 + der];
      return x[(size_t)a * num_dp + 3 * (j - 1) + der];
    };
    for (int s = 0; s < m; ++s) {
      const double d[6] = {wp(s, 0), wp(s + 1, 0), wp(s, 1), wp(s + 1, 1), wp(s, 2), wp(s + 1, 2)};
      double c[6];
      quintic_from_boundary(d, T[s], c);
      for (int j = 0; j < 6; ++j) coeff(s, 6 * a + j) = c[j];
    }
  }
}

}  // namespace gtop_amd
