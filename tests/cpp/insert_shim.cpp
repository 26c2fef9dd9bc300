// insert_shim.cpp — GradTrajOptimizer::insertWaypoint (csrc/grad_traj_optimizer.hpp) on a scene file written by
// tests/scenes.py.  The scene is optimised on the device; the object then takes a waypoint at the time of its least
// clearance (GTOP_INSERT_AT_TIME at validateTrajectory's clearance_time), a second one in its longest segment with a
// push, is optimised again on the problem of two segments more, and a call with a bad option is shown to change
// nothing.  Each state is printed — the free derivatives, the segment times, the coefficients, the report — as one JSON
// object that tests/test_gpu_insert_shim.py checks against the Python binding.
//
//   gtop_insert_shim <scene.txt> [max_evals = 20]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"
#include "scene_file.h"

using namespace gtop_amd;
using scene_file::put_list;

namespace {

// the JSON is collected and printed at the end: the optimizer reports on stdout while it runs
std::string json;

// x, segment times, coefficients and the whole-trajectory report of the object's current state
bool put_state(const char *name, GradTrajOptimizer &opt, const GradTrajOptimizer::Limits &lim,
               const GradTrajOptimizer::InsertInfo *info, const char *tail) {
  std::vector<double> T;
  opt.getSegmentTime(T);
  Matrix coeff;
  opt.getCoefficient(coeff);
  GradTrajOptimizer::Report r;
  opt.validateTrajectory(lim, &r);
  const bool ok = opt.ok();
  const double rep[4] = {(double)r.n_samples, r.clearance, r.clearance_time, r.time_sum};
  json += std::string("\"") + name + "\": {\"ok\": " + (ok ? "1" : "0") + ", ";
  put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ", ");
  put_list(json, "segment_time", T.data(), T.size(), ", ");
  put_list(json, "coeff", coeff.a.data(), coeff.a.size(), ", ");
  if (info) {
    const double row[6] = {(double)info->segment, info->local_time, (double)info->fell_back, (double)info->clamped,
                           info->distance, (double)info->pushed};
    put_list(json, "info", row, 6, ", ");
  }
  put_list(json, "report", rep, 4, "");
  json += std::string("}") + tail;
  return ok;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <scene.txt> [max_evals]\n", argv[0]);
    return 1;
  }
  scene_file::Scene sc;
  if (!scene_file::read_scene(argv[1], sc)) return 1;
  GradTrajOptimizer::Limits lim;
  lim.margin = 0.3;
  GradTrajOptimizer::Config cfg;
  cfg.max_evals = argc > 2 ? std::atoi(argv[2]) : 20;
  cfg.time_limit_2 = 5.0;            // evaluation-capped so the run is reproducible
  cfg.optimize_on_device = 1;
  GradTrajOptimizer opt(cfg);
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  bool all_ok = opt.ok();
  json += "{\n";
  all_ok = put_state("solved", opt, lim, nullptr, ",\n") && all_ok;

  // a waypoint where the clearance is least
  GradTrajOptimizer::Report r;
  opt.validateTrajectory(lim, &r);
  GradTrajOptimizer::InsertOptions at;
  at.mode = GTOP_INSERT_AT_TIME;
  at.when = r.clearance_time;
  GradTrajOptimizer::InsertInfo info;
  bool done = opt.insertWaypoint(at, &info);
  all_ok = put_state("at_time", opt, lim, &info, ",\n") && done && all_ok;

  // a bad option: false, and nothing changed
  GradTrajOptimizer::InsertOptions bad;
  bad.min_fraction = 0.75;
  const bool refused = !opt.insertWaypoint(bad) && !opt.ok();
  json += std::string("\"refused\": ") + (refused ? "1" : "0") + ",\n";
  put_state("after_refusal", opt, lim, nullptr, ",\n");

  // a second one in the longest segment, pushed up the gradient where the field is closer than 1 m
  GradTrajOptimizer::InsertOptions longest;
  longest.push = 0.25;
  longest.push_below = 1.0;
  done = opt.insertWaypoint(longest, &info);
  all_ok = put_state("longest", opt, lim, &info, ",\n") && done && all_ok;

  // the optimizer on the problem of two segments more
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  all_ok = opt.ok() && all_ok;
  all_ok = put_state("resolved", opt, lim, nullptr, ",\n") && all_ok;
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return all_ok && refused ? 0 : 2;
}
