// retime_shim.cpp — GradTrajOptimizer::Config::reallocate_time, segmentReport and reallocateSegmentTime
// (csrc/grad_traj_optimizer.hpp) on a scene file written by tests/scenes.py.  The scene is optimised twice on the
// device, with reallocate_time 0 and 1; each run prints the free derivatives, the segment times and the coefficients
// it ends with and the per-segment report there; the first run then stretches its times by limits
// (reallocateSegmentTime, GTOP_RETIME_LIMITS at max_vel = 0.8 of its largest segment figure, scale_x) and prints
// that state too — one JSON object that tests/test_gpu_retime_shim.py checks against the Python binding.
//
//   gtop_retime_shim <scene.txt> [max_evals = 20]
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

// x, segment times, coefficients and the segment report of the object's current state
bool put_state(const char *name, GradTrajOptimizer &opt, const GradTrajOptimizer::Limits &lim, const char *tail) {
  std::vector<double> T;
  opt.getSegmentTime(T);
  Matrix coeff;
  opt.getCoefficient(coeff);
  std::vector<GradTrajOptimizer::SegmentReport> rows;
  const bool ok = opt.segmentReport(lim, &rows);
  std::vector<double> flat;
  for (const auto &r : rows)
    for (double v : {(double)r.n_samples, (double)r.first_sample, r.clearance, r.clearance_time, (double)r.n_below_margin,
                     (double)r.n_out_of_map, r.max_vel_norm, r.max_acc_norm, r.max_vel_axis, r.max_acc_axis})
      flat.push_back(v);
  json += std::string("\"") + name + "\": {\"ok\": " + (ok && opt.ok() ? "1" : "0") + ", ";
  put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ", ");
  put_list(json, "segment_time", T.data(), T.size(), ", ");
  put_list(json, "coeff", coeff.a.data(), coeff.a.size(), ", ");
  put_list(json, "segments", flat.data(), flat.size(), "");
  json += std::string("}") + tail;
  return ok && opt.ok();
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
  bool all_ok = true;
  json += "{\n";
  for (int reallocate = 0; reallocate < 2; ++reallocate) {
    GradTrajOptimizer::Config cfg;
    cfg.max_evals = argc > 2 ? std::atoi(argv[2]) : 20;
    cfg.time_limit_2 = 5.0;            // evaluation-capped so the run is reproducible
    cfg.optimize_on_device = 1;
    cfg.reallocate_time = reallocate;
    GradTrajOptimizer opt(cfg);
    if (!opt.ok()) {
      std::fprintf(stderr, "%s\n", opt.lastError());
      return 2;
    }
    opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
    opt.updateSDFMap(sc.obstacles);
    opt.setPath(sc.waypoints);
    opt.optimizeTrajectory(OPT_SECOND_STEP);
    all_ok = all_ok && opt.ok();
    all_ok = put_state(reallocate ? "reallocate1" : "reallocate0", opt, lim, ",\n") && all_ok;
    if (reallocate == 0) {
      std::vector<GradTrajOptimizer::SegmentReport> rows;
      opt.segmentReport(lim, &rows);
      double vmax = 0.0;
      for (const auto &r : rows) vmax = std::fmax(vmax, r.max_vel_norm);
      GradTrajOptimizer::RetimeOptions o;
      o.max_vel = 0.8 * vmax;
      o.scale_x = true;
      o.report = lim;
      const bool done = opt.reallocateSegmentTime(o);
      char buf[64];
      std::snprintf(buf, sizeof buf, "\"max_vel\": %.17g,\n", o.max_vel);
      json += buf;
      all_ok = put_state("limits", opt, lim, ",\n") && done && all_ok;
    }
  }
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return all_ok ? 0 : 2;
}
