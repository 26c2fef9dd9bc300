// validate_shim.cpp — GradTrajOptimizer::validateTrajectory (csrc/grad_traj_optimizer.hpp) on a scene file written by
// tests/scenes.py: the report of the straight-line start and of the optimised trajectory, with the free derivatives
// each was taken at, as one JSON object that tests/test_gpu_validate_shim.py checks against the Python binding's
// gtop_validate_batch on the same inputs.
//
//   gtop_validate_shim <scene.txt> [max_evals = 40] [optimize_on_device = 0]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"
#include "scene_file.h"

using namespace gtop_amd;

namespace {

// one state's JSON entry, as text (printed at the end: the optimizer reports on stdout while it runs)
std::string state_json(const char *name, GradTrajOptimizer &opt, const GradTrajOptimizer::Limits &lim, bool comma) {
  GradTrajOptimizer::Report r;
  const bool pass = opt.validateTrajectory(lim, &r);
  char buf[1024];
  std::snprintf(buf, sizeof buf, "\"%s\": {\"ok\": %d, \"pass\": %d, \"report\": [%d, %.17g, %.17g, %d, %d, %.17g, %d, %.17g, %.17g, %.17g, %.17g, %.17g],\n",
              name, opt.ok() ? 1 : 0, pass ? 1 : 0, r.n_samples, r.clearance, r.clearance_time, r.clearance_index,
              r.n_below_margin, r.first_below_time, r.n_out_of_map, r.max_vel_norm, r.max_acc_norm, r.max_vel_axis,
              r.max_acc_axis, r.time_sum);
  std::string out = buf;
  out += "\"x\": [";
  const std::vector<double> &x = opt.freeDerivatives();
  for (size_t i = 0; i < x.size(); ++i) {
    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", x[i]);
    out += buf;
  }
  out += comma ? "]},\n" : "]}\n";
  return out;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <scene.txt> [max_evals] [optimize_on_device]\n", argv[0]);
    return 1;
  }
  scene_file::Scene sc;
  if (!scene_file::read_scene(argv[1], sc)) return 1;
  GradTrajOptimizer::Config cfg;
  cfg.max_evals = argc > 2 ? std::atoi(argv[2]) : 40;
  cfg.time_limit_2 = 5.0;          // evaluation-capped so the run is reproducible
  cfg.optimize_on_device = argc > 3 ? std::atoi(argv[3]) : 0;
  GradTrajOptimizer opt(cfg);
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  GradTrajOptimizer::Limits lim;
  lim.margin = 0.3;
  lim.max_vel = 4.0;
  // before a path is set there is nothing to validate: refused, not a crash
  const bool early = opt.validateTrajectory(lim);
  const bool early_ok = opt.ok();
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  const std::string start = state_json("start", opt, lim, true);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  const std::string optimised = state_json("optimised", opt, lim, false);
  std::printf("{\"early_pass\": %d, \"early_ok\": %d,\n", early ? 1 : 0, early_ok ? 1 : 0);
  std::vector<double> seg_time;
  opt.getSegmentTime(seg_time);
  std::printf("\"segment_times\": [");
  for (size_t i = 0; i < seg_time.size(); ++i) std::printf("%s%.17g", i ? ", " : "", seg_time[i]);
  std::printf("],\n");
  std::printf("%s%s}\n", start.c_str(), optimised.c_str());
  return opt.ok() ? 0 : 2;
}
