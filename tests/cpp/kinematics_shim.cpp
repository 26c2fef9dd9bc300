// kinematics_shim.cpp — GradTrajOptimizer::certifyKinematics (csrc/grad_traj_optimizer.hpp) on a scene file written by
// tests/scenes.py.  The scene is optimised on the device; the kinematic certificate of the optimised trajectory is then
// taken with the limits off, at limits no flight of this path keeps (0.01 m/s), at generous ones (100 m/s, 1000 m/s^2,
// per axis), at level 0 alone and with bad options, and printed with the free derivatives as one JSON object that
// tests/test_gpu_kinematics_shim.py checks against the Python binding.
//
//   gtop_kinematics_shim <scene.txt> [max_evals = 20]
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

void put_certificate(const char *name, GradTrajOptimizer &opt, double max_vel, double max_acc, bool per_axis,
                     int max_depth, int max_refine) {
  GradTrajOptimizer::KinematicOptions o;
  o.max_vel = max_vel;
  o.max_acc = max_acc;
  o.per_axis = per_axis;
  o.max_depth = max_depth;
  o.max_refine = max_refine;
  GradTrajOptimizer::KinematicReport r;
  const bool within = opt.certifyKinematics(o, r);
  const double row[11] = {(double)r.verdict, r.ub_vel, r.lo_vel, r.lo_vel_time, r.ub_acc, r.lo_acc, r.lo_acc_time,
                          r.first_violation_time, (double)r.n_undecided, (double)r.n_refinements, r.time_sum};
  json += std::string("\"") + name + "\": {\"within\": " + (within ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") + ", ";
  put_list(json, "kin", row, 11, "},\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <scene.txt> [max_evals]\n", argv[0]);
    return 1;
  }
  scene_file::Scene sc;
  if (!scene_file::read_scene(argv[1], sc)) return 1;
  GradTrajOptimizer::Config cfg;
  cfg.max_evals = argc > 2 ? std::atoi(argv[2]) : 20;
  cfg.time_limit_2 = 5.0;            // evaluation-capped so the run is reproducible
  cfg.optimize_on_device = 1;
  GradTrajOptimizer opt(cfg);
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  json += "{\n";
  {   // before a path is set there is nothing to certify
    GradTrajOptimizer::KinematicReport r;
    const bool within = opt.certifyKinematics(GradTrajOptimizer::KinematicOptions(), r);
    json += std::string("\"no_path\": {\"within\": ") + (within ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") + "},\n";
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  const bool solved = opt.ok();
  put_certificate("off", opt, 0.0, 0.0, false, 2, 256);
  put_certificate("tight", opt, 0.01, 0.01, false, 2, 256);
  put_certificate("generous", opt, 100.0, 1000.0, true, 2, 256);
  put_certificate("level0", opt, 100.0, 0.0, false, 0, 0);
  put_certificate("bad_depth", opt, 1.0, 1.0, false, 4, 256);
  put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ",\n");
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return solved ? 0 : 2;
}
