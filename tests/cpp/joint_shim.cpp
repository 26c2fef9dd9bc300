// joint_shim.cpp — GradTrajOptimizer::jointGradient and optimizeJoint (csrc/grad_traj_optimizer.hpp) on a scene file
// written by tests/scenes.py.  The scene is optimised on the device; the joint gradient of the optimised trajectory is
// taken, Dp and the segment times are optimised together (once with bad options, once for real), and everything is
// printed as one JSON object that tests/test_gpu_joint_shim.py checks against the Python binding.
//
//   gtop_joint_shim <scene.txt> [max_evals = 20]
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"
#include "scene_file.h"

using namespace gtop_amd;
using scene_file::put_list;

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
  // the JSON is collected and printed at the end: the optimizer reports on stdout while it runs
  std::string json = "{\n";
  {   // before a path is set there is nothing to differentiate
    double c = 0.0;
    std::vector<double> gx, gT;
    const bool got = opt.jointGradient(&c, &gx, &gT);
    const bool moved = opt.optimizeJoint(GradTrajOptimizer::JointOptConfig());
    json += std::string("\"no_path\": {\"gradient\": ") + (got ? "1" : "0") + ", \"optimized\": " + (moved ? "1" : "0") +
            ", \"ok\": " + (opt.ok() ? "1" : "0") + "},\n";
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  const bool solved = opt.ok();
  const std::vector<double> x0 = opt.freeDerivatives();
  put_list(json, "x", x0.data(), x0.size(), ",\n");
  std::vector<double> T0;
  opt.getSegmentTime(T0);
  put_list(json, "T", T0.data(), T0.size(), ",\n");

  double cost = 0.0;
  std::vector<double> gx, gT;
  std::vector<std::array<double, 4>> parts;
  const bool got = opt.jointGradient(&cost, &gx, &gT, &parts);
  json += std::string("\"gradient_ok\": ") + (got && opt.ok() ? "1" : "0") + ",\n";
  put_list(json, "cost", &cost, 1, ",\n");
  put_list(json, "gx", gx.data(), gx.size(), ",\n");
  put_list(json, "gT", gT.data(), gT.size(), ",\n");
  std::vector<double> flat;
  for (const auto &p : parts) flat.insert(flat.end(), p.begin(), p.end());
  put_list(json, "parts", flat.data(), flat.size(), ",\n");

  GradTrajOptimizer::JointOptConfig bad;
  bad.t_min = 0.01;   // below 0.0301: refused, nothing changes
  const bool bad_moved = opt.optimizeJoint(bad);
  std::vector<double> T_after_bad;
  opt.getSegmentTime(T_after_bad);
  json += std::string("\"bad\": {\"optimized\": ") + (bad_moved ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") +
          ", \"unchanged\": " + (T_after_bad == T0 && opt.freeDerivatives() == x0 ? "1" : "0") + "},\n";

  GradTrajOptimizer::JointOptConfig jc;
  jc.rho = 2.0;
  jc.max_evals = 15;
  GradTrajOptimizer::JointOptInfo ji;
  const bool moved = opt.optimizeJoint(jc, &ji);
  std::vector<double> T1;
  opt.getSegmentTime(T1);
  const double info[8] = {(double)ji.code, (double)ji.evaluations, ji.f_start, ji.f, ji.cost, ji.time_sum,
                          ji.free_gradient_x, ji.free_gradient_t};
  json += std::string("\"optimized\": ") + (moved && opt.ok() ? "1" : "0") + ",\n";
  put_list(json, "info", info, 8, ",\n");
  put_list(json, "x_new", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ",\n");
  put_list(json, "T_new", T1.data(), T1.size(), ",\n");

  // the object's problem is the new point: its next gradient call runs there
  double cost1 = 0.0;
  opt.jointGradient(&cost1, nullptr, nullptr);
  put_list(json, "cost_at_new", &cost1, 1, ",\n");
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return solved ? 0 : 2;
}
