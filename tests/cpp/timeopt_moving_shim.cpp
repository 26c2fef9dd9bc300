// timeopt_moving_shim.cpp — GradTrajOptimizer::timeGradientMoving and optimizeSegmentTimesMoving
// (csrc/grad_traj_optimizer.hpp) on a scene file written by tests/scenes.py.  The scene is optimised on the device; one
// constant-velocity box and a start time are set, which switches the moving-obstacle cost on: timeGradient then refuses,
// timeGradientMoving serves; the segment times are optimised under the box (once with bad options, once for real), and
// everything is printed as one JSON object that tests/test_gpu_time_moving_shim.py checks against the Python binding.
//
//   gtop_timeopt_moving_shim <scene.txt> <max_evals> <t0> <9 numbers: the box's p0, vel, scale>
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
  if (argc < 13) {
    std::fprintf(stderr, "usage: %s <scene.txt> <max_evals> <t0> <box p0 vel scale: 9>\n", argv[0]);
    return 1;
  }
  scene_file::Scene sc;
  if (!scene_file::read_scene(argv[1], sc)) return 1;
  const double t0 = std::atof(argv[3]);
  Vec3 p0{}, vel{}, scale{};
  for (int k = 0; k < 3; ++k) {
    p0[k] = std::atof(argv[4 + k]);
    vel[k] = std::atof(argv[7 + k]);
    scale[k] = std::atof(argv[10 + k]);
  }
  GradTrajOptimizer::Config cfg;
  cfg.max_evals = std::atoi(argv[2]);
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
    std::vector<double> g;
    const bool got = opt.timeGradientMoving(&c, &g);
    const bool moved = opt.optimizeSegmentTimesMoving(GradTrajOptimizer::TimeOptConfig());
    json += std::string("\"no_path\": {\"gradient\": ") + (got ? "1" : "0") + ", \"optimized\": " + (moved ? "1" : "0") +
            ", \"ok\": " + (opt.ok() ? "1" : "0") + "},\n";
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  const bool solved = opt.ok();
  put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ",\n");
  std::vector<double> T0;
  opt.getSegmentTime(T0);
  put_list(json, "T", T0.data(), T0.size(), ",\n");

  double cost = 0.0, gt0 = 0.0;
  std::vector<double> gT;
  std::vector<std::array<double, 6>> parts;
  {   // without boxes: timeGradient's numbers, the added columns 0
    std::vector<std::array<double, 4>> p4;
    double c4 = 0.0;
    std::vector<double> g4;
    const bool a = opt.timeGradient(&c4, &g4, &p4), b = opt.timeGradientMoving(&cost, &gT, &gt0, &parts);
    bool same = a && b && c4 == cost && g4 == gT && gt0 == 0.0 && parts.size() == p4.size();
    for (size_t s = 0; same && s < parts.size(); ++s) {
      for (int k = 0; k < 4; ++k) same = same && parts[s][k] == p4[s][k];
      same = same && parts[s][4] == 0.0 && parts[s][5] == 0.0;
    }
    json += std::string("\"static_same\": ") + (same ? "1" : "0") + ",\n";
  }
  opt.setMovingObstacles({p0}, {vel}, {scale});
  opt.setStartTime(t0);
  {   // the mode is on: the static call refuses, nothing changes
    double c = 0.0;
    const bool got = opt.timeGradient(&c, nullptr);
    json += std::string("\"static_refused\": ") + (!got && !opt.ok() ? "1" : "0") + ",\n";
  }
  const bool got = opt.timeGradientMoving(&cost, &gT, &gt0, &parts);
  json += std::string("\"gradient_ok\": ") + (got && opt.ok() ? "1" : "0") + ",\n";
  put_list(json, "cost", &cost, 1, ",\n");
  put_list(json, "gT", gT.data(), gT.size(), ",\n");
  put_list(json, "gt0", &gt0, 1, ",\n");
  std::vector<double> flat;
  for (const auto &p : parts) flat.insert(flat.end(), p.begin(), p.end());
  put_list(json, "parts", flat.data(), flat.size(), ",\n");

  GradTrajOptimizer::TimeOptConfig bad;
  bad.t_min = 0.01;   // below 0.0301: refused, nothing changes
  const bool bad_moved = opt.optimizeSegmentTimesMoving(bad);
  std::vector<double> T_after_bad;
  opt.getSegmentTime(T_after_bad);
  json += std::string("\"bad\": {\"optimized\": ") + (bad_moved ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") +
          ", \"unchanged\": " + (T_after_bad == T0 ? "1" : "0") + "},\n";

  GradTrajOptimizer::TimeOptConfig tc;
  tc.rho = 2.0;
  tc.max_evals = 30;
  GradTrajOptimizer::TimeOptInfo ti;
  const bool moved = opt.optimizeSegmentTimesMoving(tc, &ti);
  std::vector<double> T1;
  opt.getSegmentTime(T1);
  const double info[8] = {(double)ti.code, (double)ti.accepted, (double)ti.evaluations, ti.f_start, ti.f, ti.cost,
                          ti.free_gradient, ti.time_sum};
  json += std::string("\"optimized\": ") + (moved && opt.ok() ? "1" : "0") + ",\n";
  put_list(json, "info", info, 8, ",\n");
  put_list(json, "T_new", T1.data(), T1.size(), ",\n");

  // the object's problem is the new times
  double cost1 = 0.0;
  opt.timeGradientMoving(&cost1, nullptr);
  put_list(json, "cost_at_T_new", &cost1, 1, ",\n");
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return solved ? 0 : 2;
}
