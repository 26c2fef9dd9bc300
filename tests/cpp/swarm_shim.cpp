// swarm_shim.cpp — GradTrajOptimizer::swarmGradient and optimizeSwarm (csrc/grad_traj_optimizer.hpp) on a scene file
// written by tests/scenes.py.  Three robots share the scene's map: the first flies the scene's waypoints, the second the
// same waypoints the other way round, the third the first's lifted by 0.4 m — so their plans meet.  Each is optimised on
// the device alone; then the swarm gradient of the three plans is taken and the swarm is optimised (once with bad
// options, once for real).  Everything is printed as one JSON object that tests/test_gpu_swarm_shim.py checks against
// the Python binding.
//
//   gtop_swarm_shim <scene.txt> [max_evals = 10]
#include <array>
#include <cstdio>
#include <cstdlib>
#include <memory>
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
  cfg.max_evals = argc > 2 ? std::atoi(argv[2]) : 10;
  cfg.time_limit_2 = 5.0;            // evaluation-capped so the run is reproducible
  cfg.optimize_on_device = 1;
  std::vector<std::vector<Vec3>> paths(3, sc.waypoints);
  for (size_t i = 0; i < sc.waypoints.size(); ++i) paths[1][i] = sc.waypoints[sc.waypoints.size() - 1 - i];
  for (Vec3 &p : paths[2]) p[2] += 0.4;

  std::vector<std::unique_ptr<GradTrajOptimizer>> own;
  std::vector<GradTrajOptimizer *> robots;
  for (int r = 0; r < 3; ++r) {
    own.emplace_back(new GradTrajOptimizer(cfg));
    if (!own.back()->ok()) {
      std::fprintf(stderr, "%s\n", own.back()->lastError());
      return 2;
    }
    robots.push_back(own.back().get());
  }
  // the JSON is collected and printed at the end: the optimizer reports on stdout while it runs
  std::string json = "{\n";
  GradTrajOptimizer::SwarmOptions so;
  so.dt = 0.05;
  so.n_samples = 200;
  so.w = 50.0;
  so.radius = 1.0;
  so.sweeps = 2;
  so.evals_per_sweep = 8;
  {   // before a path is set there is no swarm
    std::vector<double> S;
    const bool got = GradTrajOptimizer::swarmGradient(robots, so, &S, nullptr);
    const bool moved = GradTrajOptimizer::optimizeSwarm(robots, so);
    json += std::string("\"no_path\": {\"gradient\": ") + (got ? "1" : "0") + ", \"optimized\": " + (moved ? "1" : "0") +
            ", \"ok\": " + (robots[0]->ok() ? "1" : "0") + "},\n";
  }
  bool solved = true;
  std::vector<double> x0;
  for (int r = 0; r < 3; ++r) {
    robots[r]->initSDFMap(sc.map_size, sc.origin, sc.resolution);
    robots[r]->updateSDFMap(sc.obstacles);
    robots[r]->setPath(paths[r]);
    robots[r]->optimizeTrajectory(OPT_SECOND_STEP);
    solved = solved && robots[r]->ok();
    x0.insert(x0.end(), robots[r]->freeDerivatives().begin(), robots[r]->freeDerivatives().end());
  }
  put_list(json, "x", x0.data(), x0.size(), ",\n");

  std::vector<double> S, active, flat;
  std::vector<std::vector<double>> grad;
  const bool got = GradTrajOptimizer::swarmGradient(robots, so, &S, &grad, &active);
  json += std::string("\"gradient_ok\": ") + (got && robots[0]->ok() ? "1" : "0") + ",\n";
  put_list(json, "S", S.data(), S.size(), ",\n");
  put_list(json, "active", active.data(), active.size(), ",\n");
  for (const auto &g : grad) flat.insert(flat.end(), g.begin(), g.end());
  put_list(json, "grad", flat.data(), flat.size(), ",\n");

  GradTrajOptimizer::SwarmOptions bad = so;
  bad.radius = 0.0;   // refused, nothing changes
  const bool bad_moved = GradTrajOptimizer::optimizeSwarm(robots, bad);
  std::vector<double> x_bad;
  for (int r = 0; r < 3; ++r) x_bad.insert(x_bad.end(), robots[r]->freeDerivatives().begin(), robots[r]->freeDerivatives().end());
  json += std::string("\"bad\": {\"optimized\": ") + (bad_moved ? "1" : "0") + ", \"ok\": " + (robots[0]->ok() ? "1" : "0") +
          ", \"unchanged\": " + (x_bad == x0 ? "1" : "0") + "},\n";

  std::vector<double> min_cost, x1, jflat;
  std::vector<std::array<double, 2>> joint;
  const bool moved = GradTrajOptimizer::optimizeSwarm(robots, so, &min_cost, &joint);
  json += std::string("\"optimized\": ") + (moved && robots[0]->ok() ? "1" : "0") + ",\n";
  for (int r = 0; r < 3; ++r) x1.insert(x1.end(), robots[r]->freeDerivatives().begin(), robots[r]->freeDerivatives().end());
  for (const auto &j : joint) jflat.insert(jflat.end(), j.begin(), j.end());
  put_list(json, "x_new", x1.data(), x1.size(), ",\n");
  put_list(json, "min_cost", min_cost.data(), min_cost.size(), ",\n");
  put_list(json, "joint", jflat.data(), jflat.size(), ",\n");

  // the first object's context holds its own problem again: its next optimisation runs on one row
  robots[0]->optimizeTrajectory(OPT_SECOND_STEP);
  const bool again = robots[0]->ok();
  std::vector<double> S2;
  const bool got2 = GradTrajOptimizer::swarmGradient(robots, so, &S2, nullptr);
  put_list(json, "S_after", S2.data(), S2.size(), ",\n");
  json += "\"again\": " + std::string(again && got2 ? "1" : "0") + ",\n";
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return solved && again ? 0 : 2;
}
