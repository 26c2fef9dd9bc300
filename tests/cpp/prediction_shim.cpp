// prediction_shim.cpp — GradTrajOptimizer::setMovingObstaclePredictions (csrc/grad_traj_optimizer.hpp) on a scene file
// written by tests/scenes.py with two more entries,
//   predictions N      followed by N rows: 18 coefficients (axis-major, ascending powers), t1, t2, 3 extents
//   start_time t0
// The cost function at the straight-line start (step 1) and after a short optimisation (step 2), with the free
// derivatives each was taken at, as one JSON object that tests/test_gpu_box_polynomials.py checks against the Python
// binding's gtop_cost_nlopt on the same inputs.
//
//   gtop_prediction_shim <scene.txt> [max_evals = 40] [optimize_on_device = 0]
#include <cstdio>
#include <cstdlib>
#include <array>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"
#include "scene_file.h"

using namespace gtop_amd;

namespace {

std::string list_json(const char *name, const std::vector<double> &v) {
  std::string out = std::string("\"") + name + "\": [";
  char buf[64];
  for (size_t i = 0; i < v.size(); ++i) {
    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]);
    out += buf;
  }
  return out + "]";
}

std::string state_json(const char *name, GradTrajOptimizer &opt) {
  std::vector<double> x = opt.freeDerivatives(), grad;
  const double cost = GradTrajOptimizer::costFunc(x, grad, &opt);
  char buf[128];
  std::snprintf(buf, sizeof buf, "\"%s\": {\"ok\": %d, \"cost\": %.17g, ", name, opt.ok() ? 1 : 0, cost);
  return std::string(buf) + list_json("x", x) + ", " + list_json("grad", grad) + "}";
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <scene.txt> [max_evals] [optimize_on_device]\n", argv[0]);
    return 1;
  }
  double start_time = 0.0;
  std::vector<Vec3> scale;
  std::vector<GradTrajOptimizer::Poly3> coef;
  std::vector<std::array<double, 2>> t_range;
  const auto more = [&](const std::string &key, std::istream &in, bool &good) {
    if (key == "start_time") good = bool(in >> start_time);
    else if (key == "predictions") {
      size_t count = 0;
      good = bool(in >> count);
      coef.resize(count);
      t_range.resize(count);
      scale.resize(count);
      for (size_t b = 0; good && b < count; ++b) {
        for (double &c : coef[b]) good = good && bool(in >> c);
        good = good && bool(in >> t_range[b][0] >> t_range[b][1] >> scale[b][0] >> scale[b][1] >> scale[b][2]);
      }
    } else return false;
    return true;
  };
  scene_file::Scene sc;
  if (!scene_file::read_scene(argv[1], sc, 0, more)) return 1;
  GradTrajOptimizer::Config cfg;
  cfg.max_evals = argc > 2 ? std::atoi(argv[2]) : 40;
  cfg.time_limit_2 = 5.0;          // evaluation-capped so the run is reproducible
  cfg.optimize_on_device = argc > 3 ? std::atoi(argv[3]) : 0;
  GradTrajOptimizer opt(cfg);
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  // a list the interface refuses (t1 > t2) is reported and changes nothing
  std::vector<std::array<double, 2>> backwards = t_range;
  if (!backwards.empty()) backwards[0] = {1.0, 0.0};
  opt.setMovingObstaclePredictions(coef, backwards, scale);
  const bool refused = !opt.ok();
  opt.setMovingObstaclePredictions(coef, t_range, scale);
  opt.setStartTime(start_time);
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  const std::string start = state_json("start", opt);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  const std::string optimised = state_json("optimised", opt);
  std::vector<double> seg_time;
  opt.getSegmentTime(seg_time);
  std::printf("{\"refused\": %d, %s,\n%s,\n%s}\n", refused ? 1 : 0, list_json("segment_times", seg_time).c_str(),
              start.c_str(), optimised.c_str());
  return opt.ok() ? 0 : 2;
}
