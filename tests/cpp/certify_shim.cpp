// certify_shim.cpp — GradTrajOptimizer::certifyTrajectory (csrc/grad_traj_optimizer.hpp) on a scene file written by
// tests/scenes.py.  The scene is optimised on the device; the certificate of the optimised trajectory is then taken at
// two margins (0.05 and 2.0: a room the path keeps and one it cannot) and with bad options, and printed with the free
// derivatives as one JSON object that tests/test_gpu_certify_shim.py checks against the Python binding.
//
//   gtop_certify_shim <scene.txt> [max_evals = 20]
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

void put_certificate(const char *name, GradTrajOptimizer &opt, double margin, int max_depth, int max_refine) {
  GradTrajOptimizer::CertifyOptions o;
  o.margin = margin;
  o.max_depth = max_depth;
  o.max_refine = max_refine;
  GradTrajOptimizer::CertifyReport r;
  const bool safe = opt.certifyTrajectory(o, r);
  const double row[8] = {(double)r.verdict, r.lo, r.hi, r.hi_time, r.first_violation_time, (double)r.n_undecided,
                         (double)r.n_refinements, r.time_sum};
  json += std::string("\"") + name + "\": {\"safe\": " + (safe ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") + ", ";
  put_list(json, "cert", row, 8, "},\n");
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
    GradTrajOptimizer::CertifyReport r;
    const bool safe = opt.certifyTrajectory(GradTrajOptimizer::CertifyOptions(), r);
    json += std::string("\"no_path\": {\"safe\": ") + (safe ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") + "},\n";
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  const bool solved = opt.ok();
  put_certificate("tight", opt, 0.05, 2, 256);
  put_certificate("wide", opt, 2.0, 2, 256);
  put_certificate("level0", opt, 0.05, 0, 0);
  put_certificate("bad_depth", opt, 0.05, 4, 256);
  put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ",\n");
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return solved ? 0 : 2;
}
