// certify_shim.cpp — GradTrajOptimizer::certifyTrajectory (csrc/grad_traj_optimizer.hpp) on a scene file written by
// tests/scenes.py.  The scene is optimised on the device; the certificate of the optimised trajectory is then taken at
// two margins (0.05 and 2.0: a room the path keeps and one it cannot) and with bad options, and printed with the free
// derivatives as one JSON object that tests/test_gpu_certify_shim.py checks against the Python binding.
//
//   gtop_certify_shim <scene.txt> [max_evals = 20]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"

using namespace gtop_amd;

namespace {

bool read_points(std::istream &in, std::vector<Vec3> &out) {
  size_t count = 0;
  if (!(in >> count)) return false;
  out.resize(count);
  for (Vec3 &p : out)
    if (!(in >> p[0] >> p[1] >> p[2])) return false;
  return true;
}

// the JSON is collected and printed at the end: the optimizer reports on stdout while it runs
std::string json;

void put_list(const char *name, const double *v, size_t count, const char *tail) {
  json += std::string("\"") + name + "\": [";
  char buf[64];
  for (size_t i = 0; i < count; ++i) {
    if (std::isinf(v[i])) std::snprintf(buf, sizeof buf, "%s%sInfinity", i ? ", " : "", v[i] < 0 ? "-" : "");
    else std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]);
    json += buf;
  }
  json += std::string("]") + tail;
}

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
  put_list("cert", row, 8, "},\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <scene.txt> [max_evals]\n", argv[0]);
    return 1;
  }
  Vec3 map_size{}, origin{};
  double resolution = 0.0;
  std::vector<Vec3> obstacles, waypoints;
  std::ifstream in(argv[1]);
  std::string key;
  while (in >> key) {
    bool good = true;
    if (key == "map_size") good = bool(in >> map_size[0] >> map_size[1] >> map_size[2]);
    else if (key == "origin") good = bool(in >> origin[0] >> origin[1] >> origin[2]);
    else if (key == "resolution") good = bool(in >> resolution);
    else if (key == "obstacles") good = read_points(in, obstacles);
    else if (key == "waypoints") good = read_points(in, waypoints);
    else good = false;
    if (!good) {
      std::fprintf(stderr, "scene file: bad entry '%s'\n", key.c_str());
      return 1;
    }
  }
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
  opt.initSDFMap(map_size, origin, resolution);
  opt.updateSDFMap(obstacles);
  opt.setPath(waypoints);
  opt.optimizeTrajectory(OPT_SECOND_STEP);
  const bool solved = opt.ok();
  put_certificate("tight", opt, 0.05, 2, 256);
  put_certificate("wide", opt, 2.0, 2, 256);
  put_certificate("level0", opt, 0.05, 0, 0);
  put_certificate("bad_depth", opt, 0.05, 4, 256);
  put_list("x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ",\n");
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return solved ? 0 : 2;
}
