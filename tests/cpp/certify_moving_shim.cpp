// certify_moving_shim.cpp — GradTrajOptimizer::certifyTrajectoryMoving beside certifyTrajectory
// (csrc/grad_traj_optimizer.hpp) on a scene file written by tests/scenes.py.  The scene's waypoints are flown at a
// steady velocity along x with the segment times given (setKinoPath: nothing is optimised), past one constant-velocity
// box at a start time; both certificates, and the moving one again with the box as a polynomial prediction and once
// more with no box at all, are printed with the free derivatives as one JSON object that
// tests/test_gpu_certify_moving_shim.py checks against the Python binding.
//
//   gtop_certify_moving_shim <scene.txt> <speed> <t0> <margin> <9 numbers: the box's p0, vel, scale> <segment times...>
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

std::string json;

void put_certificate(const char *name, GradTrajOptimizer &opt, bool moving, double margin, int max_depth) {
  GradTrajOptimizer::CertifyOptions o;
  o.margin = margin;
  o.max_depth = max_depth;
  o.max_refine = 64;
  GradTrajOptimizer::CertifyReport r;
  const bool safe = moving ? opt.certifyTrajectoryMoving(o, r) : opt.certifyTrajectory(o, r);
  const double row[8] = {(double)r.verdict, r.lo, r.hi, r.hi_time, r.first_violation_time, (double)r.n_undecided,
                         (double)r.n_refinements, r.time_sum};
  json += std::string("\"") + name + "\": {\"safe\": " + (safe ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") + ", ";
  put_list(json, "cert", row, 8, "},\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 16) {
    std::fprintf(stderr, "usage: %s <scene.txt> <speed> <t0> <margin> <box p0 vel scale: 9> <segment times: 2 or more>\n",
                 argv[0]);
    return 1;
  }
  scene_file::Scene sc;
  if (!scene_file::read_scene(argv[1], sc)) return 1;
  const double speed = std::atof(argv[2]), t0 = std::atof(argv[3]), margin = std::atof(argv[4]);
  Vec3 p0{}, vel{}, scale{};
  for (int k = 0; k < 3; ++k) {
    p0[k] = std::atof(argv[5 + k]);
    vel[k] = std::atof(argv[8 + k]);
    scale[k] = std::atof(argv[11 + k]);
  }
  std::vector<double> times;
  for (int i = 14; i < argc; ++i) times.push_back(std::atof(argv[i]));
  const int m = (int)times.size();
  if ((int)sc.waypoints.size() != m + 1) {
    std::fprintf(stderr, "%d segment times for %zu waypoints\n", m, sc.waypoints.size());
    return 1;
  }
  GradTrajOptimizer opt;
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  json += "{\n";
  {   // before a path is set there is nothing to certify
    GradTrajOptimizer::CertifyReport r;
    const bool safe = opt.certifyTrajectoryMoving(GradTrajOptimizer::CertifyOptions(), r);
    json += std::string("\"no_path\": {\"safe\": ") + (safe ? "1" : "0") + ", \"ok\": " + (opt.ok() ? "1" : "0") + "},\n";
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  Matrix Pos, Vel, Acc;
  Pos.resize(m + 1, 3);
  Vel.resize(m + 1, 3);
  Acc.resize(m + 1, 3);
  for (int i = 0; i < m + 1; ++i) {
    for (int a = 0; a < 3; ++a) Pos(i, a) = sc.waypoints[i][a];
    Vel(i, 0) = speed;
  }
  opt.setKinoPath(Pos, Vel, Acc, times);
  const bool set = opt.ok();
  put_certificate("no_boxes", opt, true, margin, 2);       // no list: certifyTrajectory's own result
  opt.setMovingObstacles({p0}, {vel}, {scale});
  opt.setStartTime(t0);
  put_certificate("static", opt, false, margin, 2);
  put_certificate("moving", opt, true, margin, 2);
  put_certificate("bad_depth", opt, true, margin, 4);
  GradTrajOptimizer::Poly3 coef{};                        // the same box as a prediction: c0 = p0, c1 = vel, unbounded
  for (int k = 0; k < 3; ++k) {
    coef[6 * k] = p0[k];
    coef[6 * k + 1] = vel[k];
  }
  opt.setMovingObstaclePredictions({coef}, {}, {scale});
  put_certificate("moving_poly", opt, true, margin, 2);
  put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ",\n");
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return set ? 0 : 2;
}
