// minjerk_shim.cpp — GradTrajOptimizer::Config::initial_guess (csrc/grad_traj_optimizer.hpp) on a scene file written
// by tests/scenes.py: the start point setPath (or, with velocities / accelerations / segment_times in the file,
// setKinoPath) leaves in Dp with initial_guess 0 and 1, with the segment times and the coefficients — and, for a plain
// waypoint list, the start coefficients GradTrajBatch::setPaths leaves for the list and for its first four waypoints —
// as one JSON object that tests/test_gpu_minjerk_shim.py checks against gtop_min_jerk_start.
//
//   gtop_minjerk_shim <scene.txt>
#include <cstdio>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"
#include "scene_file.h"

using namespace gtop_amd;
using scene_file::put_list;

namespace {

Matrix rows_of(const std::vector<Vec3> &pts) {
  Matrix mat((int)pts.size(), 3);
  for (size_t i = 0; i < pts.size(); ++i)
    for (int a = 0; a < 3; ++a) mat((int)i, a) = pts[i][a];
  return mat;
}

// the JSON is collected and printed at the end: libraries loaded on the way (a group's collective backend) may write
// to stdout themselves
std::string json;

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <scene.txt>\n", argv[0]);
    return 1;
  }
  scene_file::Scene sc;   // (no map is needed: map_size, origin, resolution and obstacles are read and left)
  if (!scene_file::read_scene(argv[1], sc, scene_file::KINO)) return 1;
  const std::vector<Vec3> &waypoints = sc.waypoints;
  const bool kino = !sc.seg_time.empty();
  json += kino ? "{\"kino\": 1,\n" : "{\"kino\": 0,\n";
  bool all_ok = true;
  for (int guess = 0; guess < 2; ++guess) {
    GradTrajOptimizer::Config cfg;
    cfg.initial_guess = guess;
    GradTrajOptimizer opt(cfg);
    if (!opt.ok()) {
      std::fprintf(stderr, "%s\n", opt.lastError());
      return 2;
    }
    if (kino) opt.setKinoPath(rows_of(waypoints), rows_of(sc.vel), rows_of(sc.acc), sc.seg_time);
    else opt.setPath(waypoints);
    all_ok = all_ok && opt.ok();
    std::vector<double> T;
    opt.getSegmentTime(T);
    Matrix coeff;
    opt.getCoefficient(coeff);
    json += std::string("\"guess") + (guess ? "1" : "0") + "\": {\"ok\": " + (opt.ok() ? "1" : "0") + ", ";
    put_list(json, "segment_times", T.data(), T.size(), ", ");
    put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ", ");
    const bool batch_too = !kino && waypoints.size() >= 4;
    put_list(json, "coeff", coeff.a.data(), coeff.a.size(), batch_too ? ", " : "");
    if (batch_too) {
      // GradTrajBatch forms its own start points: the whole list and its first four waypoints (two segment counts,
      // one device problem each); before an optimisation getCoefficient gives the start point's coefficients
      GradTrajBatch batch({0}, cfg);
      batch.setPaths({waypoints, std::vector<Vec3>(waypoints.begin(), waypoints.begin() + 4)});
      all_ok = all_ok && batch.ok();
      json += batch.ok() ? "\"batch_ok\": 1, " : "\"batch_ok\": 0, ";
      Matrix c0, c1;
      batch.getCoefficient(0, c0);
      batch.getCoefficient(1, c1);
      put_list(json, "batch_coeff0", c0.a.data(), c0.a.size(), ", ");
      put_list(json, "batch_coeff1", c1.a.data(), c1.a.size(), "");
    }
    json += guess ? "}\n" : "},\n";
  }
  json += "}\n";
  std::fputs(json.c_str(), stdout);
  return all_ok ? 0 : 2;
}
