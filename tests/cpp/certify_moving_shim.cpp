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
  put_list("cert", row, 8, "},\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 16) {
    std::fprintf(stderr, "usage: %s <scene.txt> <speed> <t0> <margin> <box p0 vel scale: 9> <segment times: 2 or more>\n",
                 argv[0]);
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
  if ((int)waypoints.size() != m + 1) {
    std::fprintf(stderr, "%d segment times for %zu waypoints\n", m, waypoints.size());
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
  opt.initSDFMap(map_size, origin, resolution);
  opt.updateSDFMap(obstacles);
  Matrix Pos, Vel, Acc;
  Pos.resize(m + 1, 3);
  Vel.resize(m + 1, 3);
  Acc.resize(m + 1, 3);
  for (int i = 0; i < m + 1; ++i) {
    for (int a = 0; a < 3; ++a) Pos(i, a) = waypoints[i][a];
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
  put_list("x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), ",\n");
  json += "\"done\": 1}\n";
  std::fputs(json.c_str(), stdout);
  return set ? 0 : 2;
}
