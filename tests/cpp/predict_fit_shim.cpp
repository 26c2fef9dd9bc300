// predict_fit_shim.cpp — GradTrajOptimizer::fitObstaclePredictions (csrc/grad_traj_optimizer.hpp) on a scene file
// written by tests/scenes.py with two more entries,
//   histories N    followed by, per object: its count, count rows x y z t (oldest first), then its 3 extents
//   start_time t0
// The info rows the fit returns and the report of the straight-line start with the boxes in force, as one JSON object
// that tests/test_gpu_prediction_shim.py checks against the Python binding's host fit and report on the same inputs;
// before that, a list with one empty history, which is refused and changes nothing.
//
//   gtop_predict_fit_shim <scene.txt> <mode> <degree> <lambda> <horizon> <inflate> <regularise_horizon>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"
#include "scene_file.h"

using namespace gtop_amd;

int main(int argc, char **argv) {
  if (argc < 8) {
    std::fprintf(stderr, "usage: %s <scene.txt> <mode> <degree> <lambda> <horizon> <inflate> <regularise_horizon>\n", argv[0]);
    return 1;
  }
  double start_time = 0.0;
  std::vector<GradTrajOptimizer::History> histories;
  std::vector<Vec3> scales;
  const auto more = [&](const std::string &key, std::istream &in, bool &good) {
    if (key == "start_time") good = bool(in >> start_time);
    else if (key == "histories") {
      size_t objects = 0;
      good = bool(in >> objects);
      histories.resize(good ? objects : 0);
      scales.resize(histories.size());
      for (size_t b = 0; good && b < objects; ++b) {
        size_t count = 0;
        good = bool(in >> count);
        histories[b].resize(good ? count : 0);
        for (auto &smp : histories[b]) good = good && bool(in >> smp[0] >> smp[1] >> smp[2] >> smp[3]);
        good = good && bool(in >> scales[b][0] >> scales[b][1] >> scales[b][2]);
      }
    } else return false;
    return true;
  };
  scene_file::Scene sc;
  if (!scene_file::read_scene(argv[1], sc, 0, more)) return 1;
  GradTrajOptimizer::PredictOptions po;
  po.mode = std::atoi(argv[2]);
  po.degree = std::atoi(argv[3]);
  po.lambda = std::atof(argv[4]);
  po.horizon = std::atof(argv[5]);
  po.inflate = std::atof(argv[6]);
  po.regularise_horizon = std::atoi(argv[7]) != 0;
  GradTrajOptimizer opt{GradTrajOptimizer::Config()};
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  opt.initSDFMap(sc.map_size, sc.origin, sc.resolution);
  opt.updateSDFMap(sc.obstacles);
  opt.setPath(sc.waypoints);
  opt.setStartTime(start_time);
  if (!opt.ok()) {
    std::fprintf(stderr, "%s\n", opt.lastError());
    return 2;
  }
  GradTrajOptimizer::Limits lim;
  lim.margin = 0.3;
  lim.use_boxes = true;
  std::string json = "{";
  const auto report = [&](const char *name, const char *tail) {
    GradTrajOptimizer::Report r;
    const bool pass = opt.validateTrajectory(lim, &r);
    const double v[12] = {(double)r.n_samples, r.clearance, r.clearance_time, (double)r.clearance_index,
                          (double)r.n_below_margin, r.first_below_time, (double)r.n_out_of_map, r.max_vel_norm,
                          r.max_acc_norm, r.max_vel_axis, r.max_acc_axis, r.time_sum};
    json += std::string("\"") + name + "_pass\": " + (pass && opt.ok() ? "1" : "0") + ", ";
    scene_file::put_list(json, name, v, 12, tail);
  };
  report("report_static", ",\n");
  // one object without samples: the whole list is refused, nothing is set
  std::vector<GradTrajOptimizer::History> holed = histories;
  if (!holed.empty()) holed.back().clear();
  const std::vector<GradTrajOptimizer::PredictInfo> refused = opt.fitObstaclePredictions(holed, scales, po);
  json += std::string("\"refused\": ") + (opt.ok() ? "0" : "1") + ", ";
  if (!refused.empty()) scene_file::put_list(json, "refused_last", refused.back().data(), 12, ",\n");
  report("report_after_refusal", ",\n");
  const std::vector<GradTrajOptimizer::PredictInfo> info = opt.fitObstaclePredictions(histories, scales, po);
  const bool fitted = opt.ok();
  std::vector<double> flat;
  for (const auto &row : info) flat.insert(flat.end(), row.begin(), row.end());
  scene_file::put_list(json, "info", flat.data(), flat.size(), ",\n");
  report("report", ",\n");
  std::vector<double> seg_time;
  opt.getSegmentTime(seg_time);
  scene_file::put_list(json, "segment_times", seg_time.data(), seg_time.size(), ",\n");
  scene_file::put_list(json, "x", opt.freeDerivatives().data(), opt.freeDerivatives().size(), "}\n");
  std::fputs(json.c_str(), stdout);
  return fitted && opt.ok() ? 0 : 2;
}
