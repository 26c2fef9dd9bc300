// scene_file.h — what the programs of tests/cpp that run a scene share: the reader of the scene files tests/scenes.py
// writes, and the writer of a JSON list of doubles.
//
// A scene file is a sequence of entries `key values...`:
//   map_size x y z | origin x y z | resolution r | obstacles N (N points) | waypoints N (N points)
// and, of a kinodynamic front end (KINO): velocities N (N points) | accelerations N (N points) | segment_times N (N values).
#ifndef GTOP_TESTS_SCENE_FILE_H_
#define GTOP_TESTS_SCENE_FILE_H_

#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <string>
#include <vector>

#include "grad_traj_optimizer.hpp"

namespace scene_file {

using gtop_amd::Vec3;

struct Scene {
  Vec3 map_size{}, origin{};
  double resolution = 0.0;
  std::vector<Vec3> obstacles, waypoints, vel, acc;
  std::vector<double> seg_time;   // with vel / acc: the kinodynamic form (setKinoPath)
};

inline bool read_points(std::istream &in, std::vector<Vec3> &out) {
  size_t count = 0;
  if (!(in >> count)) return false;
  out.resize(count);
  for (Vec3 &p : out)
    if (!(in >> p[0] >> p[1] >> p[2])) return false;
  return true;
}

// KINO: the three kinodynamic keys are read too (without it they are bad entries, like any unknown key).
// LENIENT (gtop_batch_devices): nothing is written to stderr, and an entry whose values do not parse ends the reading
// instead of failing it; an unknown key still fails.
enum : unsigned { KINO = 1, LENIENT = 2 };
// The keys one program reads beyond these: whether `key` is one of them, and in `good` whether its values parsed.
using MoreKeys = std::function<bool(const std::string &key, std::istream &in, bool &good)>;

// false: a bad entry (reported on stderr as "scene file: bad entry '<key>'"); the caller exits with 1
inline bool read_scene(const char *file, Scene &sc, unsigned flags = 0, const MoreKeys &more = nullptr) {
  const bool kino = (flags & KINO) != 0, lenient = (flags & LENIENT) != 0;
  std::ifstream in(file);
  std::string key;
  while (in >> key) {
    bool good = true;
    if (key == "map_size") good = bool(in >> sc.map_size[0] >> sc.map_size[1] >> sc.map_size[2]);
    else if (key == "origin") good = bool(in >> sc.origin[0] >> sc.origin[1] >> sc.origin[2]);
    else if (key == "resolution") good = bool(in >> sc.resolution);
    else if (key == "obstacles") good = read_points(in, sc.obstacles);
    else if (key == "waypoints") good = read_points(in, sc.waypoints);
    else if (kino && key == "velocities") good = read_points(in, sc.vel);
    else if (kino && key == "accelerations") good = read_points(in, sc.acc);
    else if (kino && key == "segment_times") {
      size_t count = 0;
      good = bool(in >> count);
      sc.seg_time.resize(good ? count : 0);
      for (double &t : sc.seg_time) good = good && bool(in >> t);
    } else if (!(more && more(key, in, good))) {
      if (lenient) return false;
      good = false;
    }
    if (!good && !lenient) {
      std::fprintf(stderr, "scene file: bad entry '%s'\n", key.c_str());
      return false;
    }
  }
  return true;
}

// `"name": [v0, v1, ...]` + tail appended to json: %.17g, an infinity as JSON's Infinity / -Infinity
inline void put_list(std::string &json, const char *name, const double *v, size_t count, const char *tail) {
  json += std::string("\"") + name + "\": [";
  char buf[64];
  for (size_t i = 0; i < count; ++i) {
    if (std::isinf(v[i])) std::snprintf(buf, sizeof buf, "%s%sInfinity", i ? ", " : "", v[i] < 0 ? "-" : "");
    else std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]);
    json += buf;
  }
  json += std::string("]") + tail;
}

}  // namespace scene_file

#endif  // GTOP_TESTS_SCENE_FILE_H_
