// The launch plan of the minimum-jerk start point (csrc/gtop_minjerk_plan.{h,cpp}) as text, and its LDS slot map walked
// on the host: tests/test_minjerk_plan.py and tests/test_gpu_minjerk.py (through tests/minjerk_plan.py) read the output.
// Plain C++, no HIP.
//   minjerk_plan_dump plan B M [B M ...]   one line of key=value per pair
//   minjerk_plan_dump consts                the limits
//   minjerk_plan_dump slots                 every (waypoint, entry, lane) of every supported m has a slot of its own
//                                           inside the planned LDS bytes: one line per violation
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gtop_minjerk_plan.h"

namespace {

int plans(int argc, char **argv) {
  if (argc < 4 || (argc - 2) % 2) return 2;
  for (int i = 2; i + 1 < argc; i += 2) {
    const int B = atoi(argv[i]), m = atoi(argv[i + 1]);
    GtopMinJerkPlan p;
    const bool ok = gtop_minjerk_plan(B, m, &p);
    if (ok != p.supported) return 3;
    printf("B=%d m=%d supported=%d lanes=%d blocks=%u lds_bytes=%zu\n", B, m, (int)p.supported, p.lanes, p.blocks,
           p.lds_bytes);
  }
  return 0;
}

int slots() {
  int bad = 0;
  for (int m = kMinJerkMinSegments; m <= kMinJerkMaxSegments; ++m) {
    GtopMinJerkPlan p;
    if (!gtop_minjerk_plan(1, m, &p)) {
      if (++bad <= 50) printf("m=%d: refused\n", m);
      continue;
    }
    const size_t doubles = p.lds_bytes / sizeof(double);
    std::vector<int> owners(doubles, 0);
    for (int k = 1; k < m; ++k)
      for (int c = 0; c < kMinJerkBlockDoubles; ++c)
        for (int lane = 0; lane < p.lanes; ++lane) {
          const int s = gtop_minjerk_slot(k, c, lane, p.lanes);
          if (s < 0 || (size_t)s >= doubles) {
            if (++bad <= 50) printf("m=%d k=%d c=%d lane=%d: slot %d outside %zu doubles\n", m, k, c, lane, s, doubles);
            continue;
          }
          ++owners[s];
          // consecutive lanes, consecutive doubles: a wavefront's 8-byte accesses fall on distinct banks
          if (lane && s != gtop_minjerk_slot(k, c, lane - 1, p.lanes) + 1 && ++bad <= 50)
            printf("m=%d k=%d c=%d lane=%d: not next to lane %d\n", m, k, c, lane, lane - 1);
        }
    for (size_t s = 0; s < doubles; ++s)
      if (owners[s] != 1 && ++bad <= 50) printf("m=%d: slot %zu owned %d times\n", m, s, owners[s]);
  }
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "plan")) return plans(argc, argv);
  if (argc > 1 && !strcmp(argv[1], "slots")) return slots();
  if (argc > 1 && !strcmp(argv[1], "consts")) {
    printf("min_segments=%d max_segments=%d block_doubles=%d max_lanes=%d min_lanes=%d lds_budget=%zu\n",
           kMinJerkMinSegments, kMinJerkMaxSegments, kMinJerkBlockDoubles, kMinJerkMaxLanes, kMinJerkMinLanes,
           kMinJerkLdsBudget);
    return 0;
  }
  return 2;
}
