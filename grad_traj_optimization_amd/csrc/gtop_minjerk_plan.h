// gtop_minjerk_plan.h — the launch plan of the minimum-jerk start point (gtop_minjerk.hip) and the ONE statement of
// its rule: one lane per trajectory; a lane keeps the three doubles per interior waypoint of its eliminated diagonal
// blocks in LDS, lane-interleaved, so the lanes of a workgroup fall as the segment count grows.  The launcher takes the
// grid, the workgroup and the LDS bytes from gtop_minjerk_plan, the kernel its LDS index from the function below.  No
// HIP header: gtop_minjerk_plan.cpp builds with a host compiler alone (tests/test_minjerk_plan.py).
#ifndef GTOP_MINJERK_PLAN_H_
#define GTOP_MINJERK_PLAN_H_

#include <stddef.h>

#include "gtop_launch_rule.h"   // GTOP_HD

constexpr int kMinJerkMinSegments = 2;
constexpr int kMinJerkMaxSegments = 227;     // the evaluation's own limit (gtop_launch_rule.h)
constexpr int kMinJerkBlockDoubles = 3;      // the inverse of a symmetric 2 x 2 block
constexpr int kMinJerkMaxLanes = 64;         // one wavefront per workgroup at the most
constexpr int kMinJerkMinLanes = 8;
constexpr size_t kMinJerkLdsBudget = 65536;  // bytes of LDS a workgroup may ask for without an attribute of its own

struct GtopMinJerkPlan {
  bool supported;      // false: m out of range or B < 0 (everything below is 0 then)
  int lanes;           // trajectories (= threads) per workgroup: 64, 32, 16 or 8
  unsigned blocks;     // workgroups: ceil(B / lanes); 0 for B = 0 (nothing is launched)
  size_t lds_bytes;    // lanes * 24 (m - 1)
};

// Trajectories per workgroup: the largest power of two from 64 down to 8 whose blocks fit the budget —
// 64 up to 43 segments, 32 up to 86, 16 up to 171, 8 up to the limit of 227.
GTOP_HD constexpr int gtop_minjerk_lanes(int m) {
  int lanes = kMinJerkMaxLanes;
  while (lanes > kMinJerkMinLanes &&
         (size_t)lanes * kMinJerkBlockDoubles * sizeof(double) * (size_t)(m - 1) > kMinJerkLdsBudget)
    lanes >>= 1;
  return lanes;
}

// LDS slot (in doubles) of entry c (0 .. 2) of interior waypoint k (1 .. m - 1) of lane `lane`: consecutive lanes hold
// consecutive doubles, so a wavefront's 8-byte accesses fall on distinct banks.
GTOP_HD constexpr int gtop_minjerk_slot(int k, int c, int lane, int lanes) {
  return ((k - 1) * kMinJerkBlockDoubles + c) * lanes + lane;
}

// The plan of B trajectories of m segments; returns plan->supported.
bool gtop_minjerk_plan(int B, int m, GtopMinJerkPlan *plan);

#endif  // GTOP_MINJERK_PLAN_H_
