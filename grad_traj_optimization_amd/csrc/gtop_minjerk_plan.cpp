// gtop_minjerk_plan.cpp — the launch plan of the minimum-jerk start point (gtop_minjerk_plan.h): every decision
// gtop_launch_min_jerk_start (gtop_minjerk.hip) takes from the batch and the segment count.  Host only, no HIP.
#include "gtop_minjerk_plan.h"

bool gtop_minjerk_plan(int B, int m, GtopMinJerkPlan *plan) {
  GtopMinJerkPlan p{};
  p.supported = B >= 0 && m >= kMinJerkMinSegments && m <= kMinJerkMaxSegments;
  if (p.supported) {
    p.lanes = gtop_minjerk_lanes(m);
    p.blocks = (unsigned)(((size_t)B + p.lanes - 1) / p.lanes);
    p.lds_bytes = (size_t)p.lanes * kMinJerkBlockDoubles * sizeof(double) * (size_t)(m - 1);
  }
  *plan = p;
  return p.supported;
}
