// gtop_insert.hip — batched waypoint insertion on gfx950 (gtop_insert_waypoints_device of include/gtop.h; DESIGN.md
// §5.16): ONE segment of each trajectory is cut at a local time tl, the new junction takes the old curve's position,
// velocity and acceleration there, and the row of m segments becomes a row of m + 1 that describes the same curve.
// (Not in the reference, whose waypoint count is fixed by setPath; the per-segment report of gtop_segments.hip names
// this remedy beside the time stretch of gtop_retime.hip.)
//
// One WAVEFRONT per trajectory, four to a workgroup that shares nothing: no LDS, no barrier, no atomics.  The decision
// (which segment, where) is wave-uniform — the arg-max of LONGEST is a wavefront reduction over ceil(m / 64) passes of
// coalesced loads, the walk of AT_TIME is segment_of (gtop_report_common.h) on every lane at once — and so is the new
// junction: every lane forms it from the 18 coefficients of the cut segment, which arrive as broadcasts.  Then the lanes
// stride over the row's 9m + (m + 1) (+ 18m with bounds) output entries; an entry is a copy through the junction map or
// one of the new values.  Every output entry is written exactly once, rows are written coalesced.
//
// Every step is ONE rounded IEEE operation in the order include/gtop.h writes it — the file is compiled unfused — so a
// numpy twin reproduces the bits (tests/insert_twin.py).  All loops are bounded by m and every index is formed from
// 0 <= s <= m - 1: a NaN or zero segment time gives garbage in that row and touches no memory but the row's own.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_device_common.h"   // poly_eval
#include "gtop_edt_lookup.h"
#include "gtop_kernels.h"
#include "gtop_report_common.h"   // segment_of

#pragma clang fp contract(off)

namespace {

constexpr int kInsertWaves = 4;   // trajectories per workgroup

struct InsertArgs {
  int B, m, t_stride, when_stride, mode;
  const double *x, *coeff, *T, *when, *lb, *ub;
  double *x_out, *T_out, *lb_out, *ub_out, *info;
  double min_fraction, push, push_below, bos, vos, aos;
};

__device__ __forceinline__ int wave_min_int(int v) {
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

// the first index of the largest of ts[0 .. m-1]: a lane keeps the first of its own largest (a later one replaces it
// only on strict >), the wavefront the lowest index among the lanes that hold the maximum.  (A row of NaN times holds
// no maximum: the index is clamped, the row is garbage.)
__device__ __forceinline__ int longest_segment(const double *__restrict__ ts, int m, int lane) {
  double best = -INFINITY;
  int at = INT32_MAX;
  for (int i = lane; i < m; i += 64) {
    const double v = ts[i];
    if (v > best || at == INT32_MAX) {
      best = v;
      at = i;
    }
  }
  const double top = wave_max(best);
  return min(wave_min_int(best == top ? at : INT32_MAX), m - 1);
}

// first and second derivative of sum_j c[j] t^j by Horner, the integer factor applied to the coefficient first
__device__ __forceinline__ double horner_vel(const double *c, double t) {
  return ((((5.0 * c[5]) * t + 4.0 * c[4]) * t + 3.0 * c[3]) * t + 2.0 * c[2]) * t + c[1];
}
__device__ __forceinline__ double horner_acc(const double *c, double t) {
  return (((20.0 * c[5]) * t + 12.0 * c[4]) * t + 6.0 * c[3]) * t + 2.0 * c[2];
}

__device__ __forceinline__ double pick3(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

// One row of 9m entries (x_out, lb_out or ub_out) from the row of 9 (m - 1) it grows out of: entry r of an axis is
// junction r / 3 + 1, component r % 3; junctions up to s are copied, junction s + 1 is new, those behind it are the old
// ones one place on.  fresh[comp][axis]: the new junction's three components.
__device__ __forceinline__ void insert_row(const double *__restrict__ src, double *__restrict__ dst, int m, int s,
                                           const double (&fresh)[3][3], int lane) {
  const int per_axis = 3 * m, old_axis = 3 * m - 3, cut = 3 * s;
  for (int e = lane; e < 3 * per_axis; e += 64) {
    const int k = (e >= per_axis) + (e >= 2 * per_axis), r = e - k * per_axis;
    double v;
    if (r < cut) {
      v = src[k * old_axis + r];
    } else if (r < cut + 3) {
      const int comp = r - cut;
      v = comp == 0 ? pick3(fresh[0], k) : (comp == 1 ? pick3(fresh[1], k) : pick3(fresh[2], k));
    } else {
      v = src[k * old_axis + r - 3];
    }
    dst[e] = v;
  }
}

__global__ void __launch_bounds__(64 * kInsertWaves)
insert_waypoints_kernel(const InsertArgs a, const GtopGrid g, const double *__restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kInsertWaves + (threadIdx.x >> 6)));
  if (b >= a.B) return;   // the whole wavefront
  const int m = a.m;
  const double *ts = a.T + (size_t)b * a.t_stride;

  // ---- the decision: segment s, local time tl ----
  double t = a.mode == GTOP_INSERT_AT_TIME ? a.when[(size_t)b * a.when_stride] : -1.0;
  const bool at_time = a.mode == GTOP_INSERT_AT_TIME && t >= 0.0 && t < INFINITY;
  const bool fell_back = a.mode == GTOP_INSERT_AT_TIME && !at_time;
  int s;
  double tl, Ts;
  if (at_time) {
    s = (int)segment_of(ts, m, t);
    tl = t;
    Ts = ts[s];
  } else {
    s = longest_segment(ts, m, lane);
    Ts = ts[s];
    tl = 0.5 * Ts;
  }
  const double lo = a.min_fraction * Ts, hi = Ts - lo;
  const double tc = fmin(fmax(tl, lo), hi);
  const bool clamped = tc != tl;
  tl = tc;

  // ---- the new junction ----
  const double *seg = a.coeff + ((size_t)b * m + s) * 18;
  double fresh[3][3];   // [p | v | a][axis]
  for (int k = 0; k < 3; ++k) {
    const double *c = seg + 6 * k;
    fresh[0][k] = poly_eval(c, tl);
    fresh[1][k] = horner_vel(c, tl);
    fresh[2][k] = horner_acc(c, tl);
  }
  double d_field = 0.0;
  bool pushed = false;
  if (a.push > 0.0) {   // (d, g) of gtop_edt_query_device at (p, -1): the static lookup of gtop_edt_lookup.h
    const double *p = fresh[0];
    const bool out = gtop_edt_out_of_map(g, p);
    int idx[3];
    double diff[3], values[2][2][2], grad[3];
    gtop_edt_corners(g, rec, p, idx, diff, values);   // (out of the map: clamped indices, memory-safe)
    const GtopTrilinear tri = gtop_edt_trilinear(diff, values);
    gtop_edt_gradient(g, diff, values, tri, grad);
    d_field = out ? -1.0 : tri.d;
    const double n = sqrt(grad[0] * grad[0] + grad[1] * grad[1] + grad[2] * grad[2]);
    pushed = !out && !(d_field >= a.push_below) && !(n == 0.0);
    if (pushed)
      for (int k = 0; k < 3; ++k) fresh[0][k] = fresh[0][k] + (a.push * grad[k]) / n;
  }

  // ---- the outputs: every entry once ----
  const size_t n_old = 9 * (size_t)(m - 1), n_new = 9 * (size_t)m;
  insert_row(a.x + b * n_old, a.x_out + b * n_new, m, s, fresh, lane);
  if (a.lb) {   // the new waypoint's bounds: gtop_default_bounds' rule around the final p
    const double below[3][3] = {{fresh[0][0] - a.bos, fresh[0][1] - a.bos, fresh[0][2] - a.bos},
                                {-a.vos, -a.vos, -a.vos},
                                {-a.aos, -a.aos, -a.aos}};
    const double above[3][3] = {{fresh[0][0] + a.bos, fresh[0][1] + a.bos, fresh[0][2] + a.bos},
                                {a.vos, a.vos, a.vos},
                                {a.aos, a.aos, a.aos}};
    insert_row(a.lb + b * n_old, a.lb_out + b * n_new, m, s, below, lane);
    insert_row(a.ub + b * n_old, a.ub_out + b * n_new, m, s, above, lane);
  }
  double *to = a.T_out + (size_t)b * (m + 1);
  for (int i = lane; i <= m; i += 64) to[i] = i < s ? ts[i] : (i == s ? tl : (i == s + 1 ? Ts - tl : ts[i - 1]));
  if (a.info && lane < GTOP_INSERT_INFO) {
    const double row[GTOP_INSERT_INFO] = {(double)s, tl, fell_back ? 1.0 : 0.0, clamped ? 1.0 : 0.0, d_field,
                                          pushed ? 1.0 : 0.0};
    double v = row[0];
    for (int i = 1; i < GTOP_INSERT_INFO; ++i) v = lane == i ? row[i] : v;
    a.info[(size_t)b * GTOP_INSERT_INFO + lane] = v;
  }
}

}  // namespace

hipError_t gtop_launch_insert_waypoints(const GtopGrid &g, const double *rec, int mode, double min_fraction, double push,
                                        double push_below, double bos, double vos, double aos, int B, int m,
                                        const double *x, const double *coeff, const double *T, int t_stride,
                                        const double *when, int when_stride, const double *lb, const double *ub,
                                        double *x_out, double *T_out, double *lb_out, double *ub_out, double *info,
                                        hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const InsertArgs a = {B, m, t_stride, when_stride, mode, x, coeff, T, when, lb, ub, x_out, T_out, lb_out, ub_out, info,
                        min_fraction, push, push_below, bos, vos, aos};
  hipLaunchKernelGGL(insert_waypoints_kernel, dim3((B + kInsertWaves - 1) / kInsertWaves), dim3(64 * kInsertWaves), 0,
                     stream, a, g, rec);
  return hipGetLastError();
}
