// gtop_retime.hip — segment-time reallocation on gfx950, batched (gtop_reallocate_times_device of include/gtop.h).
//
// The reference carries the remedy as a commented block behind the solve (src/grad_traj_optimizer.cpp:209-227 of
// EpicOne1/grad_traj_optimization, "reallocate segment time"): the times of the straight-line path are replaced by
// length / mean_v of the waypoints as the optimizer left them.  That is mode LENGTH.  Mode LIMITS is what a batched
// planner needs beside it: the segments whose velocity or acceleration figure in the per-segment report
// (gtop_segments.hip) breaks a limit are stretched by the ratio that would bring a time-scaled curve back inside.
//
// One LANE per trajectory, O(m), setup-side and latency bound.  Every step is ONE rounded IEEE operation — the file is
// compiled unfused — so a numpy twin reproduces the bits (tests/segments_twin.py).  A lane reads a time before it writes
// it, and touches its own row alone: T_out may be T itself when the times are per trajectory.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_kernels.h"

#pragma clang fp contract(off)

namespace {

// LENGTH: waypoint 0 is Df[k][0], waypoint m is Df[k][3], interior waypoint j is x[3 (j - 1) + k (3m - 3)]; `len` is the
// one expression of setup_paths_kernel (gtop_setup.hip), the first AND the last segment take init_time (:226).
__global__ void __launch_bounds__(64)
retime_length_kernel(int B, int m, const double *__restrict__ x, const double *__restrict__ Df, double mean_v,
                     double init_time, double *__restrict__ T_out) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (size_t)B) return;
  const int ndp = 3 * m - 3;
  const double *xb = x + b * (size_t)(3 * ndp), *df = Df + b * 18;
  double *to = T_out + b * (size_t)m;
  double p[3] = {df[0], df[6], df[12]};
  for (int i = 0; i < m; ++i) {
    double q[3];
    for (int k = 0; k < 3; ++k) q[k] = i == m - 1 ? df[6 * k + 3] : xb[k * ndp + 3 * i];
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    to[i] = (i == 0 || i == m - 1) ? len / mean_v + init_time : len / mean_v;
    for (int k = 0; k < 3; ++k) p[k] = q[k];
  }
}

struct RetimeLimits {
  double max_vel, max_acc, max_ratio;
  int per_axis, uniform, scale_x;
};

__device__ __forceinline__ double retime_ratio(const double *__restrict__ row, const RetimeLimits &o) {
  const double V = row[o.per_axis ? 8 : 6], A = row[o.per_axis ? 9 : 7];
  const double rv = o.max_vel > 0.0 ? V / o.max_vel : 0.0;
  const double ra = o.max_acc > 0.0 ? sqrt(A / o.max_acc) : 0.0;
  return fmin(fmax(fmax(rv, ra), 1.0), o.max_ratio);
}

// LIMITS.  x may be NULL unless scale_x.  T_out == T is served for t_stride == m: T[s] is read before T_out[s] is
// written, by the lane that owns the row.
__global__ void __launch_bounds__(64)
retime_limits_kernel(int B, int m, double *x, const double *T, int t_stride, const double *__restrict__ seg_report,
                     RetimeLimits o, double *T_out) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (size_t)B) return;
  const int ndp = 3 * m - 3;
  const double *ts = T + b * (size_t)t_stride, *rows = seg_report + b * (size_t)m * GTOP_SEG_REPORT;
  double *to = T_out + b * (size_t)m;
  double lam = 1.0;
  if (o.uniform)
    for (int s = 0; s < m; ++s) lam = fmax(lam, retime_ratio(rows + (size_t)s * GTOP_SEG_REPORT, o));
  double prev = 1.0;
  for (int s = 0; s < m; ++s) {
    const double ratio = o.uniform ? lam : retime_ratio(rows + (size_t)s * GTOP_SEG_REPORT, o);
    const double t = ts[s];
    to[s] = ratio * t;
    if (o.scale_x && s >= 1) {                      // junction k = s between segments s - 1 and s
      const double rho = fmax(prev, ratio), rho2 = rho * rho;
      double *xk = x + b * (size_t)(3 * ndp) + 3 * (s - 1);
      for (int k = 0; k < 3; ++k) {
        xk[k * ndp + 1] = xk[k * ndp + 1] / rho;
        xk[k * ndp + 2] = xk[k * ndp + 2] / rho2;
      }
    }
    prev = ratio;
  }
}

}  // namespace

hipError_t gtop_launch_retime_length(int B, int m, const double *x, const double *Df, double mean_v, double init_time,
                                     double *T_out, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(retime_length_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, B, m, x, Df, mean_v, init_time, T_out);
  return hipGetLastError();
}

hipError_t gtop_launch_retime_limits(int B, int m, double *x, const double *T, int t_stride, const double *seg_report,
                                     double max_vel, double max_acc, double max_ratio, int per_axis, int uniform,
                                     int scale_x, double *T_out, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const RetimeLimits o = {max_vel, max_acc, max_ratio, per_axis, uniform, scale_x};
  hipLaunchKernelGGL(retime_limits_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, B, m, x, T, t_stride, seg_report, o,
                     T_out);
  return hipGetLastError();
}
