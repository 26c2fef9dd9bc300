// gtop_joint.hip — the cost with its derivatives with respect to the free waypoint values x AND the segment times T
// from one pass, and what the joint optimizer launches around the batched MMA update, on gfx950, fp64
// (include/gtop_joint.h).
//
// The pass is gtop_time_pass.h's with its GX switch on: the lookups, the cost, gT and parts are the time pass's own
// expressions (the same bits as gtop_time.hip's kernel), and the 18 sums per segment that d cost / d x needs ride on the
// same samples.  One wavefront per trajectory, kTimeWaves per workgroup, no LDS, no workgroup barrier.  Every row
// pointer has a stride of its own: the public gradient runs on separate buffers, the optimizer on its packed state.

#include "gtop_time_pass.h"

namespace {

// sum_s T_s in a fixed order: lane l takes s = l, l + 64, ... in order, then the wavefront's butterfly
__device__ __forceinline__ double joint_time_sum(const double *T, int m, int lane) {
  double v = 0.0;
  for (int s = lane; s < m; s += 64) v += T[s];
  return gtop_wave_sum(v);
}

__global__ void __launch_bounds__(64 * kTimeWaves)
joint_pass_kernel(const TimeParams P, int B, int m, const GtopJointRows R, const double *__restrict__ Df, int with_rho,
                  double rho, double *__restrict__ parts /*[B][m][4] or NULL*/) {
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTimeWaves + (threadIdx.x >> 6)));
  if (b >= B) return;
  const double *T = R.T + (size_t)b * R.t_stride;
  TimeMoving none{};
  const double c = time_pass<false, false, GTOP_TIME_PARTS, true>(
      P, none, m, lane, R.x + (size_t)b * R.x_stride, Df + (size_t)b * 18, T, with_rho ? rho : 0.0,
      R.gT + (size_t)b * R.gt_stride, parts ? parts + (size_t)b * m * GTOP_TIME_PARTS : nullptr,
      R.gx + (size_t)b * R.gx_stride);
  double f = c;
  if (with_rho) f = c + rho * joint_time_sum(T, m, lane);
  if (lane == 0) {
    R.f[(size_t)b * R.f_stride] = f;
    if (R.aux) R.aux[(size_t)b * R.aux_stride] = R.aux_plain ? c : f;
  }
}

__global__ void __launch_bounds__(256)
joint_pack_kernel(int B, int m, const double *__restrict__ x, const double *__restrict__ T, int t_stride,
                  const double *__restrict__ lb, const double *__restrict__ ub, const double *__restrict__ T_lo,
                  double t_min, double t_max, double *__restrict__ z0, double *__restrict__ zlb,
                  double *__restrict__ zub) {
  const size_t n = 9 * (size_t)(m - 1), nz = n + m, total = (size_t)B * nz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / nz, j = i - b * nz;
    if (j < n) {
      z0[i] = x[b * n + j];
      zlb[i] = lb[b * n + j];
      zub[i] = ub[b * n + j];
    } else {
      const size_t s = j - n;
      const double lo = T_lo ? fmax(t_min, T_lo[b * m + s]) : t_min;
      z0[i] = T[b * t_stride + s];
      zlb[i] = lo;
      zub[i] = lo > t_max ? lo : t_max;
    }
  }
}

// one wavefront per row
__global__ void __launch_bounds__(64)
joint_report_kernel(int B, int m, const double *__restrict__ z, const double *__restrict__ g,
                    const double *__restrict__ zlb, const double *__restrict__ zub, const double *__restrict__ minf,
                    const int *__restrict__ code, const int *__restrict__ nevals, double *__restrict__ x_out,
                    double *__restrict__ T_out, double *__restrict__ info) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const size_t n = 9 * (size_t)(m - 1), nz = n + m, o = (size_t)b * nz;
  double gfree_x = 0.0, gfree_T = 0.0, tsum = 0.0;
  for (size_t j = lane; j < nz; j += 64) {
    const double v = z[o + j], d = g[o + j], lo = zlb[o + j], hi = zub[o + j];
    const bool held = lo >= hi || (v <= lo && d > 0.0) || (v >= hi && d < 0.0);
    const bool is_T = j >= n;
    const double a = held ? 0.0 : fabs(d);
    gfree_x = is_T ? gfree_x : fmax(gfree_x, a);
    gfree_T = is_T ? fmax(gfree_T, a) : gfree_T;
    if (is_T) {
      T_out[(size_t)b * m + (j - n)] = v;
    } else {
      x_out[(size_t)b * n + j] = v;
    }
  }
  for (int s = lane; s < m; s += 64) tsum += z[o + n + s];
  tsum = gtop_wave_sum(tsum);
  gfree_x = time_wave_max(gfree_x);
  gfree_T = time_wave_max(gfree_T);
  if (lane == 0) {
    double *r = info + (size_t)b * GTOP_JOINT_INFO;
    r[0] = (double)code[b]; r[1] = (double)nevals[b]; r[3] = minf[b];
    r[5] = tsum; r[6] = gfree_x; r[7] = gfree_T;
  }
}

}  // namespace

hipError_t gtop_launch_joint_pass(const GtopGrid &g, const double *rec, const GtopTimeCost &p, int B, int m,
                                  const GtopJointRows &rows, const double *Df, int with_rho, double rho, double *parts,
                                  hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(joint_pass_kernel, dim3((B + kTimeWaves - 1) / kTimeWaves), dim3(64 * kTimeWaves), 0, stream,
                     time_params(g, rec, p), B, m, rows, Df, with_rho, rho, parts);
  return hipGetLastError();
}

hipError_t gtop_launch_joint_pack(int B, int m, const double *x, const double *T, int t_stride, const double *lb,
                                  const double *ub, const double *T_lo, double t_min, double t_max, double *z0,
                                  double *zlb, double *zub, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const size_t total = (size_t)B * (10 * (size_t)m - 9);
  const unsigned blocks = (unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(joint_pack_kernel, dim3(blocks), dim3(256), 0, stream, B, m, x, T, t_stride, lb, ub, T_lo, t_min,
                     t_max, z0, zlb, zub);
  return hipGetLastError();
}

hipError_t gtop_launch_joint_report(int B, int m, const double *z, const double *g, const double *zlb, const double *zub,
                                    const double *minf, const int *code, const int *nevals, double *x_out, double *T_out,
                                    double *info, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(joint_report_kernel, dim3(B), dim3(64), 0, stream, B, m, z, g, zlb, zub, minf, code, nevals, x_out,
                     T_out, info);
  return hipGetLastError();
}
