// gtop_time.hip — the derivative of the cost with respect to every segment time, and the optimizer of the time
// allocation built on it, on gfx950, fp64 (include/gtop_time.h).
//
// The pass over a trajectory and the optimizer's row loop are gtop_time_pass.h's, shared with the kernels under the
// moving-obstacle cost (gtop_time_moving.hip); here they are instantiated without it: one wavefront per trajectory,
// several per workgroup, no workgroup barrier, T, g, the trial T' and its g' of the optimizer in LDS (4 m doubles per
// wavefront).

#include "gtop_time_pass.h"

namespace {

__global__ void __launch_bounds__(64 * kTimeWaves)
time_gradient_kernel(const TimeParams P, int B, int m, const double *__restrict__ x, const double *__restrict__ Df,
                     const double *__restrict__ T, int t_stride, double *__restrict__ cost /*[B]*/,
                     double *__restrict__ gT /*[B][m]*/, double *__restrict__ parts /*[B][m][4] or NULL*/) {
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTimeWaves + (threadIdx.x >> 6)));
  if (b >= B) return;
  const size_t n = 9 * (size_t)(m - 1);
  TimeMoving none{};
  const double c = time_pass<false, false, GTOP_TIME_PARTS>(P, none, m, lane, x + (size_t)b * n, Df + (size_t)b * 18,
                                                            T + (size_t)b * t_stride, 0.0, gT + (size_t)b * m,
                                                            parts ? parts + (size_t)b * m * 4 : nullptr);
  if (lane == 0) cost[b] = c;
}

// LDS: per wavefront T | g | T' | g', m doubles each
__global__ void __launch_bounds__(64 * kTimeWaves)
time_optimize_kernel(const TimeParams P, const TimeOpt O, int B, int m, const double *__restrict__ x,
                     const double *__restrict__ Df, const double *__restrict__ T, int t_stride,
                     const double *__restrict__ T_lo /*[B][m] or NULL*/, double *__restrict__ T_out /*[B][m]*/,
                     double *__restrict__ info /*[B][8]*/) {
  extern __shared__ double time_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTimeWaves + wave));
  if (b >= B) return;
  const size_t n = 9 * (size_t)(m - 1);
  const double *xb = x + (size_t)b * n, *dfb = Df + (size_t)b * 18, *Tin = T + (size_t)b * t_stride;
  const double *lo_row = T_lo ? T_lo + (size_t)b * m : nullptr;
  TimeMoving none{};
  time_optimize_row<false, false>(P, none, O, b, m, lane, xb, dfb, Tin, lo_row, time_lds + (size_t)wave * 4 * m, T_out,
                                  info);
}

}  // namespace

hipError_t gtop_launch_time_gradient(const GtopGrid &g, const double *rec, const GtopTimeCost &p, int B, int m,
                                     const double *x, const double *Df, const double *T, int t_stride, double *cost,
                                     double *gT, double *parts, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(time_gradient_kernel, dim3((B + kTimeWaves - 1) / kTimeWaves), dim3(64 * kTimeWaves), 0, stream,
                     time_params(g, rec, p), B, m, x, Df, T, t_stride, cost, gT, parts);
  return hipGetLastError();
}

hipError_t gtop_launch_time_optimize(const GtopGrid &g, const double *rec, const GtopTimeCost &p, double rho,
                                     double t_min, double t_max, double first_move, double ftol_rel, double xtol_abs,
                                     int max_evals, int B, int m, const double *x, const double *Df, const double *T,
                                     int t_stride, const double *T_lo, double *T_out, double *info, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const TimeOpt O = {rho, t_min, t_max, first_move, ftol_rel, xtol_abs, max_evals};
  const size_t lds = (size_t)kTimeWaves * 4 * m * sizeof(double);   // 29 056 bytes at m = 227
  hipLaunchKernelGGL(time_optimize_kernel, dim3((B + kTimeWaves - 1) / kTimeWaves), dim3(64 * kTimeWaves), lds, stream,
                     time_params(g, rec, p), O, B, m, x, Df, T, t_stride, T_lo, T_out, info);
  return hipGetLastError();
}
