// gtop_time_moving.hip — the derivative of the cost with respect to every segment time, and the optimizer of the time
// allocation, under the moving-obstacle cost, on gfx950, fp64 (include/gtop_time_moving.h).
//
// The pass and the optimizer's row loop are gtop_time_pass.h's with MOV: one wavefront per trajectory, four per
// workgroup.  The workgroup stages the box list once in LDS (stage_boxes<POLY>, at most 32 rows of 24 doubles) — before
// any wavefront of a partial last workgroup leaves, since the staging holds the workgroup's barriers.  Per wavefront the
// gradient kernel keeps the segments' own derivatives and q_s in LDS (2 m doubles) until the sum over the later
// segments is known, so that every output entry is written exactly once; the optimizer keeps T, g, T', g' and q (5 m
// doubles: 36 320 bytes per workgroup at m = 227, 42 464 with the boxes).

#include "gtop_time_pass.h"

namespace {

// the box list as stage_boxes takes it (GtopBoxList's pointers), and the rows' start times on the boxes' clock
struct TimeBoxes {
  const double *p0, *vel, *scale;   // polynomial list: p0 = the rows, the other two NULL
  int nbox;                          // 1 .. GTOP_MOVING_MAX_BOXES under MOV
  const double *t0;                  // NULL: every start 0
  int t0_stride;                     // 0: one shared value
};

// parts [B][m][GTOP_TIME_MOVING_PARTS] or NULL, gt0 [B] or NULL.  Without MOV (the cost term off, or no boxes): the
// static pass, [4] = [5] = gt0 = 0.
template <bool MOV, bool POLY>
__global__ void __launch_bounds__(64 * kTimeWaves)
time_moving_gradient_kernel(const TimeParams P, const TimeBoxes K, int B, int m, const double *__restrict__ x,
                            const double *__restrict__ Df, const double *__restrict__ T, int t_stride,
                            double *__restrict__ cost, double *__restrict__ gT, double *__restrict__ gt0,
                            double *__restrict__ parts) {
  extern __shared__ double time_lds[];
  __shared__ double bx[MOV ? GTOP_MOVING_MAX_BOXES : 1][kBoxRowOf<POLY>];
  if constexpr (MOV) stage_boxes<POLY>(bx, K.p0, K.vel, K.scale, 0, K.nbox, (int)threadIdx.x, 64 * kTimeWaves);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTimeWaves + wave));
  if (b >= B) return;
  const size_t n = 9 * (size_t)(m - 1);
  const double *xb = x + (size_t)b * n, *dfb = Df + (size_t)b * 18, *Tb = T + (size_t)b * t_stride;
  double *pb = parts ? parts + (size_t)b * m * GTOP_TIME_MOVING_PARTS : nullptr;
  TimeMoving M{};
  double c;
  if constexpr (MOV) {
    double *g = time_lds + (size_t)wave * 2 * m;
    M.bx = &bx[0][0];
    M.nbox = K.nbox;
    M.tau0 = K.t0 ? K.t0[(size_t)b * K.t0_stride] : 0.0;
    M.q = g + m;
    c = time_pass<true, POLY, GTOP_TIME_MOVING_PARTS>(P, M, m, lane, xb, dfb, Tb, 0.0, g, pb);
    time_wave_sync();
    for (int s = lane; s < m; s += 64) gT[(size_t)b * m + s] = g[s];
  } else {
    c = time_pass<false, false, GTOP_TIME_MOVING_PARTS>(P, M, m, lane, xb, dfb, Tb, 0.0, gT + (size_t)b * m, pb);
  }
  if (lane == 0) {
    cost[b] = c;
    if (gt0) gt0[b] = M.gt0;
  }
}

// LDS: per wavefront T | g | T' | g' | q, m doubles each
template <bool POLY>
__global__ void __launch_bounds__(64 * kTimeWaves)
time_moving_optimize_kernel(const TimeParams P, const TimeBoxes K, const TimeOpt O, int B, int m,
                            const double *__restrict__ x, const double *__restrict__ Df, const double *__restrict__ T,
                            int t_stride, const double *__restrict__ T_lo, double *__restrict__ T_out,
                            double *__restrict__ info) {
  extern __shared__ double time_lds[];
  __shared__ double bx[GTOP_MOVING_MAX_BOXES][kBoxRowOf<POLY>];
  stage_boxes<POLY>(bx, K.p0, K.vel, K.scale, 0, K.nbox, (int)threadIdx.x, 64 * kTimeWaves);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTimeWaves + wave));
  if (b >= B) return;
  const size_t n = 9 * (size_t)(m - 1);
  const double *xb = x + (size_t)b * n, *dfb = Df + (size_t)b * 18, *Tin = T + (size_t)b * t_stride;
  const double *lo_row = T_lo ? T_lo + (size_t)b * m : nullptr;
  double *lds = time_lds + (size_t)wave * 5 * m;
  TimeMoving M{};
  M.bx = &bx[0][0];
  M.nbox = K.nbox;
  M.tau0 = K.t0 ? K.t0[(size_t)b * K.t0_stride] : 0.0;
  M.q = lds + 4 * m;
  time_optimize_row<true, POLY>(P, M, O, b, m, lane, xb, dfb, Tin, lo_row, lds, T_out, info);
}

TimeBoxes time_boxes(const GtopBoxList &boxes, const double *t0, int t0_stride) {
  const bool poly = boxes.kind == GTOP_BOX_LIST_POLYNOMIAL;
  return {poly ? boxes.rows : boxes.p0, poly ? nullptr : boxes.vel, poly ? nullptr : boxes.scale, boxes.count, t0,
          t0_stride};
}

}  // namespace

hipError_t gtop_launch_time_gradient_moving(const GtopGrid &g, const double *rec, const GtopTimeCost &p,
                                            const GtopBoxList &boxes, const double *t0, int t0_stride, int B, int m,
                                            const double *x, const double *Df, const double *T, int t_stride,
                                            double *cost, double *gT, double *gt0, double *parts, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  if (boxes.count < 0 || boxes.count > GTOP_MOVING_MAX_BOXES) return hipErrorInvalidValue;   // (the staging's rows)
  const dim3 grid((B + kTimeWaves - 1) / kTimeWaves), block(64 * kTimeWaves);
  const TimeParams P = time_params(g, rec, p);
  const TimeBoxes K = time_boxes(boxes, t0, t0_stride);
  const size_t lds = (size_t)kTimeWaves * 2 * m * sizeof(double);   // 14 528 bytes at m = 227
  if (boxes.count == 0)
    hipLaunchKernelGGL((time_moving_gradient_kernel<false, false>), grid, block, 0, stream, P, K, B, m, x, Df, T,
                       t_stride, cost, gT, gt0, parts);
  else if (boxes.kind == GTOP_BOX_LIST_POLYNOMIAL)
    hipLaunchKernelGGL((time_moving_gradient_kernel<true, true>), grid, block, lds, stream, P, K, B, m, x, Df, T,
                       t_stride, cost, gT, gt0, parts);
  else
    hipLaunchKernelGGL((time_moving_gradient_kernel<true, false>), grid, block, lds, stream, P, K, B, m, x, Df, T,
                       t_stride, cost, gT, gt0, parts);
  return hipGetLastError();
}

hipError_t gtop_launch_time_optimize_moving(const GtopGrid &g, const double *rec, const GtopTimeCost &p,
                                            const GtopBoxList &boxes, const double *t0, int t0_stride, double rho,
                                            double t_min, double t_max, double first_move, double ftol_rel,
                                            double xtol_abs, int max_evals, int B, int m, const double *x,
                                            const double *Df, const double *T, int t_stride, const double *T_lo,
                                            double *T_out, double *info, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  if (boxes.count < 1 || boxes.count > GTOP_MOVING_MAX_BOXES) return hipErrorInvalidValue;   // (the staging's rows)
  const dim3 grid((B + kTimeWaves - 1) / kTimeWaves), block(64 * kTimeWaves);
  const TimeParams P = time_params(g, rec, p);
  const TimeBoxes K = time_boxes(boxes, t0, t0_stride);
  const TimeOpt O = {rho, t_min, t_max, first_move, ftol_rel, xtol_abs, max_evals};
  const size_t lds = (size_t)kTimeWaves * 5 * m * sizeof(double);   // 36 320 bytes at m = 227
  if (boxes.kind == GTOP_BOX_LIST_POLYNOMIAL)
    hipLaunchKernelGGL(time_moving_optimize_kernel<true>, grid, block, lds, stream, P, K, O, B, m, x, Df, T, t_stride,
                       T_lo, T_out, info);
  else
    hipLaunchKernelGGL(time_moving_optimize_kernel<false>, grid, block, lds, stream, P, K, O, B, m, x, Df, T, t_stride,
                       T_lo, T_out, info);
  return hipGetLastError();
}
