// gtop_minjerk.hip — the minimum-jerk start point on gfx950, batched (gtop_min_jerk_start_device of include/gtop.h).
//
// The reference's PolyQPGeneration(type == 1) (src/qp_generator.cpp:242-315 of EpicOne1/grad_traj_optimization) fixes
// the waypoint positions and solves Dp = -Rpp^-1 Rfp' Df with dense inverses.  Here R is never formed.  With the jerk
// integral of one quintic segment of duration T in the order [p(0), p(T), v(0), v(T), a(0), a(T)]
//
//   M(1) = [  720 -720  360  360   60  -60 ]      M(T)(i,j) = M(1)(i,j) / T^(5 - o_i - o_j),
//          [ -720  720 -360 -360  -60   60 ]      o = 0 for a position, 1 for a velocity, 2 for an acceleration
//          [  360 -360  192  168   36  -24 ]
//          [  360 -360  168  192   24  -36 ]
//          [   60  -60   36   24    9   -3 ]
//          [  -60   60  -24  -36   -3    9 ]
//
// the normal equations in u_k = (v_k, a_k), k = 1 .. m-1, are block tridiagonal, 2 x 2 blocks, symmetric positive
// definite, the same matrix for the three axes (Ta = T[k-1], Tb = T[k]):
//
//   D_k = [ 192/Ta^3 + 192/Tb^3    -36/Ta^2 + 36/Tb^2 ]      U_k = [ 168/Tb^3   -24/Tb^2 ]
//         [ -36/Ta^2 + 36/Tb^2       9/Ta   +  9/Tb   ]            [  24/Tb^2    -3/Tb   ]
//   D_k u_k + U_{k-1}' u_{k-1} + U_k u_{k+1} = -g_k
//   g_k(v) = 360 (p_{k-1} - p_k)/Ta^4 + 360 (p_k - p_{k+1})/Tb^4
//   g_k(a) = -60 (p_{k-1} - p_k)/Ta^3 +  60 (p_k - p_{k+1})/Tb^3
//
// u_0 and u_m are the boundary pairs of Df and move to the right-hand side.
//
// One LANE per trajectory, block elimination front to back, O(m):
//   forward   S_k = D_k - U_{k-1}' J_{k-1} U_{k-1},  J_k = S_k^-1,  y_k = J_k (-g_k - U_{k-1}' y_{k-1} [- U_k u_m, k = m-1])
//             with J_0 = 0 and y_0 = u_0, so that the first waypoint needs no statement of its own
//   backward  u_{m-1} = y_{m-1},  u_k = y_k - J_k U_k u_{k+1}
// The y_k of the three axes are exactly the six v, a slots x has per waypoint and live there between the sweeps; the
// three doubles of J_k wait in LDS, lane-interleaved (gtop_minjerk_plan.h: the lanes per workgroup fall as m grows).
// Positions are read, never written.  A lane's arithmetic depends on nothing but its own row, so equal rows get equal
// bits whatever their index, the batch or the sharing of T.  A zero segment time makes 1/T infinite and the row's v, a
// NaN; every loop is bounded by m.
// Setup-side and latency bound: rows of x lie n doubles apart, every lane walks its own cache lines (three streams of
// 24 bytes per waypoint), about 2 m dependent steps of some 60 fp64 operations and one division each.

#include <hip/hip_runtime.h>

#include "gtop_kernels.h"
#include "gtop_minjerk_plan.h"

namespace {

__global__ void __launch_bounds__(kMinJerkMaxLanes)
min_jerk_start_kernel(int B, int m, double *x, const double *__restrict__ Df, const double *__restrict__ T,
                      int t_stride) {
  extern __shared__ double jblk[];   // gtop_minjerk_slot(k, c, lane, lanes)
  const int lanes = blockDim.x, lane = threadIdx.x;
  const size_t b = (size_t)blockIdx.x * lanes + lane;
  if (b >= (size_t)B) return;
  const int ndp = 3 * m - 3;
  double *xb = x + b * (size_t)(3 * ndp);
  const double *df = Df + b * 18, *ts = T + b * (size_t)t_stride;

  double pprev[3], pcur[3], yv[3], ya[3];
  for (int a = 0; a < 3; ++a) {
    pprev[a] = df[6 * a];
    pcur[a] = xb[a * ndp];
    yv[a] = df[6 * a + 1];   // y_0 = u_0
    ya[a] = df[6 * a + 2];
  }
  double j11 = 0.0, j12 = 0.0, j22 = 0.0;   // J_0 = 0
  double ia1 = 1.0 / ts[0];
  double ia2 = ia1 * ia1, ia3 = ia2 * ia1, ia4 = ia2 * ia2;

  // ---- forward
  for (int k = 1; k < m; ++k) {
    const bool last = k == m - 1;
    const double ib1 = 1.0 / ts[k];
    const double ib2 = ib1 * ib1, ib3 = ib2 * ib1, ib4 = ib2 * ib2;
    // U_{k-1} (of Ta) and U_k (of Tb)
    const double a11 = 168.0 * ia3, a12 = -24.0 * ia2, a21 = 24.0 * ia2, a22 = -3.0 * ia1;
    const double b11 = 168.0 * ib3, b12 = -24.0 * ib2, b21 = 24.0 * ib2, b22 = -3.0 * ib1;
    // S_k = D_k - U_{k-1}' (J_{k-1} U_{k-1})
    const double w11 = j11 * a11 + j12 * a21, w12 = j11 * a12 + j12 * a22;
    const double w21 = j12 * a11 + j22 * a21, w22 = j12 * a12 + j22 * a22;
    const double s11 = (192.0 * ia3 + 192.0 * ib3) - (a11 * w11 + a21 * w21);
    const double s12 = (36.0 * ib2 - 36.0 * ia2) - (a11 * w12 + a21 * w22);
    const double s22 = (9.0 * ia1 + 9.0 * ib1) - (a12 * w12 + a22 * w22);
    const double idet = 1.0 / (s11 * s22 - s12 * s12);
    j11 = s22 * idet;
    j12 = -s12 * idet;
    j22 = s11 * idet;
    jblk[gtop_minjerk_slot(k, 0, lane, lanes)] = j11;
    jblk[gtop_minjerk_slot(k, 1, lane, lanes)] = j12;
    jblk[gtop_minjerk_slot(k, 2, lane, lanes)] = j22;
    for (int a = 0; a < 3; ++a) {
      const double pnext = last ? df[6 * a + 3] : xb[a * ndp + 3 * k];
      const double da = pprev[a] - pcur[a], db = pcur[a] - pnext;
      double rv = -(360.0 * da * ia4 + 360.0 * db * ib4) - (a11 * yv[a] + a21 * ya[a]);
      double ra = -(60.0 * db * ib3 - 60.0 * da * ia3) - (a12 * yv[a] + a22 * ya[a]);
      if (last) {
        const double vm = df[6 * a + 4], am = df[6 * a + 5];
        rv -= b11 * vm + b12 * am;
        ra -= b21 * vm + b22 * am;
      }
      yv[a] = j11 * rv + j12 * ra;
      ya[a] = j12 * rv + j22 * ra;
      xb[a * ndp + 3 * (k - 1) + 1] = yv[a];
      xb[a * ndp + 3 * (k - 1) + 2] = ya[a];
      pprev[a] = pcur[a];
      pcur[a] = pnext;
    }
    ia1 = ib1; ia2 = ib2; ia3 = ib3; ia4 = ib4;
  }

  // ---- backward: (yv, ya) hold u_{k+1}
  for (int k = m - 2; k >= 1; --k) {
    const double ib1 = 1.0 / ts[k];
    const double ib2 = ib1 * ib1, ib3 = ib2 * ib1;
    const double b11 = 168.0 * ib3, b12 = -24.0 * ib2, b21 = 24.0 * ib2, b22 = -3.0 * ib1;
    const double k11 = jblk[gtop_minjerk_slot(k, 0, lane, lanes)];
    const double k12 = jblk[gtop_minjerk_slot(k, 1, lane, lanes)];
    const double k22 = jblk[gtop_minjerk_slot(k, 2, lane, lanes)];
    for (int a = 0; a < 3; ++a) {
      const double tv = b11 * yv[a] + b12 * ya[a], ta = b21 * yv[a] + b22 * ya[a];
      yv[a] = xb[a * ndp + 3 * (k - 1) + 1] - (k11 * tv + k12 * ta);
      ya[a] = xb[a * ndp + 3 * (k - 1) + 2] - (k12 * tv + k22 * ta);
      xb[a * ndp + 3 * (k - 1) + 1] = yv[a];
      xb[a * ndp + 3 * (k - 1) + 2] = ya[a];
    }
  }
}

}  // namespace

hipError_t gtop_launch_min_jerk_start(int B, int m, double *x, const double *Df, const double *T, int t_stride,
                                      hipStream_t stream) {
  GtopMinJerkPlan plan;
  if (!gtop_minjerk_plan(B, m, &plan)) return hipErrorInvalidValue;
  if (plan.blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(min_jerk_start_kernel, dim3(plan.blocks), dim3(plan.lanes), plan.lds_bytes, stream, B, m, x, Df, T,
                     t_stride);
  return hipGetLastError();
}
