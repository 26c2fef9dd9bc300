// gtop_report_common.h — the device helpers the trajectory report (gtop_validate.hip) and the per-segment report
// (gtop_segments.hip) share: the polynomial's derivatives, the wavefront maximum and the staging of the box list in
// LDS.  One statement of each, so that the two kernels form the same velocity, acceleration and distance bit for bit
// (the library is built with -ffp-contract=on: the same source expression rounds the same way wherever it is inlined).
#ifndef GTOP_REPORT_COMMON_H_
#define GTOP_REPORT_COMMON_H_

#include <hip/hip_runtime.h>

constexpr int kValBoxChunk = 64;   // boxes staged in LDS per pass (4.5 KiB: 32 one-wavefront workgroups fit a CU)
// The polynomial list's object: 32 rows of 24 per pass, the most the cost term takes: 6 KiB — 26 one-wavefront
// workgroups of LDS per CU, where the kernel's 120 VGPRs admit 16.
constexpr int kValBoxChunkPoly = 32;

// first and second derivative of sum_j c[j] t^j.  Evaluation order (the quantity is fixed by the interface, the order
// is this kernel's): the terms from the highest power down, as poly_eval sums the value, each term (j c_j) * t^(j-1)
// resp. (j (j-1) c_j) * t^(j-2) with the integer factor applied to the coefficient first (exact for 2 and 4, one
// rounding otherwise) and the powers by multiplication; a*b + s contracts to an fma where written as one expression.
__device__ __forceinline__ double poly_vel(const double *c, double t) {
  const double t2 = t * t, t3 = t2 * t, t4 = t2 * t2;
  double s = (5.0 * c[5]) * t4;
  s = (4.0 * c[4]) * t3 + s;
  s = (3.0 * c[3]) * t2 + s;
  s = (2.0 * c[2]) * t + s;
  s = c[1] + s;
  return s;
}
__device__ __forceinline__ double poly_acc(const double *c, double t) {
  const double t2 = t * t, t3 = t2 * t;
  double s = (20.0 * c[5]) * t3;
  s = (12.0 * c[4]) * t2 + s;
  s = (6.0 * c[3]) * t + s;
  s = 2.0 * c[2] + s;
  return s;
}

__device__ __forceinline__ double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// boxes b0 .. b0 + nb - 1 into LDS as rows of p0, vel, scale, by the whole workgroup.  (With one wavefront per workgroup
// the barriers order that wavefront's own LDS reads and writes and nothing else.)
// POLY: box_p0 is the list's [nbox][kBoxRowPoly] rows, copied as they are.
template <bool POLY, int ROW>
__device__ __forceinline__ void stage_boxes(double (*bx)[ROW], const double *__restrict__ box_p0,
                                            const double *__restrict__ box_vel, const double *__restrict__ box_scale,
                                            int b0, int nb, int tid, int nthreads) {
  __syncthreads();
  if constexpr (POLY) {
    for (int q = tid; q < nb * ROW; q += nthreads) (&bx[0][0])[q] = box_p0[(size_t)b0 * ROW + q];
  } else {
    for (int q = tid; q < nb * 9; q += nthreads) {
      const int bb = q / 9, f = q - 9 * bb, k = f % 3;
      const size_t e = 3 * (size_t)(b0 + bb) + k;
      bx[bb][f] = f < 3 ? box_p0[e] : (f < 6 ? box_vel[e] : box_scale[e]);
    }
  }
  __syncthreads();
}

#endif  // GTOP_REPORT_COMMON_H_
