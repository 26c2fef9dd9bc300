// gtop_report_common.h — the sample loop of the kernels that walk a trajectory's getTraj samples one wavefront at a time,
// lanes over the samples 64 at a time: the trajectory report (traj_report_kernel, gtop_validate.hip), the per-segment
// report (traj_segments_kernel, gtop_segments.hip) and the post-processing (eval_trajectories_kernel, gtop_setup.hip).
// What such a kernel does per sample is stated HERE, once: (a) the chunk's accumulated sample times, (b) the segment
// walk, (c) position, velocity and acceleration, (d) the distance to the static field and the moving boxes — so count,
// times, positions, velocities, accelerations and distances are the same bits in every one of them (the library is
// built with -ffp-contract=on: the same source expression rounds the same way wherever it is inlined).  A kernel keeps
// what it does with a sample: its reductions, its stores.
#ifndef GTOP_REPORT_COMMON_H_
#define GTOP_REPORT_COMMON_H_

#include <hip/hip_runtime.h>

#include "gtop_device_common.h"   // poly_eval
#include "gtop_edt_lookup.h"

constexpr int kValBoxChunk = 64;   // boxes staged in LDS per pass (4.5 KiB: 32 one-wavefront workgroups fit a CU)
// A polynomial list: 32 rows of 24 per pass, the most the cost term takes: 6 KiB — 26 one-wavefront workgroups of LDS
// per CU, where the kernel's 120 VGPRs admit 16.
constexpr int kValBoxChunkPoly = 32;
template <bool POLY> constexpr int kValBoxChunkOf = POLY ? kValBoxChunkPoly : kValBoxChunk;

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

// ---- (a) the sample times ----
// getTraj (polynomial_traj.hpp:69-78) accumulates the sample time (eval_t += dt_sample) and tests eval_t <= time_sum, so
// the time of sample k is that sum, not k * dt_sample.  A wavefront's loop carries base_t, the time of its chunk's
// sample 0, and runs `while (base_t <= time_sum)`.
// The time of sample `skip` by the same additions, one after the other: base_t of a wavefront's first chunk (0 for the
// only wavefront of a trajectory).
__device__ __forceinline__ double sample_time_of(int skip, double dt_sample) {
  double base_t = 0.0;
  for (int i = 0; i < skip; ++i) base_t += dt_sample;
  return base_t;
}
// One chunk: eval_t, the accumulated time of the lane's sample; live, whether that sample exists (monotone in the lane
// index); next_base, base_t of this wavefront's next chunk, `stride` samples on (64 times the wavefronts that share the
// trajectory).
struct ChunkTimes {
  double eval_t, next_base;
  bool live;
};
__device__ __forceinline__ ChunkTimes chunk_times(double base_t, double dt_sample, int lane, int stride, double time_sum) {
  ChunkTimes c;
  c.eval_t = base_t;
  for (int i = 0; i < lane; ++i) c.eval_t += dt_sample;
  c.next_base = base_t;
  for (int i = 0; i < stride; ++i) c.next_base += dt_sample;
  c.live = c.eval_t <= time_sum;
  return c;
}

// ---- (b) the segment walk ----
// polynomial_traj.hpp:48-51: the segment trajectory time t falls into; t becomes the time inside it.  The reference
// walks off the end when t == time_sum exactly; here the last segment is extended instead.
// (unsigned, and to be kept so where it indexes the coefficients: through the inlined call the compiler no longer sees
// that the index is non-negative, and a signed one costs a sign extension in the address and a different schedule —
// 8 % of eval_trajectories_kernel's time at 1 024 trajectories.)
__device__ __forceinline__ unsigned segment_of(const double *ts, int m, double &t) {
  unsigned idx = 0;
  while ((int)idx < m - 1 && ts[idx] <= t) {
    t -= ts[idx];
    ++idx;
  }
  return idx;
}

// ---- (c) position, velocity, acceleration ----
// of the sample at time t of the segment with the coefficient row seg = [cx0..5 | cy0..5 | cz0..5], and the running
// maxima they enter: per axis (vax, aax) and of the squared norms (vmax2, amax2: sqrt is monotone, taken by the caller
// once at the end).
__device__ __forceinline__ void sample_motion(const double *seg, double t, double p[3], double &vax, double &aax,
                                              double &vmax2, double &amax2) {
  double v[3], a[3];
  for (int k = 0; k < 3; ++k) {
    const double *c = seg + 6 * k;
    p[k] = poly_eval(c, t);
    v[k] = poly_vel(c, t);
    a[k] = poly_acc(c, t);
    vax = fmax(vax, fabs(v[k]));
    aax = fmax(aax, fabs(a[k]));
  }
  vmax2 = fmax(vmax2, v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  amax2 = fmax(amax2, a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
}

// ---- (d) the distance ----
// evaluateEDTWithGrad(pos, tau)'s value at the lane's sample, as edt_query_kernel<false, POLY> forms it:
// tau = start + eval_t with boxes and -1 (static only) without; d = -1 out of the map.  bx holds the list's first
// kValBoxChunkOf<POLY> boxes, staged by the caller before its loop.  A longer list is restaged chunk by chunk HERE
// (RESTAGE), inside the sample loop, which only a one-wavefront workgroup can do: stage_boxes' barriers then sit in a
// loop that a workgroup's wavefronts leave at different times.  Wave-uniform control flow around the call.
// (A dead lane looks p = 0 up: clamped indices, memory-safe.)
struct SampleDistance {
  double d;
  bool out;
};
template <bool POLY, bool RESTAGE>
__device__ __forceinline__ SampleDistance sample_distance(const GtopGrid &g, const double *__restrict__ rec,
                                                          double (*bx)[kBoxRowOf<POLY>], int nbox,
                                                          const double *__restrict__ box_p0,
                                                          const double *__restrict__ box_vel,
                                                          const double *__restrict__ box_scale, bool use_boxes,
                                                          double start, double eval_t, bool live, const double p[3],
                                                          int lane) {
  constexpr int kChunk = kValBoxChunkOf<POLY>;
  const double tau = use_boxes ? start + eval_t : -1.0;
  const bool out = gtop_edt_out_of_map(g, p);
  const bool dyn = live & !out & (tau >= 0.0);
  int idx[3];
  double diff[3], values[2][2][2];
  gtop_edt_corners(g, rec, p, idx, diff, values);
  double vmax = gtop_edt_vmax(values);
  for (int b0 = 0; b0 < nbox; b0 += kChunk) {
    const int nb = min(kChunk, nbox - b0);
    if constexpr (RESTAGE)
      if (nbox > kChunk) stage_boxes<POLY>(bx, box_p0, box_vel, box_scale, b0, nb, lane, 64);   // wave-uniform
    if (dyn) {
      for (int q = 0; q < nb; ++q) {
        double bmin[3], bmax[3];
        gtop_edt_box_faces_of<POLY>(bx[q], tau, bmin, bmax);
        gtop_edt_box_min(g, bmin, bmax, idx, values, vmax);
      }
    }
  }
  return {out ? -1.0 : gtop_edt_trilinear(diff, values).d, out};
}

#endif  // GTOP_REPORT_COMMON_H_
