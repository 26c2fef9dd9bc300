// gtop_edt_lookup.h — the interpolating lookup of EDTEnvironment::evaluateEDTWithGrad
// (src/edt_environment.cpp:76-122 of EpicOne1/grad_traj_optimization) as device
// functions, shared by the batched query (gtop_edt.hip) and the trajectory reports
// (gtop_validate.hip and gtop_segments.hip, through gtop_report_common.h): the in-map
// test, base index / diff / the 8 corner values from the corner records, the staging
// of a box list in LDS, the min over one box with the exact skip, and the
// trilinear value.  The library is built with -ffp-contract=on, so the same source
// expression rounds the same way wherever it is inlined: all of them get the same
// distance, bit for bit.  The gradient (gtop_edt_gradient) is the query kernel's and the waypoint insertion's
// (gtop_insert.hip).
// The centre of a POLYNOMIAL box (gtop_set_moving_box_polynomials) is stated here once for those two kernels and for
// the cost bodies (mov_min_boxes, gtop_wave_kernel.h).
// The derivative of the box-lowered corner values with respect to the boxes' time (gtop_edt_box_velocity_of,
// gtop_edt_box_min_dtau; include/gtop_time_moving.h) is stated here once too, for the segment-time pass of
// gtop_time_pass.h.
// The STATIC lookup (base index, diff, trilinear value; the gradient in gtop_edt.hip) is unfused, as poly_eval is:
// it is sdf_map.cpp's arithmetic operation for operation, so a static query returns the bits of the reference's
// getDistWithGradTrilinear.  Fused, a gradient component that cancels between corners of very different size (free
// voxels at 10000 beside an obstacle's: v1 - v0 = 0.03 at |v| = 5750) left the reference by 3e-11 of itself, past
// the 1e-12 the query is held to (tests/test_gpu_records.py, the window without new points).
#ifndef GTOP_EDT_LOOKUP_H_
#define GTOP_EDT_LOOKUP_H_

#include <hip/hip_runtime.h>

#include "gtop_kernels.h"

// isInMap, sdf_map.cpp:55-69
__device__ __forceinline__ bool gtop_edt_out_of_map(const GtopGrid &g, const double p[3]) {
  bool out = false;
  for (int k = 0; k < 3; ++k) out |= (p[k] < g.min_range[k] + 1e-4) | (p[k] > g.max_range[k] - 1e-4);
  return out;
}

// The 8 corner values of the cell of base index idx[]: the loads of sdf_map.cpp:211-219, each index clamped per axis
// (getDistance(int,int,int), :166-174), from the CORNER RECORDS (gtop_records.hip): the two consecutive records of
// levels iz and iz + 1 hold all eight, clamps applied — 64 contiguous bytes, four 16-byte loads at one address (round 3
// read four (z, z+1) pairs from four lines: 4.24 lines of 128 bytes per query, 16 bytes used of each; now 1.25).
// Called by gtop_edt_corners, and by a caller that has the index and no point (the certificate of gtop_certify.hip,
// which visits the cells a box touches).
__device__ __forceinline__ void gtop_edt_cell_values(const GtopGrid &g, const double *__restrict__ rec, const int idx[3],
                                                     double values[2][2][2]) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const int cx = min(max(idx[0], -1), g.nx - 1) + 1, cy = min(max(idx[1], -1), g.ny - 1) + 1;
  const int cz = min(max(idx[2], -1), g.nz - 1) + 1;
  const d2 *r = reinterpret_cast<const d2 *>(rec + 4 * (((size_t)cx * (g.ny + 1) + cy) * (g.nz + 2) + cz));
  const d2 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3];
  values[0][0][0] = q0.x; values[0][1][0] = q0.y; values[1][0][0] = q1.x; values[1][1][0] = q1.y;
  values[0][0][1] = q2.x; values[0][1][1] = q2.y; values[1][0][1] = q3.x; values[1][1][1] = q3.y;
}

// base index and diff of the point p, sdf_map.cpp:201-209, and the 8 corner values of that cell
__device__ __forceinline__ void gtop_edt_corners(const GtopGrid &g, const double *__restrict__ rec, const double p[3],
                                                 int idx[3], double diff[3], double values[2][2][2]) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) {
    const double pm = p[k] - 0.5 * g.res;
    idx[k] = (int)floor((pm - g.origin[k]) * g.res_inv);
    diff[k] = (p[k] - ((idx[k] + 0.5) * g.res + g.origin[k])) * g.res_inv;
  }
  gtop_edt_cell_values(g, rec, idx, values);
}

// the largest of the 8 corner values (0 at least): what a box has to undercut to matter
__device__ __forceinline__ double gtop_edt_vmax(const double values[2][2][2]) {
  double vmax = 0.0;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int z = 0; z < 2; ++z) vmax = fmax(vmax, values[x][y][z]);
  return vmax;
}

// the faces of box bx = {p0, vel, scale} at time t (obj_predictor.h:57-66, edt_environment.cpp:30-33)
__device__ __forceinline__ void gtop_edt_box_faces(const double *bx, double t, double bmin[3], double bmax[3]) {
  for (int k = 0; k < 3; ++k) {
    const double c = bx[k] + bx[3 + k] * t;
    bmax[k] = c + 0.5 * bx[6 + k];
    bmin[k] = c - 0.5 * bx[6 + k];
  }
}

// ---- the polynomial box list (gtop_set_moving_box_polynomials) ----
// A box's centre is a quintic per axis on a validity interval (PolynomialPrediction, obj_predictor.h:26-55; the call
// distToBox carries in a comment, edt_environment.cpp:28).  One row of kBoxRowPoly doubles (gtop_kernels.h) per box, the same for the
// queries, the report and the cost bodies:
//   [6 k + i] coefficient of t^i on axis k (18);  [18 + k] half extent scale_k / 2 (3);  [21] t1;  [22] t2;  [23] pad
// (no t_range: t1 = -inf, t2 = +inf, which clamp nothing).  The arithmetic is fixed by the interface (include/gtop.h):
// the time clamped into [t1, t2], then Horner in explicit fp64 fmas.  These two functions are its ONE statement on the
// device — P is whatever pointer the row is read through (LDS in the queries and the report, the constant address
// space in the cost bodies) — so the three kernels get the same centre, bit for bit.
constexpr int kBoxRowConstVel = 9;
template <typename P> __device__ __forceinline__ double gtop_box_poly_time(P row, double tau) {
  return fmin(fmax(tau, row[21]), row[22]);
}
template <typename P> __device__ __forceinline__ double gtop_box_poly_centre(P row, int k, double tc) {
  const P c = row + 6 * k;
  return fma(fma(fma(fma(fma(c[5], tc, c[4]), tc, c[3]), tc, c[2]), tc, c[1]), tc, c[0]);
}
// the faces of a polynomial box at time t; the extents are stored halved (0.5 * scale is exact, so c +- that is what
// gtop_edt_box_faces forms from the full extent)
__device__ __forceinline__ void gtop_edt_box_faces_poly(const double *row, double t, double bmin[3], double bmax[3]) {
  const double tc = gtop_box_poly_time(row, t);
  for (int k = 0; k < 3; ++k) {
    const double c = gtop_box_poly_centre(row, k, tc);
    bmax[k] = c + row[18 + k];
    bmin[k] = c - row[18 + k];
  }
}
// either list form (POLY: a template parameter of the query and report kernels)
template <bool POLY>
__device__ __forceinline__ void gtop_edt_box_faces_of(const double *row, double t, double bmin[3], double bmax[3]) {
  if constexpr (POLY) gtop_edt_box_faces_poly(row, t, bmin, bmax);
  else gtop_edt_box_faces(row, t, bmin, bmax);
}
template <bool POLY> constexpr int kBoxRowOf = POLY ? kBoxRowPoly : kBoxRowConstVel;

// boxes b0 .. b0 + nb - 1 into LDS as rows of p0, vel, scale, by the whole workgroup.  (With one wavefront per workgroup
// the barriers order that wavefront's own LDS reads and writes and nothing else.)
// POLY: box_p0 is the list's [nbox][kBoxRowPoly] rows, copied as they are.
template <bool POLY>
__device__ __forceinline__ void stage_boxes(double (*bx)[kBoxRowOf<POLY>], const double *__restrict__ box_p0,
                                            const double *__restrict__ box_vel, const double *__restrict__ box_scale,
                                            int b0, int nb, int tid, int nthreads) {
  constexpr int ROW = kBoxRowOf<POLY>;
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

// values := min(values, distance from each corner voxel's centre to the box) (edt_environment.cpp:26-73, :96-98)
__device__ __forceinline__ void gtop_edt_box_min(const GtopGrid &g, const double bmin[3], const double bmax[3],
                                                 const int idx[3], double values[2][2][2], double &vmax) {
  // per axis and corner offset: 0 inside the slab, else the distance to its nearer face (:36-40)
  double d1[3][2];
  for (int k = 0; k < 3; ++k)
    for (int o = 0; o < 2; ++o) {
      const double pt = (idx[k] + o + 0.5) * g.res + g.origin[k];
      d1[k][o] = (pt >= bmin[k] && pt <= bmax[k]) ? 0.0 : fmin(fabs(pt - bmin[k]), fabs(pt - bmax[k]));
    }
  // The corner nearest to the box takes, per axis, the smaller of the two offsets' distances, and its
  // distance is the same floating-point expression as in the loop below; every other corner's is no
  // smaller (sums of non-negative terms and sqrt round monotonically).  A box that does not undercut the
  // LARGEST of the 8 current values there cannot change any of them: skipped, bit for bit the same result —
  // with a few dozen boxes in a map most are far from a query (2^20 queries, 32 boxes: 323 -> 211 us; a
  // wavefront still pays for a box any of its 64 queries is near).
  const double near2 = fmin(d1[0][0], d1[0][1]) * fmin(d1[0][0], d1[0][1]) +
                       fmin(d1[1][0], d1[1][1]) * fmin(d1[1][0], d1[1][1]) +
                       fmin(d1[2][0], d1[2][1]) * fmin(d1[2][0], d1[2][1]);
  if (sqrt(near2) < vmax) {
    vmax = 0.0;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int z = 0; z < 2; ++z) {
          const double d2 = sqrt(d1[0][x] * d1[0][x] + d1[1][y] * d1[1][y] + d1[2][z] * d1[2][z]);   // dist.norm()
          values[x][y][z] = d2 < values[x][y][z] ? d2 : values[x][y][z];
          vmax = fmax(vmax, values[x][y][z]);
        }
  }
}

// ---- the TIME derivative of the box-lowered lookup (include/gtop_time_moving.h), stated here once ----
// The velocity c'_k of a box's centre at time t.  Constant velocity: vel_k.  Polynomial: the derivative of the quintic
// at the clamped time inside the open interval (t1, t2); outside it and at its ends the box stands: 0.
template <bool POLY>
__device__ __forceinline__ void gtop_edt_box_velocity_of(const double *row, double t, double cv[3]) {
  if constexpr (POLY) {
    const double tc = gtop_box_poly_time(row, t);
    const bool moves = t > row[21] && t < row[22];
    for (int k = 0; k < 3; ++k) {
      const double *c = row + 6 * k;
      const double v = fma(fma(fma(fma(5.0 * c[5], tc, 4.0 * c[4]), tc, 3.0 * c[3]), tc, 2.0 * c[2]), tc, c[1]);
      cv[k] = moves ? v : 0.0;
    }
  } else {
    for (int k = 0; k < 3; ++k) cv[k] = row[3 + k];
  }
}

// gtop_edt_box_min with the derivative of every corner value with respect to the box's time beside it: the VALUES are
// gtop_edt_box_min's expressions, skip included, so they come out bit for bit the same.  Per axis and corner offset
// d d1 / d t is 0 inside the slab, +c'_k below it (pt < bmin: d1 = bmin - pt) and -c'_k above it (pt > bmax).  A corner
// the box lowers (strictly: the static value wins a tie, and the earlier box among boxes) carries
// (sum_k d1_k d1'_k) / d2, 0 where d2 = 0; a corner it does not lower keeps what it carried (0 for a static value).
__device__ __forceinline__ void gtop_edt_box_min_dtau(const GtopGrid &g, const double bmin[3], const double bmax[3],
                                                      const double cv[3], const int idx[3], double values[2][2][2],
                                                      double dvals[2][2][2], double &vmax) {
  double d1[3][2], e1[3][2];
  for (int k = 0; k < 3; ++k)
    for (int o = 0; o < 2; ++o) {
      const double pt = (idx[k] + o + 0.5) * g.res + g.origin[k];
      d1[k][o] = (pt >= bmin[k] && pt <= bmax[k]) ? 0.0 : fmin(fabs(pt - bmin[k]), fabs(pt - bmax[k]));
      e1[k][o] = pt < bmin[k] ? cv[k] : (pt > bmax[k] ? -cv[k] : 0.0);
    }
  const double near2 = fmin(d1[0][0], d1[0][1]) * fmin(d1[0][0], d1[0][1]) +
                       fmin(d1[1][0], d1[1][1]) * fmin(d1[1][0], d1[1][1]) +
                       fmin(d1[2][0], d1[2][1]) * fmin(d1[2][0], d1[2][1]);
  if (sqrt(near2) < vmax) {
    vmax = 0.0;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int z = 0; z < 2; ++z) {
          const double d2 = sqrt(d1[0][x] * d1[0][x] + d1[1][y] * d1[1][y] + d1[2][z] * d1[2][z]);   // dist.norm()
          const double num = d1[0][x] * e1[0][x] + d1[1][y] * e1[1][y] + d1[2][z] * e1[2][z];
          const bool lower = d2 < values[x][y][z];
          dvals[x][y][z] = lower ? (d2 > 0.0 ? num / d2 : 0.0) : dvals[x][y][z];
          values[x][y][z] = lower ? d2 : values[x][y][z];
          vmax = fmax(vmax, values[x][y][z]);
        }
  }
}

// trilinear value, edt_environment.cpp:104-112 (= sdf_map.cpp:221-229); the intermediates are what the gradient
// (:114-121) is formed from
struct GtopTrilinear {
  double v00, v01, v10, v11, v0, v1, d;
};
__device__ __forceinline__ GtopTrilinear gtop_edt_trilinear(const double diff[3], const double values[2][2][2]) {
#pragma clang fp contract(off)
  GtopTrilinear r;
  r.v00 = (1 - diff[0]) * values[0][0][0] + diff[0] * values[1][0][0];
  r.v01 = (1 - diff[0]) * values[0][0][1] + diff[0] * values[1][0][1];
  r.v10 = (1 - diff[0]) * values[0][1][0] + diff[0] * values[1][1][0];
  r.v11 = (1 - diff[0]) * values[0][1][1] + diff[0] * values[1][1][1];
  r.v0 = (1 - diff[1]) * r.v00 + diff[1] * r.v10;
  r.v1 = (1 - diff[1]) * r.v01 + diff[1] * r.v11;
  r.d = (1 - diff[2]) * r.v0 + diff[2] * r.v1;
  return r;
}

// the gradient of that value, edt_environment.cpp:114-121 (= sdf_map.cpp:231-239), in the reference's unfused
// arithmetic: what gtop_edt_query_device returns beside the distance, and what gtop_insert_waypoints_device pushes a
// new waypoint along (gtop_insert.hip) — the same bits in both
__device__ __forceinline__ void gtop_edt_gradient(const GtopGrid &g, const double diff[3], const double values[2][2][2],
                                                  const GtopTrilinear &tl, double grad[3]) {
#pragma clang fp contract(off)
  double gx = (1 - diff[2]) * (1 - diff[1]) * (values[1][0][0] - values[0][0][0]);
  gx += (1 - diff[2]) * diff[1] * (values[1][1][0] - values[0][1][0]);
  gx += diff[2] * (1 - diff[1]) * (values[1][0][1] - values[0][0][1]);
  gx += diff[2] * diff[1] * (values[1][1][1] - values[0][1][1]);
  gx *= g.res_inv;
  grad[0] = gx;
  grad[1] = ((1 - diff[2]) * (tl.v10 - tl.v00) + diff[2] * (tl.v11 - tl.v01)) * g.res_inv;
  grad[2] = (tl.v1 - tl.v0) * g.res_inv;
}

#endif  // GTOP_EDT_LOOKUP_H_
