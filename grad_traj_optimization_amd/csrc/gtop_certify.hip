// gtop_certify.hip — the continuous-time clearance certificate of a batch of trajectories, on gfx950.  fp64: the
// static field (include/gtop.h, gtop_certify_trajectories_device) and, as a second kernel on the same
// interval tree, the static field with the context's moving boxes (gtop_certify_moving_device).
//
// The report of gtop_validate.hip looks the field up at the getTraj samples and knows nothing between two of them.
// This kernel bounds the interpolated distance over whole time intervals.  The lookup is trilinear, so affine in each
// coordinate inside a cell: over an axis-aligned box inside one cell its minimum is attained at a vertex of the box.
// A box that contains the curve over an interval, cut along the (at most 8) cells it touches, therefore gives a lower
// bound of the distance over that interval from 8 trilinear values per cell — whatever the field holds.
//
// One WAVEFRONT per trajectory, as the reports have it, on the interval tree of gtop_interval_tree.h: 64 intervals of a
// segment, or of an OPEN interval, per level.  The midpoint distance is the `dist` of edt_query_kernel<false> for
// (p, -1) through the shared lookup of gtop_edt_lookup.h: the same bits.
//
// With boxes the certified quantity is the query's `dist` for (x(t), start + t): the trilinear form over corner values
// min(static, distance from the corner voxel's centre to the nearest box).  The form does not decrease when a corner
// value grows, and a corner's distance to a box does not grow when the box's faces move outwards: with every box
// replaced by an axis-aligned box that contains it over the interval's whole range of box time, the same vertex minimum
// per touched cell is a lower bound for every point and time of the interval.  The box policy (CertNoBoxes /
// CertBoxList<POLY>) is a template parameter of the interval evaluation; the tree, the status rule and the outputs are
// one statement for both kernels.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_device_common.h"   // poly_eval
#include "gtop_edt_lookup.h"
#include "gtop_kernels.h"
#include "gtop_report_common.h"   // poly_vel

// The certifier's own arithmetic is unfused: interval ends, radii, cell ranges, sub-boxes and vertex values round as a
// numpy restatement of them does (tests/certify_twin.py).  (poly_vel, included above, keeps the fmas it has everywhere.)
#pragma clang fp contract(off)

#include "gtop_interval_tree.h"   // the tree, the statuses, the segment's staging, a row's verdict

namespace {

struct CertParams {
  GtopGrid g;
  const double *rec;
  double margin, kappa, e_map;   // kappa, e_map: the two rounding allowances' grid-dependent parts (the launcher)
  int max_depth, max_refine;
};
struct CertSeg {
  const double *cf;   // the segment's 18 coefficients (in LDS, see the kernel)
  double A[3], E[3];  // per axis: the acceleration bound and the absolute slack of the box
  double t_off;       // trajectory time of the segment's start
};
struct CertLane {     // a lane's running results
  double lo, hi, hi_t, viol_t;
};

// The box policy of an interval evaluation.  CertNoBoxes: the static certificate.  CertBoxList<POLY>: the context's
// list, staged in LDS in the chunks of the report (gtop_report_common.h), and the row's clock.
struct CertNoBoxes {
  static constexpr bool kMoving = false;
};
template <bool POLY> struct CertBoxList {
  static constexpr bool kMoving = true;
  static constexpr bool kPoly = POLY;
  double (*bx)[kBoxRowOf<POLY>];               // LDS: the list's first chunk, or the chunk staged last
  int nbox;
  const double *box_p0, *box_vel, *box_scale;  // POLY: box_p0 is the list's rows, the other two are not read
  double start;                                // the row's start time on the boxes' clock
  double delta;                                // the segment's allowance on the ends of a range of box time
};

__device__ __forceinline__ double cert_clamp01(double u) { return fmin(fmax(u, 0.0), 1.0); }

// Cell `cell` with the corner values `values`: vmin lowered by the trilinear values at the 8 vertices of the box
// [blo, bhi] cut to the cell.
__device__ __forceinline__ void cert_vertex_min(const GtopGrid &g, const int cell[3], const double values[2][2][2],
                                                const double blo[3], const double bhi[3], double &vmin) {
  double u[3][2];
  for (int k = 0; k < 3; ++k) {                         // the box cut to the cell, in the cell's local coordinates
    const double c0 = (cell[k] + 0.5) * g.res + g.origin[k];
    u[k][0] = cert_clamp01((blo[k] - c0) * g.res_inv);
    u[k][1] = cert_clamp01((bhi[k] - c0) * g.res_inv);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const double diff[3] = {u[0][e >> 2], u[1][(e >> 1) & 1], u[2][e & 1]};
    vmin = fmin(vmin, gtop_edt_trilinear(diff, values).d);
  }
}
// The larger of V and the largest absolute corner value of a cell: what the rounding of its forms scales with.
__device__ __forceinline__ double cert_corner_abs(const double values[2][2][2], double V) {
#pragma unroll
  for (int e = 0; e < 8; ++e) V = fmax(V, fabs(values[e >> 2][(e >> 1) & 1][e & 1]));
  return V;
}
// The lower bound from the vertex minimum and the largest absolute corner value of the cells touched.
__device__ __forceinline__ double cert_lb(double vmin, double vabs, double kappa) {
  const double lb = vmin - kappa * vabs;
  return lb == lb ? lb : -INFINITY;                     // (a NaN in the field certifies nothing)
}

// An axis-aligned box that contains the box of row `row` at every box time of [ta, tb] (include/gtop.h).
// Constant velocity: the faces at either end; the centre is a monotone function of the time, so are the faces.
__device__ __forceinline__ void cert_swept_faces(const double *row, double ta, double tb, double smin[3], double smax[3]) {
  double amin[3], amax[3], bmin[3], bmax[3];
  gtop_edt_box_faces(row, ta, amin, amax);
  gtop_edt_box_faces(row, tb, bmin, bmax);
  for (int k = 0; k < 3; ++k) {
    smin[k] = fmin(amin[k], bmin[k]);
    smax[k] = fmax(amax[k], bmax[k]);
  }
}
// A polynomial box: the centre at the middle of the clamped range and a radius from the velocity there and a bound of
// the acceleration over the range, as the curve's own box is formed.  A centre or radius that is not finite gives the
// box that covers everything.
__device__ __forceinline__ void cert_swept_faces_poly(const double *row, double ta, double tb, double smin[3],
                                                      double smax[3]) {
  const double tca = gtop_box_poly_time(row, ta), tcb = gtop_box_poly_time(row, tb);
  const double hh = 0.5 * (tcb - tca), tm = tca + hh, M = fmax(fabs(tca), fabs(tcb));
  const double M2 = M * M, M3 = M2 * M;
  for (int k = 0; k < 3; ++k) {
    const double *c = row + 6 * k;
    const double cm = gtop_box_poly_centre(row, k, tm);
    const double vq = ((((5.0 * c[5]) * tm + 4.0 * c[4]) * tm + 3.0 * c[3]) * tm + 2.0 * c[2]) * tm + c[1];
    const double Aq = 2.0 * fabs(c[2]) + 6.0 * fabs(c[3]) * M + 12.0 * fabs(c[4]) * M2 + 20.0 * fabs(c[5]) * M3;
    const double Qk = ((((fabs(c[5]) * M + fabs(c[4])) * M + fabs(c[3])) * M + fabs(c[2])) * M + fabs(c[1])) * M +
                      fabs(c[0]);
    double rq = fabs(vq) * hh + 0.5 * Aq * hh * hh;
    rq = rq * GTOP_CERT_INFLATE + GTOP_CERT_SLACK * Qk;
    const bool ok = isfinite(cm) && isfinite(rq);
    smin[k] = ok ? (cm - rq) - row[18 + k] : -INFINITY;
    smax[k] = ok ? (cm + rq) + row[18 + k] : INFINITY;
  }
}

// The lower bound of an interval against the static field and the boxes X over the box times [tau_a, tau_b]: the static
// bound's cells and vertices, each cell's corner values lowered to the distance to every box's swept faces.  Every loop
// is wave-uniform, a lane's own conditions (its box is `bad`, it does not touch cell q, its whole range of box time is
// negative) sit inside: a list longer than a chunk is restaged in the middle of it, as sample_distance does.  One
// cell's values are live at a time; a box's swept faces are formed again for every cell.
template <bool POLY>
__device__ __forceinline__ double cert_moving_bound(const CertParams &P, const CertBoxList<POLY> &X, const double blo[3],
                                                    const double bhi[3], bool bad, const int i0[3], const int span[3],
                                                    double tau_a, double tau_b, int lane) {
  constexpr int kChunk = kValBoxChunkOf<POLY>;
  const GtopGrid &g = P.g;
  const bool apply = tau_b >= 0.0;
  double vmin = INFINITY, vabs = 0.0;
#pragma unroll 1
  for (int q = 0; q < 8; ++q) {
    const int dx = q >> 2, dy = (q >> 1) & 1, dz = q & 1;
    const bool on = !bad && dx <= span[0] && dy <= span[1] && dz <= span[2];
    if (!__ballot(on)) continue;                        // wave-uniform
    const int cell[3] = {i0[0] + dx, i0[1] + dy, i0[2] + dz};
    double values[2][2][2];
    gtop_edt_cell_values(g, P.rec, cell, values);       // (a lane that is not `on` reads a clamped cell: memory-safe)
    const double V = cert_corner_abs(values, 0.0);         // of the STATIC values: what the forms at any time scale with
    double vmax = gtop_edt_vmax(values);
#pragma unroll 1
    for (int b0 = 0; b0 < X.nbox; b0 += kChunk) {
      const int nb = min(kChunk, X.nbox - b0);
      if (X.nbox > kChunk) stage_boxes<POLY>(X.bx, X.box_p0, X.box_vel, X.box_scale, b0, nb, lane, 64);
      if (on && apply) {
#pragma unroll 1
        for (int j = 0; j < nb; ++j) {
          double smin[3], smax[3];
          if constexpr (POLY) cert_swept_faces_poly(X.bx[j], tau_a, tau_b, smin, smax);
          else cert_swept_faces(X.bx[j], tau_a, tau_b, smin, smax);
          gtop_edt_box_min(g, smin, smax, cell, values, vmax);
        }
      }
    }
    if (on) {
      cert_vertex_min(g, cell, values, blo, bhi, vmin);
      vabs = fmax(vabs, V);
    }
  }
  return bad ? -INFINITY : cert_lb(vmin, vabs, P.kappa);
}

// One interval [a, a + w] of segment S: the midpoint's distance into R; returns the interval's status, its lower
// bound in lb.  X: the box policy.
template <class BOXES>
__device__ __forceinline__ int cert_eval(const CertParams &P, const CertSeg &S, const BOXES &X, double a, double w,
                                         int lane, CertLane &R, double &lb) {
  const GtopGrid &g = P.g;
  const double h = 0.5 * w, tc = a + h;
  double p[3], blo[3], bhi[3];
  for (int k = 0; k < 3; ++k) {
    const double *c = S.cf + 6 * k;
    p[k] = poly_eval(c, tc);
    const double v = poly_vel(c, tc);
    double r = fabs(v) * h + 0.5 * S.A[k] * h * h;
    r = r * GTOP_CERT_INFLATE + S.E[k];
    blo[k] = p[k] - r;
    bhi[k] = p[k] + r;
  }
  // the midpoint: evaluateEDTWithGrad(p, -1)'s value, as edt_query_kernel<false> forms it
  bool viol;
  {
    const double t = S.t_off + tc;
    double d;
    if constexpr (BOXES::kMoving) {                     // with boxes: edt_query_kernel<false, POLY>'s, for (p, start + t)
      d = sample_distance<BOXES::kPoly, true>(g, P.rec, X.bx, X.nbox, X.box_p0, X.box_vel, X.box_scale, true, X.start, t,
                                              true, p, lane).d;
    } else {
      const bool out = gtop_edt_out_of_map(g, p);
      int idx[3];
      double diff[3], values[2][2][2];
      gtop_edt_corners(g, P.rec, p, idx, diff, values);
      d = out ? -1.0 : gtop_edt_trilinear(diff, values).d;
    }
    if (d < R.hi || (d == R.hi && t < R.hi_t)) {
      R.hi = d; R.hi_t = t;
    }
    viol = d <= P.margin;                               // the report's comparison
    if (viol) R.viol_t = fmin(R.viol_t, t);
  }
  // the lower bound over the box
  bool bad = gtop_edt_out_of_map(g, blo) || gtop_edt_out_of_map(g, bhi);
  int i0[3] = {0, 0, 0}, span[3] = {0, 0, 0};
  if (!bad) {
    for (int k = 0; k < 3; ++k) {                       // the lookup's own cells, gtop_edt_corners
      const double lm = blo[k] - 0.5 * g.res, hm = bhi[k] - 0.5 * g.res;
      i0[k] = (int)floor((lm - g.origin[k]) * g.res_inv);
      span[k] = (int)floor((hm - g.origin[k]) * g.res_inv) - i0[k];
      bad |= !(span[k] >= 0 && span[k] <= 1);
    }
  }
  if constexpr (BOXES::kMoving) {
    // the box times of the interval, widened by the allowance on their rounding (include/gtop.h)
    const double ta = X.start + (S.t_off + a), tb = X.start + (S.t_off + (a + w));
    lb = cert_moving_bound(P, X, blo, bhi, bad, i0, span, ta - X.delta, tb + X.delta, lane);
  } else {
    lb = -INFINITY;
    if (!bad) {
      double vmin = INFINITY, vabs = 0.0;
#pragma unroll 1
      for (int q = 0; q < 8; ++q) {                     // (bounded whatever the spans hold)
        const int dx = q >> 2, dy = (q >> 1) & 1, dz = q & 1;
        if (dx > span[0] || dy > span[1] || dz > span[2]) continue;
        const int cell[3] = {i0[0] + dx, i0[1] + dy, i0[2] + dz};
        double values[2][2][2];
        gtop_edt_cell_values(g, P.rec, cell, values);
        cert_vertex_min(g, cell, values, blo, bhi, vmin);
        vabs = cert_corner_abs(values, vabs);
      }
      lb = cert_lb(vmin, vabs, P.kappa);
    }
  }
  return viol ? kViolation : (lb > P.margin ? kCertified : kOpen);
}

// What the clearance certificates add to the tree (gtop_interval_tree.h): an interval's lower bound, and a leaf's into
// the lane's lo.
template <class BOXES> struct CertNode {
  struct Bound {
    double lb;
  };
  const CertParams &P;
  const CertSeg &S;
  const BOXES &X;
  CertLane &R;
  __device__ __forceinline__ int eval(double a, double w, int lane, Bound &b) {
    return cert_eval(P, S, X, a, w, lane, R, b.lb);
  }
  __device__ __forceinline__ void leaf(const Bound &b) { R.lo = fmin(R.lo, b.lb); }
};

// One trajectory, by one wavefront: its segments in order, then the wavefront's reductions and the row of the output.
// seg_c: 18 doubles of LDS, the segment's coefficients (gtop_tree_stage_segment).
template <class BOXES>
__device__ __forceinline__ void cert_trajectory(const CertParams &P, BOXES &X, double *seg_c, int b, int lane, int m,
                                                const double *__restrict__ coeff, const double *__restrict__ T,
                                                int t_stride, double *__restrict__ cert) {
  const double *cf = coeff + (size_t)b * m * 18;   // row s = [cx0..5 | cy0..5 | cz0..5], ascending powers
  const double *ts = T + (size_t)b * t_stride;
  CertLane R = {INFINITY, INFINITY, 0.0, INFINITY};
  int nref = 0, nund = 0;
  double t_off = 0.0;                               // accumulated as the reports accumulate time_sum
  for (int s = 0; s < m; ++s) {
    const double Ts = ts[s], T2 = Ts * Ts, T3 = T2 * Ts;
    CertSeg S;
    gtop_tree_stage_segment(seg_c, cf, s, lane);
    S.cf = seg_c;
    S.t_off = t_off;
    for (int k = 0; k < 3; ++k) {
      const double *c = S.cf + 6 * k;
      S.A[k] = 2.0 * fabs(c[2]) + 6.0 * fabs(c[3]) * Ts + 12.0 * fabs(c[4]) * T2 + 20.0 * fabs(c[5]) * T3;
      // P_k = sum_j |c_j| Ts^j: what the position's and the velocity's rounding errors scale by
      const double Pk = ((((fabs(c[5]) * Ts + fabs(c[4])) * Ts + fabs(c[3])) * Ts + fabs(c[2])) * Ts + fabs(c[1])) * Ts +
                        fabs(c[0]);
      S.E[k] = GTOP_CERT_SLACK * Pk + P.e_map;
    }
    // the largest box time of the segment is what the ends of its ranges of box time round by
    if constexpr (BOXES::kMoving) X.delta = GTOP_CERT_SLACK * (fabs(X.start) + (t_off + Ts));
    CertNode<BOXES> N = {P, S, X, R};
    gtop_tree_level<0>(N, P.max_depth, P.max_refine, 0.0, 0.015625 * Ts, lane, nref, nund);
    t_off += Ts;
  }

  // ---- the wavefront's reductions ----
  double lo = R.lo, vt = R.viol_t, hd = R.hi, ht = R.hi_t;
  for (int off = 32; off > 0; off >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, off));
    vt = fmin(vt, __shfl_xor(vt, off));
    const double od = __shfl_xor(hd, off), ot = __shfl_xor(ht, off);   // lexicographic min of (distance, time)
    if (od < hd || (od == hd && ot < ht)) {
      hd = od; ht = ot;
    }
  }
  if (lane == 0) {
    double *o = cert + (size_t)b * GTOP_CERT_REPORT;
    o[0] = gtop_tree_verdict(vt, nund);
    o[1] = lo; o[2] = hd; o[3] = ht;
    o[4] = gtop_tree_first_violation(vt);
    o[5] = (double)nund; o[6] = (double)nref; o[7] = t_off;
  }
}

__global__ void __launch_bounds__(64)
traj_certify_kernel(const CertParams P, int B, int m, const double *__restrict__ coeff, const double *__restrict__ T,
                    int t_stride, double *__restrict__ cert /*[B][GTOP_CERT_REPORT]*/) {
  __shared__ double seg_c[18];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  CertNoBoxes X;
  cert_trajectory(P, X, seg_c, b, lane, m, coeff, T, t_stride, cert);
}

// The same against the static field AND the boxes (nbox > 0; POLY: box_p0 is the polynomial list's rows), at the box
// time t0[b * t0_stride] + t (t0 NULL: 0 + t).  The list's first chunk is staged once; a longer list is restaged
// inside the interval evaluation.
template <bool POLY>
__global__ void __launch_bounds__(64)
traj_certify_moving_kernel(const CertParams P, int nbox, const double *__restrict__ box_p0,
                           const double *__restrict__ box_vel, const double *__restrict__ box_scale,
                           const double *__restrict__ t0, int t0_stride, int B, int m,
                           const double *__restrict__ coeff, const double *__restrict__ T, int t_stride,
                           double *__restrict__ cert /*[B][GTOP_CERT_REPORT]*/) {
  constexpr int kChunk = kValBoxChunkOf<POLY>;
  __shared__ double seg_c[18];
  __shared__ double bx[kChunk][kBoxRowOf<POLY>];
  // The grid and the options are wave-uniform too, and beside the list's pointers, the row's clock and the masks of the
  // box loops they no longer fit the scalar register file: they go the way of the segment's coefficients.
  __shared__ CertParams Ps;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  if (lane == 0) Ps = P;
  stage_boxes<POLY>(bx, box_p0, box_vel, box_scale, 0, min(kChunk, nbox), lane, 64);
  CertBoxList<POLY> X = {bx, nbox, box_p0, box_vel, box_scale, t0 ? t0[(size_t)b * t0_stride] : 0.0, 0.0};
  cert_trajectory(Ps, X, seg_c, b, lane, m, coeff, T, t_stride, cert);
}

}  // namespace

// The grid-dependent parts of the two allowances, in plain fp64 so that a restatement follows:
// coord = the largest absolute coordinate a face of a cell of the map can have, cells = that in units of res.
static CertParams cert_params(const GtopGrid &g, const double *rec, double margin, int max_depth, int max_refine) {
  double coord = 0.0;
  int nmax = g.nx > g.ny ? g.nx : g.ny;
  nmax = nmax > g.nz ? nmax : g.nz;
  for (int k = 0; k < 3; ++k) {
    coord = fmax(coord, fmax(fabs(g.origin[k]), fmax(fabs(g.min_range[k]), fabs(g.max_range[k]))));
  }
  coord = coord + (nmax + 2) * g.res;
  const double cells = coord * g.res_inv;
  CertParams P;
  P.g = g;
  P.rec = rec;
  P.margin = margin;
  P.kappa = GTOP_CERT_KAPPA * (8.0 + cells);
  P.e_map = GTOP_CERT_SLACK * coord;
  P.max_depth = max_depth;
  P.max_refine = max_refine;
  return P;
}

hipError_t gtop_launch_traj_certify(const GtopGrid &g, const double *rec, int B, int m, const double *coeff,
                                    const double *T, int t_stride, double margin, int max_depth, int max_refine,
                                    double *cert, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const CertParams P = cert_params(g, rec, margin, max_depth, max_refine);
  hipLaunchKernelGGL(traj_certify_kernel, dim3(B), dim3(64), 0, stream, P, B, m, coeff, T, t_stride, cert);
  return hipGetLastError();
}

hipError_t gtop_launch_traj_certify_moving(const GtopGrid &g, const double *rec, const GtopBoxList &boxes, int B, int m,
                                           const double *coeff, const double *T, int t_stride, const double *t0,
                                           int t0_stride, double margin, int max_depth, int max_refine, double *cert,
                                           hipStream_t stream) {
  if (boxes.count <= 0)   // no boxes: the static certificate, the same launch
    return gtop_launch_traj_certify(g, rec, B, m, coeff, T, t_stride, margin, max_depth, max_refine, cert, stream);
  if (B <= 0) return hipSuccess;
  const CertParams P = cert_params(g, rec, margin, max_depth, max_refine);
  if (boxes.kind == GTOP_BOX_LIST_POLYNOMIAL)
    hipLaunchKernelGGL(traj_certify_moving_kernel<true>, dim3(B), dim3(64), 0, stream, P, boxes.count, boxes.rows,
                       nullptr, nullptr, t0, t0_stride, B, m, coeff, T, t_stride, cert);
  else
    hipLaunchKernelGGL(traj_certify_moving_kernel<false>, dim3(B), dim3(64), 0, stream, P, boxes.count, boxes.p0,
                       boxes.vel, boxes.scale, t0, t0_stride, B, m, coeff, T, t_stride, cert);
  return hipGetLastError();
}
