// gtop_kinematics.hip — the continuous-time KINEMATIC certificate of a batch of trajectories, on gfx950, fp64
// (include/gtop_kinematics.h, gtop_certify_kinematics_device).
//
// The reports of gtop_validate.hip and gtop_segments.hip take the maxima of the velocity and the acceleration over the
// getTraj samples and know nothing between two of them.  This kernel bounds ‖v‖, ‖a‖, max|v_k| and max|a_k| over whole
// time intervals: the value at the interval's midpoint, the first-order term from the next derivative there, and a
// bound of the derivative after that over the segment (Taylor's theorem about the midpoint).  It needs no field, no
// parameters and no boxes.
//
// The interval tree is the clearance certificate's (gtop_interval_tree.h): one WAVEFRONT per trajectory, 64 intervals
// of a segment or of an OPEN interval per level.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_kernels.h"

// Every step is ONE rounded fp64 operation in the order the header writes it: a numpy restatement reproduces the bits
// (tests/kinematics_twin.py).  The file writes its own Horner expressions for that reason.
#pragma clang fp contract(off)

#include "gtop_interval_tree.h"   // the tree, the statuses, the segment's staging, a row's verdict

static_assert(GTOP_KIN_SEG == GTOP_SEG_REPORT, "a seg buffer is legal d_seg_report input to the LIMITS reallocation");

namespace {

struct KinParams {
  double max_vel, max_acc;   // <= 0 (or NaN): that limit is off
  int per_axis, max_depth, max_refine;
};
struct KinSeg {
  const double *cf;              // the segment's 18 coefficients (in LDS, see the kernel)
  double J[3], S[3], EV[3], EA[3];   // per axis: the bounds of |jerk| and |snap|, the two absolute slacks
  double t_off;                  // trajectory time of the segment's start
};
// A lane's running results.  Figures 0 .. 3: ‖v‖, ‖a‖, max|v_k|, max|a_k| (columns 2 .. 5 and 6 .. 9 of a seg row).
struct KinLane {
  double slo[4], sub[4];                // of the segment: midpoint maxima (every level), upper bounds (leaves)
  double lo_v, lo_v_t, lo_a, lo_a_t;    // of the trajectory, the chosen figures: (value, earliest time)
  double viol_t;
  bool sviol;                           // a violating midpoint in the segment
};

__device__ __forceinline__ double kin_max3(double a, double b, double c) { return fmax(fmax(a, b), c); }

// One interval [a, a + w] of segment S: the midpoint figures into R; returns the interval's status, its four upper
// bounds in ub.
__device__ __forceinline__ int kin_eval(const KinParams &P, const KinSeg &S, double a, double w, KinLane &R,
                                        double ub[4]) {
  const double h = 0.5 * w, tc = a + h, t = S.t_off + tc;
  double v[3], ac[3], Uv[3], Ua[3];
  for (int k = 0; k < 3; ++k) {
    const double *c = S.cf + 6 * k;
    v[k] = ((((5.0 * c[5]) * tc + 4.0 * c[4]) * tc + 3.0 * c[3]) * tc + 2.0 * c[2]) * tc + c[1];
    ac[k] = (((20.0 * c[5]) * tc + 12.0 * c[4]) * tc + 6.0 * c[3]) * tc + 2.0 * c[2];
    const double j = ((60.0 * c[5]) * tc + 24.0 * c[4]) * tc + 6.0 * c[3];
    const double rv = (fabs(ac[k]) * h + 0.5 * S.J[k] * h * h) * GTOP_CERT_INFLATE + S.EV[k];
    const double ra = (fabs(j) * h + 0.5 * S.S[k] * h * h) * GTOP_CERT_INFLATE + S.EA[k];
    Uv[k] = fabs(v[k]) + rv;
    Ua[k] = fabs(ac[k]) + ra;
  }
  const double mid[4] = {sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), sqrt(ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2]),
                         kin_max3(fabs(v[0]), fabs(v[1]), fabs(v[2])), kin_max3(fabs(ac[0]), fabs(ac[1]), fabs(ac[2]))};
  ub[0] = sqrt(Uv[0] * Uv[0] + Uv[1] * Uv[1] + Uv[2] * Uv[2]) * GTOP_CERT_INFLATE;
  ub[1] = sqrt(Ua[0] * Ua[0] + Ua[1] * Ua[1] + Ua[2] * Ua[2]) * GTOP_CERT_INFLATE;
  ub[2] = kin_max3(Uv[0], Uv[1], Uv[2]);
  ub[3] = kin_max3(Ua[0], Ua[1], Ua[2]);
  // a NaN certifies nothing: the norm's bound is NaN as soon as one axis' is, and then takes the per-axis one with it
  if (!(ub[0] == ub[0])) ub[0] = ub[2] = INFINITY;
  if (!(ub[1] == ub[1])) ub[1] = ub[3] = INFINITY;
#pragma unroll
  for (int f = 0; f < 4; ++f) R.slo[f] = fmax(R.slo[f], mid[f]);
  const double Fv = P.per_axis ? mid[2] : mid[0], Fa = P.per_axis ? mid[3] : mid[1];
  const double Bv = P.per_axis ? ub[2] : ub[0], Ba = P.per_axis ? ub[3] : ub[1];
  if (Fv > R.lo_v || (Fv == R.lo_v && t < R.lo_v_t)) {
    R.lo_v = Fv; R.lo_v_t = t;
  }
  if (Fa > R.lo_a || (Fa == R.lo_a && t < R.lo_a_t)) {
    R.lo_a = Fa; R.lo_a_t = t;
  }
  const bool on_v = P.max_vel > 0.0, on_a = P.max_acc > 0.0;
  const bool viol = (on_v && Fv > P.max_vel) || (on_a && Fa > P.max_acc);   // the report passes figure <= limit
  if (viol) {
    R.viol_t = fmin(R.viol_t, t);
    R.sviol = true;
  }
  const bool cert = (!on_v || Bv <= P.max_vel) && (!on_a || Ba <= P.max_acc);
  return viol ? kViolation : (cert ? kCertified : kOpen);
}

// What the kinematic certificate adds to the tree (gtop_interval_tree.h): an interval's four upper bounds, and a leaf's
// into the segment's.  The options and the segment are held by value: behind references the compiler forms the integer
// multiples of the coefficients (21 products) a second time and reads six coefficients again, 2 % of the launch.
struct KinNode {
  struct Bound {
    double ub[4];
  };
  const KinParams P;
  const KinSeg S;
  KinLane &R;
  __device__ __forceinline__ int eval(double a, double w, int, Bound &b) { return kin_eval(P, S, a, w, R, b.ub); }
  __device__ __forceinline__ void leaf(const Bound &b) {
#pragma unroll
    for (int f = 0; f < 4; ++f) R.sub[f] = fmax(R.sub[f], b.ub[f]);
  }
};

// One trajectory per 64-lane workgroup.  seg_c: 18 doubles of LDS, the segment's coefficients (gtop_tree_stage_segment).
__global__ void __launch_bounds__(64)
traj_kinematics_kernel(const KinParams P, int B, int m, const double *__restrict__ coeff, const double *__restrict__ T,
                       int t_stride, double *__restrict__ kin /*[B][GTOP_KIN_REPORT]*/,
                       double *__restrict__ seg /*[B][m][GTOP_KIN_SEG] or NULL*/) {
  __shared__ double seg_c[18];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const double *cf = coeff + (size_t)b * m * 18;   // row s = [cx0..5 | cy0..5 | cz0..5], ascending powers
  const double *ts = T + (size_t)b * t_stride;
  KinLane R;
  R.lo_v = R.lo_a = -INFINITY;
  R.lo_v_t = R.lo_a_t = INFINITY;
  R.viol_t = INFINITY;
  int nref = 0, nund = 0;
  double t_off = 0.0;                               // accumulated as the reports accumulate time_sum
  double ub_v = -INFINITY, ub_a = -INFINITY;        // of the trajectory, the chosen figures (wave-uniform)
  for (int s = 0; s < m; ++s) {
    const double Ts = ts[s], T2 = Ts * Ts;
    KinSeg S;
    gtop_tree_stage_segment(seg_c, cf, s, lane);
    S.cf = seg_c;
    S.t_off = t_off;
    for (int k = 0; k < 3; ++k) {
      const double *c = S.cf + 6 * k;
      const double q1 = fabs(c[1]), q2 = fabs(c[2]), q3 = fabs(c[3]), q4 = fabs(c[4]), q5 = fabs(c[5]);
      S.J[k] = 6.0 * q3 + 24.0 * q4 * Ts + 60.0 * q5 * T2;
      S.S[k] = 24.0 * q4 + 120.0 * q5 * Ts;
      // what the velocity's and the acceleration's rounding errors scale with
      const double Vk = (((5.0 * q5 * Ts + 4.0 * q4) * Ts + 3.0 * q3) * Ts + 2.0 * q2) * Ts + q1;
      const double Ak = ((20.0 * q5 * Ts + 12.0 * q4) * Ts + 6.0 * q3) * Ts + 2.0 * q2;
      S.EV[k] = GTOP_CERT_SLACK * Vk;
      S.EA[k] = GTOP_CERT_SLACK * Ak;
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) R.slo[f] = R.sub[f] = -INFINITY;
    R.sviol = false;
    const int nref0 = nref, nund0 = nund;
    KinNode N = {P, S, R};
    gtop_tree_level<0>(N, P.max_depth, P.max_refine, 0.0, 0.015625 * Ts, lane, nref, nund);
    t_off += Ts;

    // ---- the segment's reductions and its row ----
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      double lo = R.slo[f], ub = R.sub[f];
      for (int off = 32; off > 0; off >>= 1) {
        lo = fmax(lo, __shfl_xor(lo, off));
        ub = fmax(ub, __shfl_xor(ub, off));
      }
      R.slo[f] = lo; R.sub[f] = ub;
    }
    const bool sviol = __ballot(R.sviol) != 0;
    ub_v = fmax(ub_v, P.per_axis ? R.sub[2] : R.sub[0]);
    ub_a = fmax(ub_a, P.per_axis ? R.sub[3] : R.sub[1]);
    if (seg && lane == 0) {
      double *o = seg + ((size_t)b * m + s) * GTOP_KIN_SEG;
      o[0] = sviol ? -1.0 : (nund == nund0 ? 1.0 : 0.0);
      o[1] = (double)(nref - nref0);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        o[2 + f] = R.slo[f];
        o[6 + f] = R.sub[f];
      }
    }
  }

  // ---- the trajectory's reductions: lexicographic (value descending, time ascending) ----
  double vt = R.viol_t, lv = R.lo_v, lvt = R.lo_v_t, la = R.lo_a, lat = R.lo_a_t;
  for (int off = 32; off > 0; off >>= 1) {
    vt = fmin(vt, __shfl_xor(vt, off));
    const double ov = __shfl_xor(lv, off), ovt = __shfl_xor(lvt, off);
    if (ov > lv || (ov == lv && ovt < lvt)) {
      lv = ov; lvt = ovt;
    }
    const double oa = __shfl_xor(la, off), oat = __shfl_xor(lat, off);
    if (oa > la || (oa == la && oat < lat)) {
      la = oa; lat = oat;
    }
  }
  if (lane == 0) {
    double *o = kin + (size_t)b * GTOP_KIN_REPORT;
    o[0] = gtop_tree_verdict(vt, nund);
    o[1] = ub_v; o[2] = lv; o[3] = lvt;
    o[4] = ub_a; o[5] = la; o[6] = lat;
    o[7] = gtop_tree_first_violation(vt);
    o[8] = (double)nund; o[9] = (double)nref; o[10] = t_off;
  }
}

}  // namespace

hipError_t gtop_launch_traj_kinematics(int B, int m, const double *coeff, const double *T, int t_stride, double max_vel,
                                       double max_acc, int per_axis, int max_depth, int max_refine, double *kin,
                                       double *seg, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const KinParams P = {max_vel, max_acc, per_axis, max_depth, max_refine};
  hipLaunchKernelGGL(traj_kinematics_kernel, dim3(B), dim3(64), 0, stream, P, B, m, coeff, T, t_stride, kin, seg);
  return hipGetLastError();
}
