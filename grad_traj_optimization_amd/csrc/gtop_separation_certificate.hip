// gtop_separation_certificate.hip — the continuous-time certificate of PAIRWISE SEPARATION of a batch of trajectories,
// on gfx950, fp64 (include/gtop_separation_certificate.h, gtop_certify_separation_device).
//
// gtop_separation.hip takes the least distance of two rows over grid samples and knows nothing between two of them.
// Here the distance of two curves is bounded from below over whole time intervals: the difference of the positions at
// the interval's midpoint, the first-order term from the difference of the velocities minimised EXACTLY over the
// interval (a point against a line segment), and a bound of the second-order remainder from the two segments'
// acceleration bounds.  It needs no field, no parameters and no boxes.
//
// The interval tree is the other certificates' (gtop_interval_tree.h), walked over the PIECES of a pair — the intervals
// between consecutive breakpoints of either row inside the pair's window — instead of the segments of a row:
//   (1) sepcert_boxes_kernel  (cull only) a wavefront per row: an axis-aligned box of its whole curve;
//   (2) sepcert_pairs_kernel  the hot one: a wavefront per pair i < j, its row stored to [i][j] and [j][i];
//   (3) sepcert_rows_kernel   a wavefront per row: the summary of row i of the matrix, and the diagonal entry.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_kernels.h"

// Every step is ONE rounded fp64 operation in the order the header writes it: a numpy restatement reproduces the bits
// (tests/sepcert_twin.py).  The file writes its own Horner expressions for that reason.
#pragma clang fp contract(off)

#include "gtop_interval_tree.h"   // the tree, the statuses, the segment's staging, a row's verdict

namespace {

constexpr double kShrink = 1.0 - 0x1p-40;   // a computed norm lowered past its rounding

struct SepCertParams {
  double min_sep, t_lo, t_hi;
  int max_depth, max_refine, hold_ends, cull;
};

// ---- what a row is inside one piece ----
enum { kBefore = -1, kAfter = -2 };   // standing; >= 0: the segment
// The row's state at common-clock time a, and the breakpoint at which it ends (INFINITY: none).  Wave-uniform.
struct RowClock {
  const double *ts;   // the row's m segment times
  double start, end;
  int m, hold;
  // the walk's own: segment s (never decreasing) and off_s, off_{s+1}
  int s;
  double off, off_next;
};
__device__ __forceinline__ void clock_init(RowClock &R, const double *ts, int m, double start, int hold) {
  R.ts = ts; R.m = m; R.start = start; R.hold = hold;
  double off = 0.0;
  for (int k = 0; k < m; ++k) off += ts[k];   // accumulated as the reports accumulate time_sum
  R.end = start + off;
  R.s = 0; R.off = 0.0; R.off_next = 0.0 + ts[0];
}
__device__ __forceinline__ int clock_state(RowClock &R, double a, double &next) {
  if (R.hold && a < R.start) {
    next = R.start;
    return kBefore;
  }
  if (R.hold && a >= R.end) {
    next = INFINITY;
    return kAfter;
  }
  while (R.s < R.m - 1 && R.start + R.off_next <= a) {
    ++R.s;
    R.off = R.off_next;
    R.off_next = R.off_next + R.ts[R.s];
  }
  next = R.start + R.off_next;
  return R.s;
}

// The library's sample expression (gtop_separation.h: position), unfused.
__device__ __forceinline__ double sample_value(const double *c, double u) {
  const double t2 = u * u, t3 = t2 * u, t4 = t2 * t2, t5 = t4 * u;
  return ((((((0.0 + t5 * c[5]) + t4 * c[4]) + t3 * c[3]) + t2 * c[2]) + u * c[1]) + c[0]);
}

// The row's 18 coefficients inside the piece into seg_c (LDS, gtop_tree_stage_segment's reason): segment `state`, or a
// standing row's (S, 0, 0, 0, 0, 0) per axis.
__device__ __forceinline__ void stage_row(double *seg_c, const double *cf, const RowClock &R, int state, int lane) {
  if (state >= 0) {
    gtop_tree_stage_segment(seg_c, cf, state, lane);
    return;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < 18) {
    double v = 0.0;
    if (lane % 6 == 0) v = state == kBefore ? cf[lane] : sample_value(cf + (R.m - 1) * 18 + lane, R.ts[R.m - 1]);
    seg_c[lane] = v;
  }
  __builtin_amdgcn_wave_barrier();
}

// Per axis the segment-wide bound of |acceleration|, and summed over the axes what the rounding errors of the position
// and of the velocity scale with.
struct RowBounds {
  double Acc[3], pos, vel;
};
__device__ __forceinline__ RowBounds row_bounds(const double *c18, double T) {
  RowBounds b;
  double P[3], V[3];
  for (int k = 0; k < 3; ++k) {
    const double *c = c18 + 6 * k;
    const double q0 = fabs(c[0]), q1 = fabs(c[1]), q2 = fabs(c[2]), q3 = fabs(c[3]), q4 = fabs(c[4]), q5 = fabs(c[5]);
    b.Acc[k] = ((20.0 * q5 * T + 12.0 * q4) * T + 6.0 * q3) * T + 2.0 * q2;
    V[k] = (((5.0 * q5 * T + 4.0 * q4) * T + 3.0 * q3) * T + 2.0 * q2) * T + q1;
    P[k] = ((((q5 * T + q4) * T + q3) * T + q2) * T + q1) * T + q0;
  }
  b.pos = (P[0] + P[1]) + P[2];
  b.vel = (V[0] + V[1]) + V[2];
  return b;
}

__device__ __forceinline__ double horner_pos(const double *c, double u) {
  return ((((c[5] * u + c[4]) * u + c[3]) * u + c[2]) * u + c[1]) * u + c[0];
}
__device__ __forceinline__ double horner_vel(const double *c, double u) {   // gtop_kinematics.hip's
  return ((((5.0 * c[5]) * u + 4.0 * c[4]) * u + 3.0 * c[3]) * u + 2.0 * c[2]) * u + c[1];
}
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// ---- the node ----
struct SepPiece {
  const double *ci, *cj;          // the two rows' 18 coefficients inside the piece (LDS)
  double start_i, off_i, start_j, off_j;
  double remc, E, min_sep;
};
// A lane's running results.
struct SepLane {
  double lo, hi, hi_t, viol_t;
};

// One interval [a, a + w] of the piece: the midpoint's figures into R; returns the status, the lower bound in lb.
__device__ __forceinline__ int sep_eval(const SepPiece &S, double a, double w, SepLane &R, double &lb) {
  const double h = 0.5 * w, tc = a + h;
  const double ui = (tc - S.start_i) - S.off_i, uj = (tc - S.start_j) - S.off_j;
  double D[3], W[3];
  for (int k = 0; k < 3; ++k) {
    D[k] = horner_pos(S.ci + 6 * k, ui) - horner_pos(S.cj + 6 * k, uj);
    W[k] = horner_vel(S.ci + 6 * k, ui) - horner_vel(S.cj + 6 * k, uj);
  }
  const double dmid = norm3(D[0], D[1], D[2]);
  const double DW = (D[0] * W[0] + D[1] * W[1]) + D[2] * W[2];
  const double WW = (W[0] * W[0] + W[1] * W[1]) + W[2] * W[2];
  const double q = (-DW) / WW;
  const double s = (WW == 0.0 || q != q) ? 0.0 : fmin(fmax(q, -h), h);
  const double dlin = norm3(D[0] + W[0] * s, D[1] + W[1] * s, D[2] + W[2] * s);
  const double rem = (S.remc * h) * h;
  lb = ((dlin * kShrink) - rem * GTOP_CERT_INFLATE) - S.E;
  if (!(lb == lb)) lb = -INFINITY;   // a NaN certifies nothing
  if (dmid < R.hi || (dmid == R.hi && tc < R.hi_t)) {
    R.hi = dmid; R.hi_t = tc;
  }
  const bool viol = dmid < S.min_sep;   // the sampled summary counts pair_min < radius
  if (viol) R.viol_t = fmin(R.viol_t, tc);
  return viol ? kViolation : (lb >= S.min_sep ? kCertified : kOpen);
}

// What the separation certificate adds to the tree; the piece is held by value, as KinNode holds its segment.
struct SepNode {
  struct Bound {
    double lb;
  };
  const SepPiece S;
  SepLane &R;
  __device__ __forceinline__ int eval(double a, double w, int, Bound &b) { return sep_eval(S, a, w, R, b.lb); }
  __device__ __forceinline__ void leaf(const Bound &b) { R.lo = fmin(R.lo, b.lb); }
};

// ---- (1) boxes ----
// One wavefront per row, lanes over the 64 intervals of a segment: a Taylor enclosure per axis about the interval's
// midpoint, reduced by min and max over the lanes and the segments.  box[b] = (xlo, ylo, zlo, xhi, yhi, zhi).
__global__ void __launch_bounds__(64)
sepcert_boxes_kernel(int B, int m, const double *__restrict__ coeff, const double *__restrict__ T, int t_stride,
                     double *__restrict__ box /*[B][6]*/) {
  __shared__ double seg_c[18];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const double *cf = coeff + (size_t)b * m * 18, *ts = T + (size_t)b * t_stride;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool nan = false;
  for (int s = 0; s < m; ++s) {
    const double Ts = ts[s], w = 0.015625 * Ts, a = (double)lane * w, h = 0.5 * w, tc = a + h;
    gtop_tree_stage_segment(seg_c, cf, s, lane);
    for (int k = 0; k < 3; ++k) {
      const double *c = seg_c + 6 * k;
      const double q0 = fabs(c[0]), q1 = fabs(c[1]), q2 = fabs(c[2]), q3 = fabs(c[3]), q4 = fabs(c[4]), q5 = fabs(c[5]);
      const double Acc = ((20.0 * q5 * Ts + 12.0 * q4) * Ts + 6.0 * q3) * Ts + 2.0 * q2;
      const double Pos = ((((q5 * Ts + q4) * Ts + q3) * Ts + q2) * Ts + q1) * Ts + q0;
      const double p = horner_pos(c, tc), v = horner_vel(c, tc);
      const double r = ((fabs(v) * h + ((0.5 * Acc) * h) * h) * GTOP_CERT_INFLATE) + GTOP_CERT_SLACK * Pos;
      const double l = p - r, u = p + r;
      nan |= !(l == l) || !(u == u);
      lo[k] = fmin(lo[k], l);
      hi[k] = fmax(hi[k], u);
    }
  }
  const bool unbounded = __ballot(nan) != 0;   // a NaN face encloses nothing: the row's box is the whole space
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], off));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], off));
    }
  if (lane < 6) {   // (a chain of selects: indexing lo / hi by the lane would put them in scratch memory)
    const double v = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lane == 2 ? lo[2] : lane == 3 ? hi[0] : lane == 4 ? hi[1] : hi[2];
    box[(size_t)b * 6 + lane] = unbounded ? (lane < 3 ? -INFINITY : INFINITY) : v;
  }
}

// ---- (2) pairs ----
// One wavefront per pair: linear index p = j (j - 1) / 2 + i, 0 <= i < j < B, so exactly B (B - 1) / 2 workgroups of one
// wavefront.  seg_c: 2 x 18 doubles of LDS, the two rows' coefficients inside the piece.  The merge of the two rows'
// breakpoints is wave-uniform scalar work; the lanes are the 64 intervals of a piece or of an OPEN interval.  No
// workgroup barrier, nothing per interval to HBM.
__global__ void __launch_bounds__(64)
sepcert_pairs_kernel(const SepCertParams P, int B, int m, const double *__restrict__ coeff, const double *__restrict__ T,
                     int t_stride, const double *__restrict__ t0, int t0_stride, const double *__restrict__ box,
                     double *__restrict__ pairs /*[B][B][GTOP_SEPCERT_PAIR]*/) {
  __shared__ double seg_c[2][18];
  const int p = blockIdx.x, lane = threadIdx.x;
  // the largest j with j (j - 1) / 2 <= p, by bisection in integers
  int jl = 1, jh = B - 1;
  while (jl < jh) {
    const int mid = (jl + jh + 1) >> 1;
    if (mid * (mid - 1) / 2 <= p) jl = mid;
    else jh = mid - 1;
  }
  const int j = jl, i = p - j * (j - 1) / 2;
  if (j >= B || i >= j) return;   // (never, with the launcher's grid)

  double out[GTOP_SEPCERT_PAIR] = {1.0, INFINITY, INFINITY, -1.0, -1.0, 0.0, 0.0, 0.0};
  bool culled = false;
  if (P.cull) {
    const double *bi = box + (size_t)i * 6, *bj = box + (size_t)j * 6;
    double g[3];
    for (int k = 0; k < 3; ++k) g[k] = fmax(fmax(bi[k] - bj[3 + k], bj[k] - bi[3 + k]), 0.0);
    const double boxdist = norm3(g[0], g[1], g[2]);
    if (boxdist >= P.min_sep) {
      out[1] = boxdist * kShrink;
      out[7] = -1.0;
      culled = true;
    }
  }
  if (!culled) {
    const double *cfi = coeff + (size_t)i * m * 18, *cfj = coeff + (size_t)j * m * 18;
    RowClock Ci, Cj;
    clock_init(Ci, T + (size_t)i * t_stride, m, t0 ? t0[(size_t)i * t0_stride] : 0.0, P.hold_ends);
    clock_init(Cj, T + (size_t)j * t_stride, m, t0 ? t0[(size_t)j * t0_stride] : 0.0, P.hold_ends);
    double wlo = P.t_lo, whi = P.t_hi;
    if (!P.hold_ends) {
      wlo = fmax(fmax(wlo, Ci.start), Cj.start);
      whi = fmin(fmin(whi, Ci.end), Cj.end);
    }
    if (wlo <= whi) {   // else: no common time
      SepLane R = {INFINITY, INFINITY, INFINITY, INFINITY};
      int nref = 0, nund = 0, pieces = 0;
      double a = wlo;
      for (int it = 0; it < 2 * m + 3; ++it) {   // 2 m + 2 breakpoints cut a held window into 2 m + 3 pieces; the
                                                 // bound holds whatever the times are
        double ni, nj;
        const int si = clock_state(Ci, a, ni), sj = clock_state(Cj, a, nj);
        const double nxt = fmin(fmin(whi, ni), nj);
        if (nxt > a || (it == 0 && whi == wlo)) {
          stage_row(seg_c[0], cfi, Ci, si, lane);
          stage_row(seg_c[1], cfj, Cj, sj, lane);
          const RowBounds bi = row_bounds(seg_c[0], si >= 0 ? Ci.ts[si] : 0.0);
          const RowBounds bj = row_bounds(seg_c[1], sj >= 0 ? Cj.ts[sj] : 0.0);
          const double A0 = bi.Acc[0] + bj.Acc[0], A1 = bi.Acc[1] + bj.Acc[1], A2 = bi.Acc[2] + bj.Acc[2];
          const double tmag = fmax(fmax(fabs(a), fabs(nxt)), fmax(fabs(Ci.start), fabs(Cj.start)));
          SepPiece S;
          S.ci = seg_c[0]; S.cj = seg_c[1];
          S.start_i = Ci.start; S.off_i = si >= 0 ? Ci.off : 0.0;
          S.start_j = Cj.start; S.off_j = sj >= 0 ? Cj.off : 0.0;
          S.remc = 0.5 * norm3(A0, A1, A2);
          S.E = GTOP_CERT_SLACK * ((bi.pos + bj.pos) + (bi.vel + bj.vel) * tmag);
          S.min_sep = P.min_sep;
          SepNode N = {S, R};
          gtop_tree_level<0>(N, P.max_depth, P.max_refine, a, 0.015625 * (nxt - a), lane, nref, nund);
          ++pieces;
        }
        if (nxt >= whi || !(nxt > a)) break;
        a = nxt;
      }
      // ---- the pair's reductions: lo and the violation by min; hi lexicographic (value, time) ascending ----
      double lo = R.lo, vt = R.viol_t, hv = R.hi, ht = R.hi_t;
      for (int off = 32; off > 0; off >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, off));
        vt = fmin(vt, __shfl_xor(vt, off));
        const double ov = __shfl_xor(hv, off), ot = __shfl_xor(ht, off);
        if (ov < hv || (ov == hv && ot < ht)) {
          hv = ov; ht = ot;
        }
      }
      out[0] = gtop_tree_verdict(vt, nund);
      out[1] = lo;
      out[2] = hv;
      out[3] = hv != INFINITY ? ht : -1.0;
      out[4] = gtop_tree_first_violation(vt);
      out[5] = (double)nund;
      out[6] = (double)nref;
      out[7] = (double)pieces;
    }
  }
  if (lane < 2 * GTOP_SEPCERT_PAIR) {   // lanes 0 .. 7: [i][j]; lanes 8 .. 15: [j][i]
    const int e = lane & (GTOP_SEPCERT_PAIR - 1);
    double v = out[0];
#pragma unroll
    for (int q = 1; q < GTOP_SEPCERT_PAIR; ++q) v = e == q ? out[q] : v;
    const size_t at = lane < GTOP_SEPCERT_PAIR ? (size_t)i * B + j : (size_t)j * B + i;
    pairs[at * GTOP_SEPCERT_PAIR + e] = v;
  }
}

// ---- (3) rows ----
// One wavefront per row i, lanes over j != i; it also writes the diagonal entry [i][i], which no pair owns.
__global__ void __launch_bounds__(64)
sepcert_rows_kernel(int B, double *__restrict__ pairs, double *__restrict__ rows /*[B][GTOP_SEPCERT_ROW]*/) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= B) return;
  const int kNone = 0x7fffffff;
  double lo = INFINITY, hi = INFINITY, hi_t = -1.0, vt = INFINITY;
  int lo_j = kNone, hi_j = kNone, unsafe = 0, undecided = 0, boxed = 0;
  for (int j = lane; j < B; j += 64) {   // rising j per lane: `<` keeps the first
    if (j == i) continue;
    const double *e = pairs + ((size_t)i * B + j) * GTOP_SEPCERT_PAIR;
    const double verdict = e[0];
    if (e[1] < lo) {
      lo = e[1]; lo_j = j;
    }
    if (e[2] < hi) {
      hi = e[2]; hi_j = j; hi_t = e[3];
    }
    if (verdict == -1.0) {
      ++unsafe;
      vt = fmin(vt, e[4]);
    }
    undecided += verdict == 0.0 ? 1 : 0;
    boxed += e[7] == -1.0 ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off), oht = __shfl_xor(hi_t, off);
    const int olj = __shfl_xor(lo_j, off), ohj = __shfl_xor(hi_j, off);
    if (ol < lo || (ol == lo && olj < lo_j)) {
      lo = ol; lo_j = olj;
    }
    if (oh < hi || (oh == hi && ohj < hi_j)) {
      hi = oh; hi_j = ohj; hi_t = oht;
    }
    vt = fmin(vt, __shfl_xor(vt, off));
    unsafe += __shfl_xor(unsafe, off);
    undecided += __shfl_xor(undecided, off);
    boxed += __shfl_xor(boxed, off);
  }
  if (lane == 0) {
    double *o = rows + (size_t)i * GTOP_SEPCERT_ROW;
    o[0] = unsafe ? -1.0 : (undecided ? 0.0 : 1.0);
    o[1] = lo; o[2] = lo_j != kNone ? (double)lo_j : -1.0;
    o[3] = hi; o[4] = hi_j != kNone ? (double)hi_j : -1.0; o[5] = hi_j != kNone ? hi_t : -1.0;
    o[6] = unsafe ? vt : -1.0;
    o[7] = (double)unsafe; o[8] = (double)undecided; o[9] = (double)boxed;
  }
  if (lane < GTOP_SEPCERT_PAIR) {
    const double diag[GTOP_SEPCERT_PAIR] = {1.0, INFINITY, INFINITY, -1.0, -1.0, 0.0, 0.0, 0.0};
    double v = diag[0];
#pragma unroll
    for (int q = 1; q < GTOP_SEPCERT_PAIR; ++q) v = lane == q ? diag[q] : v;
    pairs[((size_t)i * B + i) * GTOP_SEPCERT_PAIR + lane] = v;
  }
}

}  // namespace

static_assert(GTOP_SEPCERT_PAIR == 8 && GTOP_SEPCERT_ROW == 10, "the kernels write eight and ten entries");

size_t gtop_sepcert_work_bytes(int B) { return B <= 0 ? 0 : (size_t)B * 6 * sizeof(double); }

hipError_t gtop_launch_certify_separation(int B, int m, const double *coeff, const double *T, int t_stride,
                                          const double *t0, int t0_stride, double min_sep, double t_lo, double t_hi,
                                          int max_depth, int max_refine, int hold_ends, int cull, double *pairs,
                                          double *rows, void *work, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  double *box = static_cast<double *>(work);
  hipError_t e;
  if (cull) {
    hipLaunchKernelGGL(sepcert_boxes_kernel, dim3(B), dim3(64), 0, stream, B, m, coeff, T, t_stride, box);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (B > 1) {
    const SepCertParams P = {min_sep, t_lo, t_hi, max_depth, max_refine, hold_ends, cull};
    hipLaunchKernelGGL(sepcert_pairs_kernel, dim3(B * (B - 1) / 2), dim3(64), 0, stream, P, B, m, coeff, T, t_stride, t0,
                       t0_stride, box, pairs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(sepcert_rows_kernel, dim3(B), dim3(64), 0, stream, B, pairs, rows);
  return hipGetLastError();
}
