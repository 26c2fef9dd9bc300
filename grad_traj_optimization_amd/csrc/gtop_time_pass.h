// gtop_time_pass.h — the ONE pass over a trajectory that gives the cost and its derivative with respect to every
// segment time, and the row loop of the time optimizer built on it: shared by the static kernels (gtop_time.hip,
// include/gtop_time.h) and the kernels under the moving-obstacle cost (gtop_time_moving.hip,
// include/gtop_time_moving.h).  DESIGN.md §5.21, §5.23.
//
// With the waypoint values held in x and Df, the polynomial of segment s depends on T_s alone: its own derivative is a
// sum over the segment's own 30 samples plus the closed-form derivative of its jerk integral.  One WAVEFRONT per
// trajectory, several per workgroup.  The lanes run over (segment of a pair, sample): lanes 0 .. 29 the samples of
// segment 2p, lanes 32 .. 61 those of segment 2p + 1, so that a segment's sums stay inside one 32-lane half and are
// taken by a fixed xor butterfly — a row's bits do not depend on B or on its place.  Pairs are walked in order; an odd m
// leaves the upper half idle in the last pass.  The lookups read the corner records (gtop_edt_lookup.h).  The
// coefficients are recomputed from x, Df and T in every pass: nothing per sample or per iteration is written to HBM.
//
// MOV (a template argument: without it every line it adds is compiled out and the pass is the static one): every sample is looked
// up at its absolute time tau = tau_s + t_i, tau_s = ((t0 + T_0) + ...) + T_{s-1} carried along the pair walk in the
// evaluation's own order, against the boxes staged in LDS; beside the 8 corner values the box loop tracks their 8
// derivatives with respect to tau (gtop_edt_box_min_dtau).  T_s then also moves every LATER segment: q_s, what the
// segment's cost gains per second of delay of its start, goes to LDS and is summed from the last segment to the first.
//
// GX (a template argument, as MOV: without it every line it adds is compiled out): the pass also leaves the derivative
// with respect to every free waypoint value (gtop_joint.hip, include/gtop_joint.h).  The coefficients
// are linear in a segment's six end values per axis, so a sample adds Wp h_j + Wv h_j' + Wa h_j'' to entry j of axis k:
// 18 values per sample, summed over the half by time_half_sum's butterfly taken for all 18 at once (time_half_spread18:
// a lane keeps only its share of the values at every level, 20 shuffles for 90, and ends with ONE complete sum).  The
// lane adds the jerk term of its entry; an interior waypoint gets the end part of the segment before it plus the start
// part of the segment behind it: across the halves of a pair by one shuffle, across pairs by one carried value per lane —
// no LDS, no global traffic but the one store per entry.
#ifndef GTOP_TIME_PASS_H_
#define GTOP_TIME_PASS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_device_common.h"
#include "gtop_edt_lookup.h"
#include "gtop_kernels.h"

constexpr int kTimeWaves = 4;   // wavefronts (trajectories) per workgroup

struct TimeParams {
  GtopGrid g;
  const double *rec;   // the fp64 corner records
  double ws, wc;       // ws: 0 at step 1 already
  double alpha, d0, inv_r, alpha_over_r;
  double alpha_v, v0, inv_r_v, alpha_a, a0, inv_r_a;
  int colli, dyn;      // |wc| >= 1e-4; enable_dyn at step 2
};

// What a MOV pass reads and leaves beside that (unused without MOV).  The pass needs g_out in this wavefront's LDS too.
struct TimeMoving {
  const double *bx;   // LDS: the box rows as stage_boxes<POLY> lays them, [nbox][kBoxRowOf<POLY>]
  int nbox;
  double tau0;        // the row's start time on the boxes' clock
  double *q;          // LDS, this wavefront's: q_s [m]
  double gt0;         // out: d cost / d t0 = R_0 + q_0
};

// this wavefront's own LDS writes, before its own LDS reads (one wavefront's LDS operations execute in order)
__device__ __forceinline__ void time_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum over the 32 lanes of a half, in every lane of it; the order is the butterfly's, whatever the row
__device__ __forceinline__ double time_half_sum(double v) {
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double time_wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// time_half_sum of 18 values at once.  The same butterfly level by level (xor 16, 8, 4, 2, 1: the same pairs in the same
// order, so the same bits), but at every level a lane keeps the lower or the upper share of its values by its bit of that
// level and trades the other share for its partner's: 9 + 5 + 3 + 2 + 1 shuffles.  Lane i of the half ends with the
// complete sum of ONE value — or of a pad: 18 of the 32 lanes hold a value.  SUM = false: no shuffle and no addition, the
// lane's pick of v (of a table, or of the values' own indices: which value the lane ends with; pad for none).
template <bool SUM, typename V>
__device__ __forceinline__ V time_half_spread18(const V (&v)[18], int i, V pad) {
  V a[9], b[5], c[3], d[2];
  bool up = (i & 16) != 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const V keep = up ? v[k + 9] : v[k], send = up ? v[k] : v[k + 9];
    if constexpr (SUM) a[k] = keep + __shfl_xor(send, 16); else a[k] = keep;
  }
  up = (i & 8) != 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const V hi = k + 5 < 9 ? a[k + 5 < 9 ? k + 5 : 0] : pad;
    const V keep = up ? hi : a[k], send = up ? a[k] : hi;
    if constexpr (SUM) b[k] = keep + __shfl_xor(send, 8); else b[k] = keep;
  }
  up = (i & 4) != 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const V hi = k + 3 < 5 ? b[k + 3 < 5 ? k + 3 : 0] : pad;
    const V keep = up ? hi : b[k], send = up ? b[k] : hi;
    if constexpr (SUM) c[k] = keep + __shfl_xor(send, 4); else c[k] = keep;
  }
  up = (i & 2) != 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const V hi = k + 2 < 3 ? c[k + 2 < 3 ? k + 2 : 0] : pad;
    const V keep = up ? hi : c[k], send = up ? c[k] : hi;
    if constexpr (SUM) d[k] = keep + __shfl_xor(send, 2); else d[k] = keep;
  }
  up = (i & 1) != 0;
  const V keep = up ? d[1] : d[0], send = up ? d[0] : d[1];
  if constexpr (SUM) return keep + __shfl_xor(send, 1); else return keep;
}

// One pass over the trajectory at segment times Ts (global memory or LDS): g_out[s] = d cost / d T_s + g_add, parts
// (may be NULL) [m][NP]; returns the cost (its 1e-3 included), the same value in every lane.  NP = GTOP_TIME_PARTS, or
// GTOP_TIME_MOVING_PARTS with [4] = q_s and [5] = R_s behind the four (both 0 without MOV).
// GX: gx (3 (3m - 3) doubles, laid out as xb) gets d cost / d xb, every entry written once, by the lane that holds it.
template <bool MOV, bool POLY, int NP, bool GX = false>
__device__ __forceinline__ double time_pass(const TimeParams &P, TimeMoving &M, int m, int lane,
                                            const double *__restrict__ xb, const double *__restrict__ dfb,
                                            const double *Ts, double g_add, double *g_out, double *parts,
                                            [[maybe_unused]] double *gx = nullptr) {
  const int half = lane >> 5, i = lane & 31;
  const int ndp = 3 * m - 3;
  const double fr = (double)i / 30.0;   // d t_i / d T
  double cost = 0.0;
  [[maybe_unused]] double carry = 0.0;   // MOV: the start of segment s0 on the boxes' clock
  if constexpr (MOV) carry = M.tau0;
  // GX: the 18 entries of a segment are numbered part * 9 + axis * 3 + (0 position, 1 velocity, 2 acceleration); part 0
  // is the END part in the lower half and the START part in the upper half, part 1 the other: the two lanes of a pair that
  // hold the two parts of one waypoint's entry then sit 32 apart.  slot: the entry this lane ends with (-1: none).
  [[maybe_unused]] int slot = -1;
  [[maybe_unused]] double end_carry = 0.0;   // the upper half's end part of this lane's entry, for the next pair
  if constexpr (GX) {
    int ids[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) ids[q] = q;
    slot = time_half_spread18<false>(ids, i, -1);
  }
  for (int s0 = 0; s0 < m; s0 += 2) {
    const int sq = s0 + half;
    const bool seg_ok = sq < m;
    const int s = seg_ok ? sq : m - 1;   // (an idle half repeats the last segment: its loads stay in bounds, nothing is written)
    const double T = Ts[s];
    [[maybe_unused]] double tau_s = 0.0;
    if constexpr (MOV) {   // start(2p) = carry, start(2p + 1) = carry + T[2p]: the evaluation's left-to-right sum
      const double T_even = Ts[s0], T_odd = s0 + 1 < m ? Ts[s0 + 1] : 0.0;
      const double mid = carry + T_even;
      tau_s = half ? mid : carry;
      carry = mid + T_odd;
    }
    // derivative vector layout (src/qp_generator.cpp:363-387): start | end | waypoint 1 | ... | waypoint m-1
    const bool first = s == 0, last = s + 1 == m;
    const double *p0 = first ? dfb : xb + 3 * (s - 1);
    const double *p1 = last ? dfb + 3 : xb + 3 * s;
    const int st0 = first ? 6 : ndp, st1 = last ? 6 : ndp;
    // ---- coefficients c = A_s^-1 d and c' = d c / d T (rows of A_s: src/qp_generator.cpp:185-195) ----
    const double T2 = T * T, T3 = T2 * T, T4 = T2 * T2, T5 = T4 * T;
    const double iT = 1.0 / T, iT3 = iT * iT * iT, iT4 = iT3 * iT, iT5 = iT4 * iT;
    double c[3][6], d[3][3];   // d[k][j - 3] = c_j'
    double jc = 0.0, jd = 0.0;
    [[maybe_unused]] double jq[3][3] = {};   // GX: per axis 2 ws (q3, q4, q5), the jerk term's chain
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double a0 = p0[k * st0 + 2], v0 = p0[k * st0 + 1], q0 = p0[k * st0];
      const double aT = p1[k * st1 + 2], vT = p1[k * st1 + 1], qT = p1[k * st1];
      const double Pp = qT - q0 - v0 * T - 0.5 * a0 * T2, dP = -v0 - a0 * T;
      const double Vv = (vT - v0 - a0 * T) * T, dV = vT - v0 - 2.0 * a0 * T;
      const double Aa = (aT - a0) * T2, dA = 2.0 * (aT - a0) * T;
      c[k][0] = q0; c[k][1] = v0; c[k][2] = 0.5 * a0;
      c[k][3] = (10.0 * Pp - 4.0 * Vv + 0.5 * Aa) * iT3;
      c[k][4] = (7.0 * Vv - 15.0 * Pp - Aa) * iT4;
      c[k][5] = (6.0 * Pp - 3.0 * Vv + 0.5 * Aa) * iT5;
      d[k][0] = (10.0 * dP - 4.0 * dV + 0.5 * dA) * iT3 - 3.0 * c[k][3] * iT;
      d[k][1] = (7.0 * dV - 15.0 * dP - dA) * iT4 - 4.0 * c[k][4] * iT;
      d[k][2] = (6.0 * dP - 3.0 * dV + 0.5 * dA) * iT5 - 5.0 * c[k][5] * iT;
      // the jerk term (Jerk Hessian Q_s: src/qp_generator.cpp:226-234): c'Qc, its explicit d/dT and 2 (Qc) . c'
      const double c3 = c[k][3], c4 = c[k][4], c5 = c[k][5];
      const double q3 = 36.0 * T * c3 + 72.0 * T2 * c4 + 120.0 * T3 * c5;
      const double q4 = 72.0 * T2 * c3 + 192.0 * T3 * c4 + 360.0 * T4 * c5;
      const double q5 = 120.0 * T3 * c3 + 360.0 * T4 * c4 + 720.0 * T5 * c5;
      jc += c3 * q3 + c4 * q4 + c5 * q5;
      jd += 36.0 * c3 * c3 + 288.0 * T * c3 * c4 + 720.0 * T2 * c3 * c5 + 576.0 * T2 * c4 * c4 +
            2880.0 * T3 * c4 * c5 + 3600.0 * T4 * c5 * c5;
      jd += 2.0 * (q3 * d[k][0] + q4 * d[k][1] + q5 * d[k][2]);
      if constexpr (GX) {
        jq[k][0] = P.ws * (2.0 * q3);
        jq[k][1] = P.ws * (2.0 * q4);
        jq[k][2] = P.ws * (2.0 * q5);
      }
    }
    const double smooth = P.ws * jc, dsmooth = P.ws * jd;   // (every lane of the half holds the same two values)
    // GX: the table d c_n / d (end value), n = 3, 4, 5, in this half's entry order e = part * 3 + (0, 1, 2): the lower
    // half has (pT, vT, aT | p0, v0, a0), the upper (p0, v0, a0 | pT, vT, aT); is_start[part]: 1.0 where c0, c1, c2 move
    [[maybe_unused]] double A3[6], A4[6], A5[6], is_start[2] = {};
    [[maybe_unused]] double gsum = 0.0;   // the half's sum of this lane's entry over the samples
    if constexpr (GX) {
      const double iT2 = iT * iT;
      const double s3[3] = {-10.0 * iT3, -6.0 * iT2, -1.5 * iT}, e3[3] = {10.0 * iT3, -4.0 * iT2, 0.5 * iT};
      const double s4[3] = {15.0 * iT4, 8.0 * iT3, 1.5 * iT2}, e4[3] = {-15.0 * iT4, 7.0 * iT3, -iT2};
      const double s5[3] = {-6.0 * iT5, -3.0 * iT4, -0.5 * iT3}, e5[3] = {6.0 * iT5, -3.0 * iT4, 0.5 * iT3};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        A3[j] = half ? s3[j] : e3[j]; A3[j + 3] = half ? e3[j] : s3[j];
        A4[j] = half ? s4[j] : e4[j]; A4[j + 3] = half ? e4[j] : s4[j];
        A5[j] = half ? s5[j] : e5[j]; A5[j + 3] = half ? e5[j] : s5[j];
      }
      is_start[0] = half ? 1.0 : 0.0;
      is_start[1] = half ? 0.0 : 1.0;
    }

    // ---- the segment's samples (src/grad_traj_optimizer.cpp:345-409): lane i is sample i ----
    double cs = 0.0, ds = 0.0;
    [[maybe_unused]] double qs = 0.0;
    if (P.colli) {
      // t_i = 1e-3 + i dt (:353); a segment with T < 0.0301, where the sample COUNT hangs on the accumulated value,
      // replays the reference's addition chain
      double dt = T * (1.0 / 30.0);
      double t = (double)i * dt + 1e-3;
      bool live = i < 30;
      if (T < 0.0301) {
        dt = T / 30.0;
        t = 1e-3;
        for (int j = 0; j < i && j < 30; ++j) t += dt;
        live = live && t < T;
      }
      // (a sample past the loop bound is evaluated at the first sample's time, with weight 0: no extrapolated polynomial)
      if (!live) t = 1e-3;
      const double fri = live ? fr : 0.0;
      const double t2 = t * t, t3 = t2 * t, t4 = t2 * t2, t5 = t4 * t;
      double pos[3], vel[3], acc[3], pd[3], vd[3], ad[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double *q = c[k], *e = d[k];
        // the reference's float locals (:457-465, :477-485, :491-505)
        pos[k] = (double)(float)(q[0] + q[1] * t + q[2] * t2 + q[3] * t3 + q[4] * t4 + q[5] * t5);
        vel[k] = (double)(float)(q[1] + 2.0 * q[2] * t + 3.0 * q[3] * t2 + 4.0 * q[4] * t3 + 5.0 * q[5] * t4);
        acc[k] = (double)(float)(2.0 * q[2] + 6.0 * q[3] * t + 12.0 * q[4] * t2 + 20.0 * q[5] * t3);
        const double jerk = 6.0 * q[3] + 24.0 * q[4] * t + 60.0 * q[5] * t2;
        pd[k] = e[0] * t3 + e[1] * t4 + e[2] * t5 + vel[k] * fri;
        vd[k] = 3.0 * e[0] * t2 + 4.0 * e[1] * t3 + 5.0 * e[2] * t4 + acc[k] * fri;
        ad[k] = 6.0 * e[0] * t + 12.0 * e[1] * t2 + 20.0 * e[2] * t3 + jerk * fri;
      }
      const double vn = sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) + 1e-5;   // :358
      const double vdot = (vel[0] * vd[0] + vel[1] * vd[1] + vel[2] * vd[2]) / vn;          // d vn / d T
      // SDFMap::getDistWithGradTrilinear (:363): the cell from the float position, in double; out of the map dist = -1
      // and the gradient 0 (sdf_map.cpp:187)
      int idx[3];
      double diff[3], values[2][2][2], grad[3];
      gtop_edt_corners(P.g, P.rec, pos, idx, diff, values);
      [[maybe_unused]] double dtau = 0.0;   // MOV: d dist / d tau
      if constexpr (MOV) {
        // evaluateEDTWithGrad(pos, tau): the 8 corners min'ed with the boxes at the sample's absolute time, static only
        // for tau < 0 and out of the map (edt_environment.cpp:91-98), and the corners' derivatives beside them
        constexpr int ROW = kBoxRowOf<POLY>;
        const double tau = tau_s + t;
        const bool out = gtop_edt_out_of_map(P.g, pos);
        double dvals[2][2][2] = {};
        if (!out && tau >= 0.0) {
          double vmax = gtop_edt_vmax(values);
#pragma unroll 1
          for (int q = 0; q < M.nbox; ++q) {
            double bmin[3], bmax[3], cv[3];
            gtop_edt_box_faces_of<POLY>(M.bx + q * ROW, tau, bmin, bmax);
            gtop_edt_box_velocity_of<POLY>(M.bx + q * ROW, tau, cv);
            gtop_edt_box_min_dtau(P.g, bmin, bmax, cv, idx, values, dvals, vmax);
          }
        }
        dtau = out ? 0.0 : gtop_edt_trilinear(diff, dvals).d;
      }
      const GtopTrilinear tl = gtop_edt_trilinear(diff, values);
      gtop_edt_gradient(P.g, diff, values, tl, grad);
      double dist = tl.d;
      if (gtop_edt_out_of_map(P.g, pos)) {
        dist = -1.0;
        grad[0] = grad[1] = grad[2] = 0.0;
      }
      const double e = exp((P.d0 - dist) * P.inv_r);
      const double cd = P.alpha * e, gd = -P.alpha_over_r * e;   // :509, :514
      const double gp = grad[0] * pd[0] + grad[1] * pd[1] + grad[2] * pd[2];
      cs = P.wc * (cd * vn * dt);                                                            // :373, weighted as :417
      ds = P.wc * (gd * gp * vn * dt + cd * vdot * dt + cd * vn * (1.0 / 30.0));
      if (P.dyn) {   // the block of :383-407 with the formulas of :517-535
        double S = 0.0, dS = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double cv = P.alpha_v * exp((fabs(vel[k]) - P.v0) * P.inv_r_v);
          const double ca = P.alpha_a * exp((fabs(acc[k]) - P.a0) * P.inv_r_a);
          const double sv = (double)((vel[k] > 0.0) - (vel[k] < 0.0)), sa = (double)((acc[k] > 0.0) - (acc[k] < 0.0));
          S += cv + ca;
          dS += cv * P.inv_r_v * sv * vd[k] + ca * P.inv_r_a * sa * ad[k];
        }
        cs += S * vn * dt;
        ds += dS * vn * dt + S * vdot * dt + S * vn * (1.0 / 30.0);
      }
      if constexpr (MOV) {
        // the lookup's own clock: the sample's time moves by i / 30 per second of T_s (the dyn block does not depend on
        // tau); added behind the static expression, so that a zero dtau leaves its bits
        const double w = P.wc * (gd * dtau * vn * dt);
        ds += w * fri;
        qs = live ? w : 0.0;
        qs = time_half_sum(qs);
      }
      if constexpr (GX) {
        // h_e = d pos / d (entry e), h_e' = d vel / d e, h_e'' = d acc / d e at t: the table's polynomials, plus
        // 1, t, t^2 / 2 (and their derivatives) where the entry is a start value
        double h[6], h1[6], h2[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) {
          const int j = e % 3;
          const double st = is_start[e / 3];
          const double b0 = j == 0 ? 1.0 : (j == 1 ? t : 0.5 * t2), b1 = j == 0 ? 0.0 : (j == 1 ? 1.0 : t);
          const double b2 = j == 2 ? 1.0 : 0.0;
          h[e] = (A3[e] * t3 + A4[e] * t4 + A5[e] * t5) + st * b0;
          h1[e] = (3.0 * A3[e] * t2 + 4.0 * A4[e] * t3 + 5.0 * A5[e] * t4) + st * b1;
          h2[e] = (6.0 * A3[e] * t + 12.0 * A4[e] * t2 + 20.0 * A5[e] * t3) + st * b2;
        }
        // the weights of d pos_k, d vel_k, d acc_k in the sample's cost: the consistent gradient's terms (gtop.h)
        const double cdv = P.wc * (cd * dt), gw = P.wc * (gd * vn * dt);
        double Sdyn = 0.0;
        if (P.dyn) {
#pragma unroll
          for (int k = 0; k < 3; ++k)
            Sdyn += P.alpha_v * exp((fabs(vel[k]) - P.v0) * P.inv_r_v) + P.alpha_a * exp((fabs(acc[k]) - P.a0) * P.inv_r_a);
        }
        double v18[18];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double vk = vel[k] / vn;
          double wp = gw * grad[k], wv = cdv * vk, wa = 0.0;
          if (P.dyn) {
            const double cv = P.alpha_v * exp((fabs(vel[k]) - P.v0) * P.inv_r_v);
            const double ca = P.alpha_a * exp((fabs(acc[k]) - P.a0) * P.inv_r_a);
            const double sv = (double)((vel[k] > 0.0) - (vel[k] < 0.0)), sa = (double)((acc[k] > 0.0) - (acc[k] < 0.0));
            wv += cv * P.inv_r_v * sv * vn * dt + Sdyn * vk * dt;
            wa = ca * P.inv_r_a * sa * vn * dt;
          }
          wp = live ? wp : 0.0;
          wv = live ? wv : 0.0;
          wa = live ? wa : 0.0;
#pragma unroll
          for (int e = 0; e < 6; ++e) v18[(e / 3) * 9 + k * 3 + e % 3] = wp * h[e] + wv * h1[e] + wa * h2[e];
        }
        gsum = time_half_spread18<true>(v18, i, 0.0);
      }
      cs = live ? cs : 0.0;   // (past the loop bound, and the two idle lanes of a half: nothing reaches the sums)
      ds = live ? ds : 0.0;
      cs = time_half_sum(cs);
      ds = time_half_sum(ds);
    }
    if (seg_ok && i == 0) {
      if constexpr (MOV) {   // (the later segments' term and g_add are added once every q_s is known)
        g_out[s] = dsmooth + ds;
        M.q[s] = qs;
      } else {
        g_out[s] = (dsmooth + ds) + g_add;
      }
      if (parts) {
        double *o = parts + (size_t)s * NP;
        o[0] = smooth; o[1] = cs; o[2] = dsmooth; o[3] = ds;
        if constexpr (NP > 4) {
          o[4] = MOV ? qs : 0.0;
          if constexpr (!MOV) o[5] = 0.0;
        }
      }
    }
    if constexpr (GX) {
      // this lane's entry: the jerk term 2 ws (q3 dc3 + q4 dc4 + q5 dc5) first, the samples' sum second
      const int sl = slot < 0 ? 0 : slot, part = sl / 9, k = (sl % 9) / 3, j = sl % 3, e = part * 3 + j;
      double a3 = A3[0], a4 = A4[0], a5 = A5[0];
#pragma unroll
      for (int q = 1; q < 6; ++q) {
        a3 = e == q ? A3[q] : a3;
        a4 = e == q ? A4[q] : a4;
        a5 = e == q ? A5[q] : a5;
      }
      const double j3 = k == 0 ? jq[0][0] : (k == 1 ? jq[1][0] : jq[2][0]);
      const double j4 = k == 0 ? jq[0][1] : (k == 1 ? jq[1][1] : jq[2][1]);
      const double j5 = k == 0 ? jq[0][2] : (k == 1 ? jq[1][2] : jq[2][2]);
      const double mine = (j3 * a3 + j4 * a4 + j5 * a5) + gsum;
      // part 0: the lower half's end part meets the upper half's start part (waypoint s0 + 1); part 1: the lower half's
      // start part meets the end part carried from the pair before (waypoint s0)
      const double other = __shfl_xor(mine, 32);
      if (half == 0 && slot >= 0) {
        if (part == 0) {
          if (s0 + 1 < m) gx[k * ndp + 3 * s0 + j] = mine + other;
        } else if (s0 > 0) {
          gx[k * ndp + 3 * (s0 - 1) + j] = end_carry + mine;
        }
      }
      end_carry = other;
    }
    // the cost: the segments' two parts in segment order, by every lane alike
    const double seg_cost = smooth + cs;
    const double c_lo = __shfl(seg_cost, 0), c_hi = __shfl(seg_cost, 32);
    cost += c_lo;
    if (s0 + 1 < m) cost += c_hi;
  }
  if constexpr (MOV) {
    // R_{m-1} = 0, R_s = R_{s+1} + q_{s+1}, from the last segment to the first: gT_s = (own + R_s) + g_add
    time_wave_sync();
    double R = 0.0;
    for (int s = m - 1; s >= 0; --s) {
      const double q = M.q[s];
      if (lane == 0) {
        g_out[s] = (g_out[s] + R) + g_add;
        if (parts) parts[(size_t)s * NP + 5] = R;
      }
      R += q;
    }
    M.gt0 = R;   // R_0 + q_0
  }
  return cost + 1e-3;   // :417-418
}

struct TimeOpt {
  double rho, t_min, t_max, first_move, ftol_rel, xtol_abs;
  int max_evals;
};

// lo_s = max(t_min, T_lo[s]); lo_s > t_max pins the segment at lo_s
__device__ __forceinline__ double time_clamp(const TimeOpt &O, const double *lo_row, int s, double v) {
  const double lo = lo_row ? fmax(O.t_min, lo_row[s]) : O.t_min;
  return lo > O.t_max ? lo : fmin(fmax(v, lo), O.t_max);
}

// The optimizer's loop on one row, by its wavefront (include/gtop_time.h states the rule).  lds: this wavefront's
// T | g | T' | g', m doubles each; T_out [B][m] and info [B][8] are the batch's, b the row.
template <bool MOV, bool POLY>
__device__ __forceinline__ void time_optimize_row(const TimeParams &P, TimeMoving &M, const TimeOpt &O, int b, int m, int lane,
                                                  const double *__restrict__ xb, const double *__restrict__ dfb,
                                                  const double *__restrict__ Tin, const double *__restrict__ lo_row,
                                                  double *lds, double *__restrict__ T_out, double *__restrict__ info) {
  double *Tc = lds, *gc = Tc + m, *Tp = gc + m, *gp = Tp + m;

  double tsum = 0.0;
  for (int s = lane; s < m; s += 64) {
    const double v = time_clamp(O, lo_row, s, Tin[s]);
    Tc[s] = v;
    tsum += v;
  }
  tsum = gtop_wave_sum(tsum);
  time_wave_sync();
  double cost = time_pass<MOV, POLY, 4>(P, M, m, lane, xb, dfb, Tc, O.rho, gc, nullptr);
  time_wave_sync();
  double F = cost + O.rho * tsum;
  const double F0 = F;
  int evals = 1, accepted = 0, code = GTOP_MMA_XTOL_REACHED;
  double gmax = 0.0;
  for (int s = lane; s < m; s += 64) gmax = fmax(gmax, fabs(gc[s]));
  gmax = time_wave_max(gmax);
  if (gmax > 0.0) {
    double a = O.first_move / gmax;
    for (;;) {
      int backtracks = 0;
      double Fp = 0.0, costp = 0.0, tsump = 0.0;
      bool stop = false;
      for (;;) {
        double dmax = 0.0, slope = 0.0;
        tsump = 0.0;
        for (int s = lane; s < m; s += 64) {
          const double told = Tc[s], g = gc[s];
          const double tn = time_clamp(O, lo_row, s, told - a * g);
          const double dd = tn - told;
          Tp[s] = tn;
          tsump += tn;
          dmax = fmax(dmax, fabs(dd));
          slope += g * dd;
        }
        dmax = time_wave_max(dmax);
        slope = gtop_wave_sum(slope);
        tsump = gtop_wave_sum(tsump);
        if (dmax <= O.xtol_abs) { code = GTOP_MMA_XTOL_REACHED; stop = true; break; }
        if (evals >= O.max_evals) { code = GTOP_MMA_MAXEVAL_REACHED; stop = true; break; }
        time_wave_sync();
        costp = time_pass<MOV, POLY, 4>(P, M, m, lane, xb, dfb, Tp, O.rho, gp, nullptr);
        time_wave_sync();
        Fp = costp + O.rho * tsump;
        ++evals;
        if (Fp <= F + 1e-4 * slope) break;   // (a NaN F' is a rejection)
        a *= 0.5;
        ++backtracks;
      }
      if (stop) break;
      const double decrease = F - Fp;
      double *t0 = Tc; Tc = Tp; Tp = t0;
      double *t1 = gc; gc = gp; gp = t1;
      F = Fp; cost = costp; tsum = tsump;
      ++accepted;
      if (decrease <= O.ftol_rel * fabs(F)) { code = GTOP_MMA_FTOL_REACHED; break; }
      if (backtracks == 0) a *= 2.0;
    }
  }
  // the row's results: T_out, and the largest |g| among the segments their gradient does not hold at a bound
  double gfree = 0.0;
  for (int s = lane; s < m; s += 64) {
    const double v = Tc[s], g = gc[s];
    const double lo = lo_row ? fmax(O.t_min, lo_row[s]) : O.t_min;
    const bool held = lo > O.t_max || (v <= lo && g > 0.0) || (v >= O.t_max && g < 0.0);
    if (!held) gfree = fmax(gfree, fabs(g));
    T_out[(size_t)b * m + s] = v;
  }
  gfree = time_wave_max(gfree);
  if (lane == 0) {
    double *o = info + (size_t)b * 8;
    o[0] = (double)code; o[1] = (double)accepted; o[2] = (double)evals; o[3] = F0;
    o[4] = F; o[5] = cost; o[6] = gfree; o[7] = tsum;
  }
}

inline TimeParams time_params(const GtopGrid &g, const double *rec, const GtopTimeCost &p) {
  TimeParams P;
  P.g = g;
  P.rec = rec;
  P.ws = p.step == 1 ? 0.0 : p.ws;   // :412-415
  P.wc = p.wc;
  P.alpha = p.alpha; P.d0 = p.d0; P.inv_r = 1.0 / p.r; P.alpha_over_r = p.alpha / p.r;
  P.alpha_v = p.alpha_v; P.v0 = p.v0; P.inv_r_v = p.r_v != 0.0 ? 1.0 / p.r_v : 0.0;
  P.alpha_a = p.alpha_a; P.a0 = p.a0; P.inv_r_a = p.r_a != 0.0 ? 1.0 / p.r_a : 0.0;
  P.colli = !(fabs(p.wc) < 1e-4);   // :346
  P.dyn = p.enable_dyn && p.step == 2;   // :383
  return P;
}

#endif  // GTOP_TIME_PASS_H_
