// gtop_swarm.hip — the swarm separation cost and its gradient, on gfx950, fp64 (include/gtop_swarm.h,
// gtop_swarm_gradient_device and the rounds of gtop_optimize_swarm_device).
//
// Rows that come closer than a radius on the common clock pay a cubic hinge in the squared distance.  O(B² · samples),
// cut in three on the caller's stream:
//   (1) sep_sample_kernel   (gtop_sep_sample.h, shared with gtop_separation.hip) the trial rows — and the frozen rows,
//                           where the partners are another set — sampled on the grid into the workspace;
//   (2) swarm_pairs_kernel  the hot one: a wavefront holds 64 trial rows in its lanes for a chunk of samples and walks
//                           ALL partner rows in ascending order, the partners in scalar registers;
//   (3) swarm_rows_kernel   a wavefront per row: S_b, active_b, the per-segment moments G_n of the forces, the closed-form
//                           map d c / d q, the scatter into the layout of x — written, or added to a cost and gradient.
// and swarm_joint_kernel, which packs the closing joint evaluation of the optimizer.
//
// The workspace (private), doubles first: pos of the trial rows and pos of the frozen rows [npad][3][Bpad] each (the
// layout of gtop_sep_sample.h), acc [npad][4][Bpad] (C, Fx, Fy, Fz of sample k, row b at (k 4 + q) Bpad + b), the
// coefficient scratch of the optimizer's rounds [B][m][18], S of the joint evaluation [Bpad]; then int32: cnt
// [npad][Bpad], first / last of both sides [4][Bpad].

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_kernels.h"

// Every step is ONE rounded fp64 operation in the order the header writes it: a numpy restatement reproduces the bits
// (tests/swarm_twin.py).
#pragma clang fp contract(off)

#include "gtop_report_common.h"   // segment_of, poly_eval
#include "gtop_sep_sample.h"      // the grid, sep_sample_kernel and the position layout

namespace {

constexpr int kSwarmJ = 8;        // partners per scalar fetch: one 64-byte line per sample and axis
constexpr int kSwarmChunk = 4;    // grid samples per wavefront of the pair kernel: divides the workspace's padding, and
                                  // B = 1 024 rows on 256 samples are 1 024 wavefronts — one per SIMD of the device
static_assert(kSepChunk % kSwarmChunk == 0, "the padded samples are whole chunks");
constexpr int kSwarmMaxM = 227;   // the rows kernel's moments live in LDS: 18 doubles per segment

// ---- (2) pairs ----
// Block (tile, chunk): one wavefront, lane l holds trial row tile 64 + l at the chunk's kSwarmChunk samples
// and its 4 x kSwarmChunk running sums plus the counts over the WHOLE walk of the partners j = 0 .. Bpad-1,
// ascending — the order the header fixes.  The partners' addresses are wave-uniform, so they arrive through the scalar
// cache kSwarmJ rows at a time and enter the arithmetic as scalar operands; no LDS, no barrier.  Per pair and sample the
// distance and the hinge cost ten fp64 instructions; the force arithmetic behind them runs only where some lane of the
// wavefront has an active term among the kSwarmJ partners (a skipped term is exactly +0, so the skip changes no bit).
// The diagonal (and a row's own frozen copy) is left out by the select that forms `act`.  A padding row, a padding sample
// and a row not flown hold NaN: e is NaN, which is not active.  One coalesced store per (sample, figure) at the end.
__global__ void __launch_bounds__(64)
swarm_pairs_kernel(int Bpad, double R2, const double *__restrict__ pos_i, const double *__restrict__ pos_j,
                   double *__restrict__ acc, int *__restrict__ cnt) {
  const int lane = threadIdx.x, gi = blockIdx.x * kSepTile + lane, k0 = blockIdx.y * kSwarmChunk;
  double xi[kSwarmChunk], yi[kSwarmChunk], zi[kSwarmChunk];
  double C[kSwarmChunk], Fx[kSwarmChunk], Fy[kSwarmChunk], Fz[kSwarmChunk];
  int na[kSwarmChunk];
#pragma unroll
  for (int kk = 0; kk < kSwarmChunk; ++kk) {
    const size_t x = (size_t)(k0 + kk) * 3 * Bpad + gi;
    xi[kk] = pos_i[x]; yi[kk] = pos_i[x + Bpad]; zi[kk] = pos_i[x + 2 * (size_t)Bpad];
    C[kk] = Fx[kk] = Fy[kk] = Fz[kk] = 0.0;
    na[kk] = 0;
  }
  for (int j0 = 0; j0 < Bpad; j0 += kSwarmJ) {   // wave-uniform
    // (one running pointer: 24 offsets held over the walk would not fit the scalar registers)
    const double *pj = pos_j + (size_t)k0 * 3 * Bpad + j0;
#pragma unroll
    for (int kk = 0; kk < kSwarmChunk; ++kk) {
      const double *px = pj, *py = px + Bpad, *pz = py + Bpad;
      pj = pz + Bpad;
      double dx[kSwarmJ], dy[kSwarmJ], dz[kSwarmJ], e[kSwarmJ];
      bool act[kSwarmJ], any = false;
#pragma unroll
      for (int jj = 0; jj < kSwarmJ; ++jj) {
        dx[jj] = xi[kk] - px[jj]; dy[jj] = yi[kk] - py[jj]; dz[jj] = zi[kk] - pz[jj];
        const double d2 = (dx[jj] * dx[jj] + dy[jj] * dy[jj]) + dz[jj] * dz[jj];
        e[jj] = R2 - d2;
        act[jj] = e[jj] > 0.0 && j0 + jj != gi;
        any |= act[jj];
      }
      if (__any(any)) {
#pragma unroll
        for (int jj = 0; jj < kSwarmJ; ++jj) {
          const double e2 = e[jj] * e[jj], e3 = e2 * e[jj];
          const double fx = e2 * dx[jj], fy = e2 * dy[jj], fz = e2 * dz[jj];
          C[kk] += act[jj] ? e3 : 0.0;
          Fx[kk] += act[jj] ? fx : 0.0;
          Fy[kk] += act[jj] ? fy : 0.0;
          Fz[kk] += act[jj] ? fz : 0.0;
          na[kk] += act[jj] ? 1 : 0;
        }
      }
    }
  }
#pragma unroll
  for (int kk = 0; kk < kSwarmChunk; ++kk) {
    const size_t o = (size_t)(k0 + kk) * 4 * Bpad + gi;
    acc[o] = C[kk]; acc[o + Bpad] = Fx[kk]; acc[o + 2 * (size_t)Bpad] = Fy[kk]; acc[o + 3 * (size_t)Bpad] = Fz[kk];
    cnt[(size_t)(k0 + kk) * Bpad + gi] = na[kk];
  }
}

// ---- (3) rows ----
// the local time and the segment of grid sample k of a row, as sep_sample_kernel forms them for a flown sample
__device__ __forceinline__ unsigned swarm_walk(const SepGrid &G, int k, double start, double time_sum, const double *ts,
                                               int m, double &u) {
  u = sep_tau(G, k) - start;
  if (G.hold_ends) u = u < 0.0 ? 0.0 : (u > time_sum ? time_sum : u);
  return segment_of(ts, m, u);
}

// the first k in [lo, hi) whose segment is >= s (the segment is non-decreasing in k: every step of tau_k, of the
// subtractions and of the walk is a monotone rounding); hi if there is none
__device__ __forceinline__ int swarm_first_in(const SepGrid &G, int lo, int hi, unsigned s, double start, double time_sum,
                                              const double *ts, int m) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    double u;
    if (swarm_walk(G, mid, start, time_sum, ts, m, u) >= s) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// the value lane l holds, l wave-uniform: two v_readlane, the result a scalar operand
__device__ __forceinline__ double swarm_lane_value(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// One wavefront per row b.  The sums whose order the header fixes run over k ascending, so they are serial — but what
// they add is not.  S_b: 64 samples at a time are fetched by the lanes, and the chain takes them out of the lanes'
// registers one v_readlane at a time (a lane past the last flown sample holds +0, which adds nothing); active_b is an
// integer sum.  The moments G_n of segment s and axis a: the segments' sample ranges are found first (lanes over the
// segments, a bisection each: the segment is non-decreasing in k); then, kSwarmStage samples at a time, the lanes stage
// the local times and the three forces in LDS (each its own k: the loads and the walks in parallel), and item
// (s, a, n) — a lane each, 64 items a pass — adds F_k u_k^n over the staged samples of ITS segment only, k ascending.
// The moments live in LDS; then lanes over the 9 (m-1) free variables: the closed-form d c / d q of the two segments
// that share the waypoint, the segment before it first.  Every output entry is written (or added to) exactly once.
constexpr int kSwarmStage = 256;

__global__ void __launch_bounds__(64)
swarm_rows_kernel(SepGrid G, double w, int B, int Bpad, int m, const double *__restrict__ T, int t_stride,
                  const double *__restrict__ t0, int t0_stride, const int *__restrict__ first,
                  const int *__restrict__ last, const double *__restrict__ acc, const int *__restrict__ cnt, int add,
                  double *__restrict__ f, double *__restrict__ g, double *__restrict__ active) {
  __shared__ double Gs[kSwarmMaxM * 18];
  __shared__ double su[kSwarmStage], sf[3][kSwarmStage];
  __shared__ int kstart[kSwarmMaxM + 1];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const int kf = first[b], kl = last[b];
  const double *ts = T + (size_t)b * t_stride;
  double time_sum = 0.0;
  for (int s = 0; s < m; ++s) time_sum += ts[s];
  const double start = t0 ? t0[(size_t)b * t0_stride] : 0.0;

  double sum = 0.0;
  int n_act = 0;
  for (int k0 = kf; k0 <= kl; k0 += 64) {   // wave-uniform
    const int k = k0 + lane;
    const double c = k <= kl ? acc[(size_t)k * 4 * Bpad + b] : 0.0;
    n_act += k <= kl ? cnt[(size_t)k * Bpad + b] : 0;
#pragma unroll 8
    for (int kk = 0; kk < 64; ++kk) sum += swarm_lane_value(c, kk);
  }
  for (int off = 32; off > 0; off >>= 1) n_act += __shfl_xor(n_act, off);
  if (lane == 0) {
    const double S = (w * G.dt) * sum;
    f[b] = add ? f[b] + S : S;
    if (active) active[b] = (double)n_act;
  }

  // kstart[s]: the first flown k whose segment is >= s; segment s has the samples kstart[s] .. kstart[s + 1] - 1
  const int items = m * 18, kend = max(kl + 1, kf);
  for (int s = lane; s <= m; s += 64)
    kstart[s] = s == 0 ? kf : s == m ? kend : swarm_first_in(G, kf, kend, (unsigned)s, start, time_sum, ts, m);
  for (int item = lane; item < items; item += 64) Gs[item] = 0.0;
  __syncthreads();
  for (int c0 = kf; c0 < kend; c0 += kSwarmStage) {   // wave-uniform
    const int c1 = min(c0 + kSwarmStage, kend);
    for (int k = c0 + lane; k < c1; k += 64) {
      double u;
      swarm_walk(G, k, start, time_sum, ts, m, u);
      const double *fk = acc + ((size_t)k * 4 + 1) * Bpad + b;
      su[k - c0] = u;
      sf[0][k - c0] = fk[0]; sf[1][k - c0] = fk[Bpad]; sf[2][k - c0] = fk[2 * (size_t)Bpad];
    }
    __syncthreads();
    for (int base = 0; base < items; base += 64) {   // wave-uniform
      const int s_lo = base / 18, s_hi = min((base + 63) / 18, m - 1);
      if (kstart[s_lo] >= c1 || kstart[s_hi + 1] <= c0) continue;   // none of the pass's segments in this stage
      const int item = base + lane;
      if (item < items) {
        const int s = item / 18, r = item - s * 18, a = r / 6, n = r - a * 6;
        const int lo = max(kstart[s], c0), hi = min(kstart[s + 1], c1);
        double Gn = Gs[item];
        for (int k = lo; k < hi; ++k) {
          const double uk = su[k - c0], F = sf[a][k - c0];
          const double u2 = uk * uk, u3 = u2 * uk, u4 = u2 * u2, u5 = u4 * uk;
          const double p = n == 1 ? uk : n == 2 ? u2 : n == 3 ? u3 : n == 4 ? u4 : u5;
          Gn += n == 0 ? F : F * p;
        }
        Gs[item] = Gn;
      }
    }
    __syncthreads();   // the stage may be written again
  }

  const int ndp = 3 * m - 3, nvar = 3 * ndp;
  const double K = (-6.0 * w) * G.dt;
  for (int e = lane; e < nvar; e += 64) {
    const int axis = e / ndp, c = e - axis * ndp, j = c / 3 + 1, q = c - 3 * (j - 1);
    double part[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {   // 0: the end of segment j-1 (pT, vT, aT); 1: the start of segment j
      const int s = side == 0 ? j - 1 : j;
      const double *Gq = Gs + s * 18 + axis * 6;
      const double Ts = ts[s], T2 = Ts * Ts, T3 = T2 * Ts, T4 = T2 * T2, T5 = T4 * Ts;
      double h;
      if (side == 0) {
        if (q == 0) h = (((10.0 / T3) * Gq[3] + (-15.0 / T4) * Gq[4]) + (6.0 / T5) * Gq[5]);
        else if (q == 1) h = (((-4.0 / T2) * Gq[3] + (7.0 / T3) * Gq[4]) + (-3.0 / T4) * Gq[5]);
        else h = (((0.5 / Ts) * Gq[3] + (-1.0 / T2) * Gq[4]) + (0.5 / T3) * Gq[5]);
      } else {
        if (q == 0) h = (((Gq[0] + (-10.0 / T3) * Gq[3]) + (15.0 / T4) * Gq[4]) + (-6.0 / T5) * Gq[5]);
        else if (q == 1) h = (((Gq[1] + (-6.0 / T2) * Gq[3]) + (8.0 / T3) * Gq[4]) + (-3.0 / T4) * Gq[5]);
        else h = (((0.5 * Gq[2] + (-1.5 / Ts) * Gq[3]) + (1.5 / T2) * Gq[4]) + (-0.5 / T3) * Gq[5]);
      }
      part[side] = K * h;
    }
    const double v = part[0] + part[1];
    double *o = g + (size_t)b * nvar + e;
    *o = add ? *o + v : v;
  }
}

// the closing joint evaluation of the optimizer: joint [B][2] = the context's own cost | S (NULL: +0)
__global__ void __launch_bounds__(256)
swarm_joint_kernel(int B, const double *__restrict__ cost, const double *__restrict__ S, double *__restrict__ joint) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  joint[2 * (size_t)b] = cost[b];
  joint[2 * (size_t)b + 1] = S ? S[b] : 0.0;
}

struct SwarmWork {
  double *pos[2], *acc, *coeff, *S;
  int *cnt, *first[2], *last[2];
};

SwarmWork swarm_work(void *work, int B, int m, int n_samples) {
  const size_t Bpad = sep_round_up(B, kSepTile), npad = sep_round_up(n_samples, kSepChunk);
  SwarmWork W;
  W.pos[0] = static_cast<double *>(work);
  W.pos[1] = W.pos[0] + npad * 3 * Bpad;
  W.acc = W.pos[1] + npad * 3 * Bpad;
  W.coeff = W.acc + npad * 4 * Bpad;
  W.S = W.coeff + (size_t)B * m * 18;
  W.cnt = reinterpret_cast<int *>(W.S + Bpad);
  W.first[0] = W.cnt + npad * Bpad;
  W.last[0] = W.first[0] + Bpad;
  W.first[1] = W.last[0] + Bpad;
  W.last[1] = W.first[1] + Bpad;
  return W;
}

}  // namespace

static_assert(kSwarmMaxM * 18 * sizeof(double) <= 64 * 1024, "the moments of a row fit one workgroup's LDS");

size_t gtop_swarm_work_bytes(int B, int m, int n_samples) {
  if (B <= 0) return 0;
  const size_t Bpad = sep_round_up(B, kSepTile), npad = sep_round_up(n_samples, kSepChunk);
  return (npad * 10 * Bpad + (size_t)B * m * 18 + Bpad) * sizeof(double) + (npad * Bpad + 4 * Bpad) * sizeof(int);
}

double *gtop_swarm_coeff_scratch(void *work, int B, int m, int n_samples) { return swarm_work(work, B, m, n_samples).coeff; }
double *gtop_swarm_joint_scratch(void *work, int B, int m, int n_samples) { return swarm_work(work, B, m, n_samples).S; }

hipError_t gtop_launch_swarm_sample(const GtopSwarmGrid &g, int B, int m, const double *coeff, const double *T,
                                    int t_stride, const double *t0, int t0_stride, int side, void *work,
                                    hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const SwarmWork W = swarm_work(work, B, m, g.n_samples);
  const SepGrid G = {g.t_lo, g.dt, g.n_samples, g.hold_ends};
  return sep_launch_sample(G, B, m, coeff, T, t_stride, t0, t0_stride, W.pos[side], W.first[side], W.last[side], stream);
}

hipError_t gtop_launch_swarm_terms(const GtopSwarmGrid &g, double w, double radius, int B, int m, const double *T,
                                   int t_stride, const double *t0, int t0_stride, int partner_side, int add, double *f,
                                   double *grad, double *active, void *work, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const SwarmWork W = swarm_work(work, B, m, g.n_samples);
  const SepGrid G = {g.t_lo, g.dt, g.n_samples, g.hold_ends};
  const int Bpad = sep_round_up(B, kSepTile), npad = sep_round_up(g.n_samples, kSepChunk);
  hipLaunchKernelGGL(swarm_pairs_kernel, dim3(Bpad / kSepTile, npad / kSwarmChunk), dim3(64), 0, stream, Bpad,
                     radius * radius, W.pos[0], W.pos[partner_side], W.acc, W.cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(swarm_rows_kernel, dim3(B), dim3(64), 0, stream, G, w, B, Bpad, m, T, t_stride, t0, t0_stride,
                     W.first[0], W.last[0], W.acc, W.cnt, add, f, grad, active);
  return hipGetLastError();
}

hipError_t gtop_launch_swarm_joint(int B, const double *cost, const double *S, double *joint, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(swarm_joint_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, cost, S, joint);
  return hipGetLastError();
}
