// gtop_separation.hip — PAIRWISE figures of a batch of trajectories, on gfx950, fp64 (include/gtop_separation.h,
// gtop_separation_device and gtop_select_distinct_device).
//
// For every pair of rows the least and the greatest distance between the two curves on a common time grid: the mutual
// clearance of rows that are the robots of a swarm, and the distance by which candidates of one robot are told apart.
// O(B² · samples), so the work is cut in three on the caller's stream:
//   (1) sep_sample_kernel  every row sampled on the grid into the caller's workspace, once;
//   (2) sep_pairs_kernel   the hot one: a workgroup per 64 x 64 tile of pairs, upper-triangular tiles only, one side
//                          in the lanes and the other in scalar registers;
//   (3) sep_rows_kernel    a wavefront per row: the summary from the matrix row and, for the nearest pair, from the
//                          workspace.
// and sep_select_kernel, the greedy selection of distinct candidates over the greatest distances.
//
// The workspace (private): pos [npad][3][Bpad] doubles — sample k, axis a of row b at (k 3 + a) Bpad + b, Bpad = B rounded
// up to the tile edge, npad = n_samples rounded up to the chunk — then first [Bpad] and last [Bpad] int32, the flown
// samples of a row (contiguous in k; first > last: none).  A sample at which a row is NOT flown, a padding row and a
// padding sample hold NaN: the difference to anything is NaN, and fmin / fmax leave a NaN operand out, so the pair
// kernel needs no test per sample and no bound on k or b.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_kernels.h"

// Every step is ONE rounded fp64 operation in the order the header writes it: a numpy restatement reproduces the bits
// (tests/separation_twin.py).
#pragma clang fp contract(off)

#include "gtop_report_common.h"   // segment_of, poly_eval
#include "gtop_sep_sample.h"      // the grid, sep_sample_kernel (1) and the workspace's layout: shared with gtop_swarm.hip

namespace {

constexpr int kSepWaves = 8;     // wavefronts per tile; each takes kSepTile / kSepWaves rows of the broadcast side
constexpr int kSepJ = kSepTile / kSepWaves;
constexpr int kSepMaxB = 4096;   // = GTOP_SEP_MAX_B: the selection's flags live in LDS

// ---- (2) pairs ----
// Tile (ti, tj), tj >= ti, of 64 x 64 pairs; eight wavefronts a tile, each on its own: no LDS, no barrier.  Lane l holds
// row ti 64 + l's position at the sample (three coalesced loads of 512 bytes a wavefront, which the tile's eight
// wavefronts share in the vector cache); wavefront w takes the 8 rows tj 64 + 8 w .. + 7 of the other side, whose
// addresses are wave-uniform, so their positions arrive through the SCALAR cache (one s_load_dwordx16 per sample and
// axis) and enter the arithmetic as scalar operands — a broadcast that costs the vector unit and the LDS nothing.  Per
// pair and sample: 3 subtractions, 3 products, 2 sums, a min and a max — ten fp64 instructions, nothing else; the 16
// running figures of a lane stay in 32 VGPRs, nothing per sample goes to HBM.  The loop is unrolled by the chunk: the
// compiler quiets (v_max x, x) the running figures where it cannot see that they came out of a min or a max, which is
// at the loop's head only (16 instructions per 64 pair-samples), and fetches a sample ahead.
// (Measured against the same tile with both sides staged through LDS, the lane side conflict-free and the other side
// as ds_read_b128 broadcasts: this form is 8 % faster at B = 1 024 and at B = 4 096)
__global__ void __launch_bounds__(kSepTile * kSepWaves)
sep_pairs_kernel(int B, int Bpad, int npad, const double *__restrict__ pos, double *__restrict__ pair_min,
                 double *__restrict__ pair_max) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  // (the wavefront's index as a scalar: what makes the other side's addresses uniform to the compiler)
  const int lane = threadIdx.x & 63, j0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kSepJ;
  double mn[kSepJ], mx[kSepJ];
#pragma unroll
  for (int j = 0; j < kSepJ; ++j) {
    mn[j] = INFINITY;
    mx[j] = -INFINITY;
  }
  const double *pi = pos + ti * kSepTile + lane, *pj = pos + tj * kSepTile + j0;
  for (int k0 = 0; k0 < npad; k0 += kSepChunk) {
#pragma unroll
    for (int kk = 0; kk < kSepChunk; ++kk) {
      const size_t x = (size_t)(k0 + kk) * 3 * Bpad, y = x + Bpad, z = y + Bpad;
      const double xi = pi[x], yi = pi[y], zi = pi[z];
#pragma unroll
      for (int j = 0; j < kSepJ; ++j) {
        const double dx = xi - pj[x + j], dy = yi - pj[y + j], dz = zi - pj[z + j];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        mn[j] = fmin(mn[j], d2);   // a NaN d2 (a row not flown at the sample) is left out of both
        mx[j] = fmax(mx[j], d2);
      }
    }
  }
  const int gi = ti * kSepTile + lane;
#pragma unroll
  for (int j = 0; j < kSepJ; ++j) {
    const int gj = tj * kSepTile + j0 + j;
    if (gi >= B || gj >= B) continue;
    const bool none = gi == gj || mx[j] == -INFINITY;   // the diagonal; no common sample
    const double lo = none ? INFINITY : sqrt(mn[j]), hi = none ? -INFINITY : sqrt(mx[j]);
    pair_min[(size_t)gi * B + gj] = lo;
    pair_max[(size_t)gi * B + gj] = hi;
    if (ti != tj) {   // the mirrored entry (a diagonal tile computes both)
      pair_min[(size_t)gj * B + gi] = lo;
      pair_max[(size_t)gj * B + gi] = hi;
    }
  }
}

// ---- (3) rows ----
// One wavefront per row i.  Lanes over j: the least pair_min (the least j on a tie), the count below the radius, the
// count of rows with a common sample.  Then lanes over the common samples of (i, j*): the earliest k whose d2 is the
// least — the same expression on the same stored positions as the pair kernel's, so equality with its minimum is exact.
__global__ void __launch_bounds__(64)
sep_rows_kernel(SepGrid G, double radius, int B, int Bpad, const double *__restrict__ pos, const int *__restrict__ first,
                const int *__restrict__ last, const double *__restrict__ pair_min, double *__restrict__ rows) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= B) return;
  const int kfi = first[i], kli = last[i];
  double best = INFINITY;
  int bj = 0x7fffffff, near = 0, common = 0;
  for (int j = lane; j < B; j += 64) {   // rising j per lane: `<` keeps the first
    if (j == i) continue;
    const double v = pair_min[(size_t)i * B + j];
    if (v < best) {
      best = v; bj = j;
    }
    near += (radius > 0.0 && v < radius) ? 1 : 0;
    common += max(kfi, first[j]) <= min(kli, last[j]) ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(best, off);
    const int oj = __shfl_xor(bj, off);
    near += __shfl_xor(near, off);
    common += __shfl_xor(common, off);
    if (ov < best || (ov == best && oj < bj)) {
      best = ov; bj = oj;
    }
  }
  const bool have = bj != 0x7fffffff;
  double bd = INFINITY;
  int bk = 0x7fffffff;
  if (have) {   // wave-uniform
    const int lo = max(kfi, first[bj]), hi = min(kli, last[bj]);
    for (int k = lo + lane; k <= hi; k += 64) {   // rising k per lane
      const double *pk = pos + (size_t)k * 3 * Bpad;
      const double dx = pk[i] - pk[bj], dy = pk[Bpad + i] - pk[Bpad + bj],
                   dz = pk[2 * (size_t)Bpad + i] - pk[2 * (size_t)Bpad + bj];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < bd) {
        bd = d2; bk = k;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd, off);
      const int ok = __shfl_xor(bk, off);
      if (od < bd || (od == bd && ok < bk)) {
        bd = od; bk = ok;
      }
    }
  }
  if (lane == 0) {
    double *o = rows + (size_t)i * GTOP_SEP_ROW;
    o[0] = best;
    o[1] = have ? (double)bj : -1.0;
    o[2] = bk != 0x7fffffff ? sep_tau(G, bk) : -1.0;
    o[3] = (double)near;
    o[4] = (double)common;
    o[5] = kli >= kfi ? (double)(kli - kfi + 1) : 0.0;
  }
}

// ---- the greedy selection of distinct candidates ----
// One workgroup.  alive[r]: r is eligible, not chosen, and at least min_gap from every row chosen so far — kept up to
// date by one pass over column c of pair_max after each choice, so a round is one (cost, index) minimum over the rows
// still alive.
constexpr int kSelThreads = 256;

__global__ void __launch_bounds__(kSelThreads)
sep_select_kernel(int B, const unsigned char *__restrict__ pass, const double *__restrict__ cost,
                  const double *__restrict__ pair_max, double min_gap, int K, int *__restrict__ chosen,
                  int *__restrict__ count) {
  __shared__ unsigned char alive[kSepMaxB];
  __shared__ double sc[kSelThreads / 64];
  __shared__ int si[kSelThreads / 64];
  __shared__ int pick;
  const int tid = threadIdx.x;
  for (int r = tid; r < B; r += kSelThreads) alive[r] = (!pass || pass[r] != 0) && isfinite(cost[r]);
  __syncthreads();
  int n = 0;
  for (; n < K; ++n) {
    double c = INFINITY;
    int i = 0x7fffffff;
    for (int r = tid; r < B; r += kSelThreads) {   // rising r per thread: `<` keeps the first
      if (alive[r] && cost[r] < c) {
        c = cost[r]; i = r;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double oc = __shfl_xor(c, off);
      const int oi = __shfl_xor(i, off);
      if (oc < c || (oc == c && oi < i)) {
        c = oc; i = oi;
      }
    }
    if ((tid & 63) == 0) {
      sc[tid >> 6] = c; si[tid >> 6] = i;
    }
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < kSelThreads / 64; ++q)
        if (sc[q] < c || (sc[q] == c && si[q] < i)) {
          c = sc[q]; i = si[q];
        }
      pick = i;
    }
    __syncthreads();
    const int p = pick;
    if (p == 0x7fffffff) break;   // uniform: no row qualifies
    if (tid == 0 && chosen) chosen[n] = p;
    for (int r = tid; r < B; r += kSelThreads)
      if (alive[r] && (r == p || !(pair_max[(size_t)r * B + p] >= min_gap))) alive[r] = 0;
    __syncthreads();   // alive is settled, and sc / si / pick may be written again
  }
  if (chosen)
    for (int t = n + tid; t < K; t += kSelThreads) chosen[t] = -1;
  if (tid == 0 && count) count[0] = n;
}

}  // namespace

static_assert(GTOP_SEP_ROW == 6, "the rows kernel writes six entries");

size_t gtop_separation_work_bytes(int B, int n_samples) {
  if (B <= 0) return 0;
  const size_t Bpad = sep_round_up(B, kSepTile), npad = sep_round_up(n_samples, kSepChunk);
  return npad * 3 * Bpad * sizeof(double) + 2 * Bpad * sizeof(int);
}

hipError_t gtop_launch_separation(int B, int m, const double *coeff, const double *T, int t_stride, const double *t0,
                                  int t0_stride, double t_lo, double dt, int n_samples, int hold_ends, double radius,
                                  double *pair_min, double *pair_max, double *rows, void *work, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int Bpad = sep_round_up(B, kSepTile), npad = sep_round_up(n_samples, kSepChunk), tiles = Bpad / kSepTile;
  double *pos = static_cast<double *>(work);
  int *first = reinterpret_cast<int *>(pos + (size_t)npad * 3 * Bpad), *last = first + Bpad;
  const SepGrid G = {t_lo, dt, n_samples, hold_ends};
  // enough blocks along the samples to fill the device at small B, a stride loop beyond that
  const int gy = min((npad + 3) / 4, max(1, 4096 / tiles));
  hipLaunchKernelGGL(sep_sample_kernel, dim3(tiles, gy), dim3(kSepTile, 4), 0, stream, G, B, Bpad, npad, m, coeff, T,
                     t_stride, t0, t0_stride, pos, first, last);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sep_pairs_kernel, dim3(tiles, tiles), dim3(kSepTile * kSepWaves), 0, stream, B, Bpad, npad, pos,
                     pair_min, pair_max);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(sep_rows_kernel, dim3(B), dim3(64), 0, stream, G, radius, B, Bpad, pos, first, last, pair_min, rows);
  return hipGetLastError();
}

hipError_t gtop_launch_select_distinct(int B, const unsigned char *pass, const double *cost, const double *pair_max,
                                       double min_gap, int K, int *chosen, int *count, hipStream_t stream) {
  hipLaunchKernelGGL(sep_select_kernel, dim3(1), dim3(kSelThreads), 0, stream, B, pass, cost, pair_max, min_gap, K,
                     chosen, count);
  return hipGetLastError();
}
