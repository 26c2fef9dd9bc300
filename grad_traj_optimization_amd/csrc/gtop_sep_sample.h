// gtop_sep_sample.h — the common time grid and the sample kernel of the kernels that set the rows of a batch against
// each other: the pairwise separation (gtop_separation.hip, include/gtop_separation.h) and the swarm separation cost
// (gtop_swarm.hip, include/gtop_swarm.h).  Stated HERE, once: tau_k, the start times, the flown samples, the segment walk
// and the positions are the same bits in both, so the positions the swarm term sees are the ones pair_min is taken over.
// Private to those two files; each includes it after gtop_report_common.h, under `#pragma clang fp contract(off)`.
//
// The layout the kernel writes: pos [npad][3][Bpad] doubles — sample k, axis a of row b at (k 3 + a) Bpad + b, Bpad = B
// rounded up to the tile edge, npad = n_samples rounded up to the chunk — and first [Bpad], last [Bpad] int32, the flown
// samples of a row (contiguous in k; first > last: none).  A sample at which a row is NOT flown, a padding row and a
// padding sample hold NaN.
#ifndef GTOP_SEP_SAMPLE_H_
#define GTOP_SEP_SAMPLE_H_

#include <hip/hip_runtime.h>

#include "gtop_report_common.h"   // segment_of, poly_eval

namespace {

constexpr int kSepTile = 64;     // rows per side of a tile of pairs: the lanes of a wavefront hold one side
constexpr int kSepChunk = 8;     // grid samples per turn of the pair kernel's loop (its unroll): the workspace is padded to it

__host__ __device__ inline int sep_round_up(int v, int to) { return (v + to - 1) / to * to; }

struct SepGrid {
  double t_lo, dt;
  int n, hold_ends;
};

__device__ __forceinline__ double sep_tau(const SepGrid &G, int k) { return G.t_lo + (double)k * G.dt; }

// ---- (1) sample ----
// Lanes over the rows (the stores are coalesced along b, which is how the pair kernel stages them), threadIdx.y and the
// grid's y over the samples.  Row y == 0 of the first block also leaves the row's flown range: u_k is non-decreasing in k
// (every step of tau_k and of the subtraction is a monotone rounding), so both ends are found by bisection.
__global__ void __launch_bounds__(kSepTile * 4)
sep_sample_kernel(SepGrid G, int B, int Bpad, int npad, int m, const double *__restrict__ coeff,
                  const double *__restrict__ T, int t_stride, const double *__restrict__ t0, int t0_stride,
                  double *__restrict__ pos, int *__restrict__ first, int *__restrict__ last) {
  const int b = blockIdx.x * kSepTile + threadIdx.x;
  const bool row = b < B;
  const double *ts = T + (size_t)(row ? b : 0) * t_stride;
  const double *cf = coeff + (size_t)(row ? b : 0) * m * 18;
  double time_sum = 0.0;
  for (int s = 0; s < m; ++s) time_sum += ts[s];
  const double start = (row && t0) ? t0[(size_t)b * t0_stride] : 0.0;
  const double nan = __builtin_nan("");
  for (int k = blockIdx.y * 4 + threadIdx.y; k < npad; k += gridDim.y * 4) {
    double p[3] = {nan, nan, nan};
    if (row && k < G.n) {
      double u = sep_tau(G, k) - start;
      bool flown = u >= 0.0 && u <= time_sum;
      if (G.hold_ends) {
        u = u < 0.0 ? 0.0 : (u > time_sum ? time_sum : u);
        flown = true;
      }
      if (flown) {
        const unsigned idx = segment_of(ts, m, u);
        const double *seg = cf + (size_t)idx * 18;
        for (int a = 0; a < 3; ++a) p[a] = poly_eval(seg + 6 * a, u);
      }
    }
    for (int a = 0; a < 3; ++a) pos[((size_t)k * 3 + a) * Bpad + b] = p[a];
  }
  if (blockIdx.y == 0 && threadIdx.y == 0) {
    int kf = G.n, kl = -1;   // a padding row: flown nowhere
    if (row && G.hold_ends) {
      kf = 0; kl = G.n - 1;
    } else if (row) {
      int lo = 0, hi = G.n;   // the first k with u_k >= 0
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sep_tau(G, mid) - start >= 0.0) hi = mid;
        else lo = mid + 1;
      }
      kf = lo;
      lo = 0; hi = G.n;       // the first k with u_k <= time_sum no longer true
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!(sep_tau(G, mid) - start <= time_sum)) hi = mid;
        else lo = mid + 1;
      }
      kl = lo - 1;
    }
    first[b] = kf;
    last[b] = kl;
  }
}

// the launch of the kernel above for B rows: enough blocks along the samples to fill the device at small B, a stride
// loop beyond that
inline hipError_t sep_launch_sample(const SepGrid &G, int B, int m, const double *coeff, const double *T, int t_stride,
                                    const double *t0, int t0_stride, double *pos, int *first, int *last,
                                    hipStream_t stream) {
  const int Bpad = sep_round_up(B, kSepTile), npad = sep_round_up(G.n, kSepChunk), tiles = Bpad / kSepTile;
  const int gy = min((npad + 3) / 4, max(1, 4096 / tiles));
  hipLaunchKernelGGL(sep_sample_kernel, dim3(tiles, gy), dim3(kSepTile, 4), 0, stream, G, B, Bpad, npad, m, coeff, T,
                     t_stride, t0, t0_stride, pos, first, last);
  return hipGetLastError();
}

}  // namespace

#endif  // GTOP_SEP_SAMPLE_H_
