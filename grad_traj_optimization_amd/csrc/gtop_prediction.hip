// gtop_prediction.hip — moving-obstacle predictions fitted from observation histories, on gfx950, fp64
// (include/gtop_prediction.h: gtop_fit_predictions_device, gtop_refresh_box_predictions_device).
//
// One wavefront per object, a workgroup of one wavefront: no barrier, no LDS allocation, no scratch.
//   (1) sums      the lanes take the object's samples 64 at a time, each its own 32-byte sample as two 16-byte loads (a
//                 chunk is 2 KiB contiguous apart from the ring's wrap), form the 29 terms and reduce them by the pair
//                 tree of the interface (xor 1, 2, 4, 8, 16, 32: lane l and lane l ^ m add the same two numbers, and
//                 addition commutes, so every lane ends with the chunk sum); chunk sums are added in chunk order.
//   (2) solve     the factor is the same in every lane; lane l substitutes axis l % 3, so the three axes run side by
//                 side in ONE instruction stream (lanes 0 .. 2 are the ones read afterwards).
//   (3) residual  the three axes' rows broadcast from lanes 0 .. 2, the samples read again (they are in cache), the
//                 consumers' centre at every sample.
//   (4) write     nothing but the info row unless the object was fitted; then the row, either to the caller's outputs
//                 or (CTX) straight into the context's box buffers.
// The arithmetic behind the sums is gtop_prediction_fit.h's, shared with the host form.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_kernels.h"

// Every step is ONE rounded fp64 operation in the order the header writes it: a restatement in Python scalars
// reproduces the bits (tests/predict_twin.py).
#pragma clang fp contract(off)

#include "gtop_prediction_fit.h"

namespace {

__device__ __forceinline__ double pred_tree_sum(double v) {
#pragma unroll
  for (int m = 1; m < kPredChunk; m <<= 1) v = v + __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double pred_tree_max(double v) {
#pragma unroll
  for (int m = 1; m < kPredChunk; m <<= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double pred_pick3(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

// sample i (0 <= i < cnt <= H) of the ring that starts at slot hm (0 <= hm < H)
__device__ __forceinline__ void pred_load(const double2 *__restrict__ hn, int hm, int H, int i, double smp[4]) {
  int slot = hm + i;
  if (slot >= H) slot -= H;
  const double2 a = hn[2 * (size_t)slot], b = hn[2 * (size_t)slot + 1];
  smp[0] = a.x; smp[1] = a.y; smp[2] = b.x; smp[3] = b.y;
}

// CTX == false: out_a = coef [N][18], out_b = t_range [N][2], local [N][20] or NULL.
// CTX == true:  out_a = the context's box buffer [N][kBoxRowPoly], out_b = the cost bodies' rows or NULL, scale [N][3]
//               or NULL (the extents stay).
template <int MODE, bool CTX>
__global__ void __launch_bounds__(kPredChunk)
pred_fit_kernel(int H, const double2 *__restrict__ hist, const int *__restrict__ count, const int *__restrict__ head,
                GtopPredictArgs o, double *__restrict__ out_a, double *__restrict__ out_b,
                const double *__restrict__ scale, double *__restrict__ info, double *__restrict__ local) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int raw = count[n];
  const int cnt = raw < 0 ? 0 : (raw > H ? H : raw);
  int hm = 0;
  if (head) {
    hm = head[n] % H;
    if (hm < 0) hm += H;
  }
  const double2 *hn = hist + (size_t)n * H * 2;
  double *inf = info + (size_t)n * kPredInfo;

  int status = cnt != raw ? kPredBad : (cnt == 0 ? kPredEmpty : kPredOk);
  double first[4] = {0.0, 0.0, 0.0, 0.0}, last[4] = {0.0, 0.0, 0.0, 0.0}, prev[4] = {0.0, 0.0, 0.0, 0.0};
  if (status == kPredOk) {
    pred_load(hn, hm, H, 0, first);
    pred_load(hn, hm, H, cnt - 1, last);
    if (MODE == kPredConstVel && cnt >= 2) pred_load(hn, hm, H, cnt - 2, prev);
  }
  const double t_first = first[3], t_last = last[3];
  const bool fitting = MODE == kPredPolyfit && cnt >= 2;
  const double sigma = fitting ? t_last - t_first : ((MODE == kPredConstVel && cnt >= 2) ? t_last - prev[3] : 0.0);

  // ---- (1) the finite check of every sample and, where a polynomial is fitted, the 29 sums ----
  double sums[kPredSums];
#pragma unroll
  for (int q = 0; q < kPredSums; ++q) sums[q] = 0.0;
  if (status == kPredOk) {
    bool fin = true;
    for (int base = 0; base < cnt; base += kPredChunk) {
      const int i = base + lane;
      const bool have = i < cnt;
      double smp[4] = {0.0, 0.0, 0.0, 0.0};
      if (have) pred_load(hn, hm, H, i, smp);
      fin = fin && pred_finite(smp[0]) && pred_finite(smp[1]) && pred_finite(smp[2]) && pred_finite(smp[3]);
      if (fitting) {
        double term[kPredSums];
        pred_terms((smp[3] - t_last) / sigma, smp, term);
#pragma unroll
        for (int q = 0; q < kPredSums; ++q) sums[q] = sums[q] + pred_tree_sum(have ? term[q] : 0.0);
      }
    }
    if (__any(!fin)) status = kPredBad;
    else if (cnt >= 2 && !(t_last - t_first > 0.0)) status = kPredBad;
    else if (MODE == kPredConstVel && cnt >= 2 && !(prev[3] < t_last)) status = kPredBad;
  }

  // ---- (2) this lane's axis ----
  const int k = lane % 3;
  int deg = 0;
  double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double t_start = t_first;
  if (status == kPredOk) {
    if (cnt == 1) {
      status = kPredLowered;
      g[0] = pred_pick3(last, k);
      c[0] = g[0];
      t_start = t_last;
    } else if (MODE == kPredConstVel) {
      deg = 1;
      t_start = prev[3];
      const double q2 = pred_pick3(last, k);
      g[0] = q2;
      g[1] = q2 - pred_pick3(prev, k);
      c[1] = g[1] / sigma;
      c[0] = q2 - c[1] * t_last;
    } else {
      const double e = o.regularise_horizon ? o.horizon / sigma : 0.0;
      const double lam_e = o.lambda / ((sigma * sigma) * sigma);
      double L[6][6];
      const int deg0 = o.degree < cnt - 1 ? o.degree : cnt - 1;
      deg = pred_factor(sums, lam_e, e, deg0, L);
      if (deg < o.degree) status = kPredLowered;
      double b[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) b[j] = pred_pick3(sums + 11 + 3 * j, k);
      pred_substitute(L, deg, b, g);
      if (__any(!pred_all_finite6(g))) status = kPredBad;
      else pred_to_row(g, sigma, t_last, c);
    }
    if (status != kPredBad && __any(!pred_all_finite6(c))) status = kPredBad;
  }
  double half = 0.0;
  if (CTX && scale && status <= kPredLowered) {
    const double sc = scale[3 * (size_t)n + k];
    if (__any(!(pred_finite(sc) && sc >= 0.0))) status = kPredBad;
    half = 0.5 * sc;
  }
  if (status >= kPredEmpty) {   // only the info row: status, count, zeros
    if (lane < kPredInfo) inf[lane] = lane == 0 ? (double)status : (lane == 1 ? (double)cnt : 0.0);
    return;
  }

  // ---- (3) the residuals at the consumers' own centre ----
  double row[3][6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int j = 0; j < 6; ++j) row[a][j] = __shfl(c[j], a);
  }
  double resmax[3] = {0.0, 0.0, 0.0}, esum = 0.0;
  for (int base = 0; base < cnt; base += kPredChunk) {
    const int i = base + lane;
    const bool have = i < cnt;
    double smp[4] = {0.0, 0.0, 0.0, 0.0};
    if (have) pred_load(hn, hm, H, i, smp);
    double r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r[a] = pred_centre(row[a], smp[3]) - smp[a];
      resmax[a] = fmax(resmax[a], have ? fabs(r[a]) : 0.0);
    }
    const double sq = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    esum = esum + pred_tree_sum(have ? sq : 0.0);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) resmax[a] = pred_tree_max(resmax[a]);
  const double rms = sqrt(esum / (double)(3 * (long long)cnt));
  const double t_end = t_last + o.horizon;

  // ---- (4) write ----
  if (lane == 0) {
    inf[0] = (double)status; inf[1] = (double)cnt; inf[2] = (double)deg;
    inf[3] = t_start; inf[4] = t_last; inf[5] = t_end;
    inf[6] = resmax[0]; inf[7] = resmax[1]; inf[8] = resmax[2];
    inf[9] = rms; inf[10] = 0.0; inf[11] = 0.0;
  }
  if constexpr (CTX) {
    if (scale) half = half + o.inflate * pred_pick3(resmax, k);
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      double *dst = w == 0 ? out_a : out_b;
      if (!dst) continue;
      dst += (size_t)n * kBoxRowPoly;
      if (lane < 3) {
#pragma unroll
        for (int j = 0; j < 6; ++j) dst[6 * k + j] = c[j];
        if (scale) dst[18 + k] = half;
      }
      if (lane == 0) {
        dst[21] = t_start;
        dst[22] = t_end;
      }
    }
  } else {
    if (lane < 3) {
#pragma unroll
      for (int j = 0; j < 6; ++j) out_a[18 * (size_t)n + 6 * k + j] = c[j];
      if (local) {
#pragma unroll
        for (int j = 0; j < 6; ++j) local[kPredLocal * (size_t)n + 6 * k + j] = g[j];
      }
    }
    if (lane == 0) {
      out_b[2 * (size_t)n] = t_start;
      out_b[2 * (size_t)n + 1] = t_end;
      if (local) {
        local[kPredLocal * (size_t)n + 18] = t_last;
        local[kPredLocal * (size_t)n + 19] = sigma;
      }
    }
  }
}

template <bool CTX>
hipError_t pred_launch(int mode, int N, int H, const double *hist, const int *count, const int *head,
                       const GtopPredictArgs &o, double *out_a, double *out_b, const double *scale, double *info,
                       double *local, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const double2 *h2 = reinterpret_cast<const double2 *>(hist);
  if (mode == kPredConstVel)
    pred_fit_kernel<kPredConstVel, CTX><<<N, kPredChunk, 0, stream>>>(H, h2, count, head, o, out_a, out_b, scale, info, local);
  else
    pred_fit_kernel<kPredPolyfit, CTX><<<N, kPredChunk, 0, stream>>>(H, h2, count, head, o, out_a, out_b, scale, info, local);
  return hipGetLastError();
}

}  // namespace

hipError_t gtop_launch_fit_predictions(int mode, int N, int H, const double *hist, const int *count, const int *head,
                                       const GtopPredictArgs &o, double *coef, double *t_range, double *info,
                                       double *local, hipStream_t stream) {
  return pred_launch<false>(mode, N, H, hist, count, head, o, coef, t_range, nullptr, info, local, stream);
}

hipError_t gtop_launch_refresh_predictions(int mode, int N, int H, const double *hist, const int *count, const int *head,
                                           const GtopPredictArgs &o, const double *scale, double *rows, double *cost_rows,
                                           double *info, hipStream_t stream) {
  return pred_launch<true>(mode, N, H, hist, count, head, o, rows, cost_rows, scale, info, nullptr, stream);
}
