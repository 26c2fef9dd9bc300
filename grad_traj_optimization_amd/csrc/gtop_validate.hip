// gtop_validate.hip — the safety report of a batch of trajectories and the choice
// of the best safe one, on gfx950.  fp64.
//
// The test the reference's planner front end applies to every expanded motion
// primitive (src/kinodynamic_astar.cpp:178-213 of EpicOne1/grad_traj_optimization:
// a per-axis velocity limit, :180, and evaluateCoarseEDT(pos, time) <= margin_
// along the primitive, :207), applied to the optimised polynomials at the samples
// of PolynomialTraj::getTraj (polynomial_traj.hpp:69-78) with the interpolating
// lookup EDTEnvironment::evaluateEDTWithGrad (src/edt_environment.cpp:76-122).
//
// (1) traj_report_kernel: one WAVEFRONT per trajectory (a few for small batches,
//     see the kernel), lanes over the samples 64 at a time.  What happens per sample
//     is stated once, in gtop_report_common.h: the accumulated eval_t and the segment
//     walk are eval_trajectories_kernel's (gtop_setup.hip) too, so count, times and
//     positions are the bits gtop_sample_trajectories_device stores.  Each sample's
//     distance is the `dist` of edt_query_kernel<false, POLY> (gtop_edt.hip) for
//     (pos, tau), through the shared lookup of gtop_edt_lookup.h: the same bits again.
//     This file holds what the report does with a sample.  Nothing per sample goes to
//     HBM: per sample one 64-byte gather, ~100 fp64 operations and the box loop; per
//     trajectory 96 bytes out.
// (2) select_kernel / select_finish_kernel: the pass test per row and the passing
//     row of least cost, lowest index on a tie — a two-stage reduction over
//     (cost, index) pairs ordered lexicographically, so the result does not depend
//     on how the rows fall on the lanes.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_device_common.h"
#include "gtop_edt_lookup.h"
#include "gtop_kernels.h"
#include "gtop_report_common.h"   // the sample loop's four parts, wave_max, kValBoxChunk[Poly]

namespace {

constexpr int kReportWavesPerSimd = 4;   // traj_report_kernel's occupancy (120 VGPRs; tools/kernel_resources.py)
// Per lane the running results over its samples (a lane sees its samples in rising index, so `<` keeps the earliest of
// equal values), carried from chunk to chunk; ONE wavefront reduction per quantity when the trajectory's samples are
// done.  No workgroup barrier takes part in the sample loop or in a wavefront's reduction.
//
// W = wavefronts per trajectory.  1 is the rule.  A small batch leaves most of the chip idle at one wavefront per
// trajectory (1 024 trajectories: one wavefront per SIMD, nothing to hide the box loop's LDS and sqrt latencies
// behind — 132 us with 32 boxes, against 110 us for the composed launches, which spread the same samples over 9 440
// wavefronts), so there W wavefronts share a trajectory: wavefront w takes chunks w, w + W, ...  The accumulated
// sample time is still the reference's: a wavefront reaches its chunk's first time by the same additions, one after
// the other (64 W of them per step; uniform, ~2 us over a whole trajectory).  The W partial results meet in LDS
// behind the one barrier of the kernel's end; (distance, index) pairs combine lexicographically, so the result does
// not depend on W.  Lists of more than kValBoxChunk boxes are restaged inside the sample loop, which only W = 1 can
// do without barriers in diverging loops: the launcher sends them there.
struct ReportPartial {
  double dmin, dmin_t, below_t, cnt_below, cnt_out, vmax2, amax2, vax, aax;
  int dmin_i, below_i, nsamp;
};

// POLY: the list is a polynomial one (gtop_set_moving_box_polynomials): box_p0 is its [nbox][kBoxRowPoly] rows
// (gtop_edt_lookup.h), box_vel and box_scale are not read.
template <int W, bool POLY>
__global__ void __launch_bounds__(64 * W)
traj_report_kernel(const GtopGrid g, const double *__restrict__ rec, int nbox, const double *__restrict__ box_p0,
                   const double *__restrict__ box_vel, const double *__restrict__ box_scale, int B, int m,
                   const double *__restrict__ coeff, const double *__restrict__ T, int t_stride, double dt_sample,
                   const double *__restrict__ t0, int t0_stride, double margin,
                   double *__restrict__ report /*[B][GTOP_TRAJ_REPORT]*/) {
  constexpr int kChunk = kValBoxChunkOf<POLY>;
  __shared__ double bx[kChunk][kBoxRowOf<POLY>];   // p0, vel, scale; POLY: the list's rows
  __shared__ ReportPartial part[W];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (b >= B) return;
  const double *cf = coeff + (size_t)b * m * 18;   // row s = [cx0..5 | cy0..5 | cz0..5], ascending powers
  const double *ts = T + (size_t)b * t_stride;
  double time_sum = 0.0;                            // init(), polynomial_traj.hpp:37-43
  for (int s = 0; s < m; ++s) time_sum += ts[s];
  const bool use_boxes = nbox > 0;                  // (the launcher passes 0 boxes when the limits say static only)
  const double start = (use_boxes && t0) ? t0[(size_t)b * t0_stride] : 0.0;

  // the one chunk of boxes nearly every list is: staged once
  if (use_boxes) stage_boxes<POLY>(bx, box_p0, box_vel, box_scale, 0, min(kChunk, nbox), threadIdx.x, 64 * W);

  double dmin = INFINITY, dmin_t = 0.0, below_t = -1.0;
  int dmin_i = 0x7fffffff, below_i = 0x7fffffff, n_below = 0, n_out = 0;
  double vmax2 = 0.0, amax2 = 0.0, vax = 0.0, aax = 0.0;   // squared norms: sqrt is monotone, taken once at the end

  double base_t = sample_time_of(64 * w, dt_sample);   // the time of this wavefront's first chunk's sample 0
  int first = 64 * w, nsamp = 0;                    // index of the chunk's sample 0; samples this wavefront saw
  while (base_t <= time_sum) {                      // wave-uniform
    const auto [eval_t, next_base, live] = chunk_times(base_t, dt_sample, lane, 64 * W, time_sum);   // sample first + lane
    double p[3] = {0, 0, 0};
    if (live) {
      double t = eval_t;
      const unsigned seg = segment_of(ts, m, t);
      sample_motion(cf + seg * 18, t, p, vax, aax, vmax2, amax2);
    }
    const auto [d, out] = sample_distance<POLY, W == 1>(g, rec, bx, nbox, box_p0, box_vel, box_scale, use_boxes, start,
                                                        eval_t, live, p, lane);
    if (live) {
      const int k = first + lane;
      if (d < dmin) {
        dmin = d; dmin_t = eval_t; dmin_i = k;
      }
      if (d <= margin) {                              // the reference's comparison, kinodynamic_astar.cpp:207
        if (n_below == 0) {
          below_i = k; below_t = eval_t;
        }
        ++n_below;
      }
      n_out += out;
    }
    nsamp += __popcll(__ballot(live));
    first += 64 * W;
    base_t = next_base;
  }

  // ---- the wavefront's reductions ----
  double gd = dmin;
  int gi = dmin_i;
  for (int off = 32; off > 0; off >>= 1) {           // lexicographic min of (distance, sample index)
    const double od = __shfl_xor(gd, off);
    const int oi = __shfl_xor(gi, off);
    if (od < gd || (od == gd && oi < gi)) {
      gd = od; gi = oi;
    }
  }
  int gb = below_i;
  for (int off = 32; off > 0; off >>= 1) gb = min(gb, __shfl_xor(gb, off));
  const double cnt_below = gtop_wave_sum((double)n_below), cnt_out = gtop_wave_sum((double)n_out);
  vmax2 = wave_max(vmax2);
  amax2 = wave_max(amax2);
  vax = wave_max(vax);
  aax = wave_max(aax);
  ReportPartial &mine = part[w];
  if (lane == 0) {
    mine.dmin = INFINITY; mine.dmin_t = -1.0; mine.dmin_i = 0x7fffffff;   // no sample with a comparable distance
    mine.below_t = -1.0; mine.below_i = 0x7fffffff;
    mine.cnt_below = cnt_below; mine.cnt_out = cnt_out; mine.nsamp = nsamp;
    mine.vmax2 = vmax2; mine.amax2 = amax2; mine.vax = vax; mine.aax = aax;
  }
  __builtin_amdgcn_wave_barrier();                    // (LDS operations of one wavefront complete in order)
  if (gi != 0x7fffffff && dmin_i == gi) {             // the one lane that holds the first sample of least distance
    mine.dmin = dmin; mine.dmin_t = dmin_t; mine.dmin_i = dmin_i;
  }
  if (gb != 0x7fffffff && below_i == gb) {
    mine.below_t = below_t; mine.below_i = below_i;
  }
  __syncthreads();                                    // W = 1: this wavefront's own writes, no more
  if (threadIdx.x == 0) {
    ReportPartial r = part[0];
    for (int k = 1; k < W; ++k) {
      const ReportPartial o = part[k];
      if (o.dmin < r.dmin || (o.dmin == r.dmin && o.dmin_i < r.dmin_i)) {
        r.dmin = o.dmin; r.dmin_t = o.dmin_t; r.dmin_i = o.dmin_i;
      }
      if (o.below_i < r.below_i) {
        r.below_i = o.below_i; r.below_t = o.below_t;
      }
      r.cnt_below += o.cnt_below; r.cnt_out += o.cnt_out; r.nsamp += o.nsamp;
      r.vmax2 = fmax(r.vmax2, o.vmax2); r.amax2 = fmax(r.amax2, o.amax2);
      r.vax = fmax(r.vax, o.vax); r.aax = fmax(r.aax, o.aax);
    }
    double *o = report + (size_t)b * GTOP_TRAJ_REPORT;
    o[0] = (double)r.nsamp;
    o[1] = r.dmin; o[2] = r.dmin_t; o[3] = r.dmin_i == 0x7fffffff ? -1.0 : (double)r.dmin_i;
    o[4] = r.cnt_below; o[5] = r.below_t; o[6] = r.cnt_out;
    o[7] = sqrt(r.vmax2); o[8] = sqrt(r.amax2); o[9] = r.vax; o[10] = r.aax; o[11] = time_sum;
  }
}

// ---- selection ----
struct SelLimits {
  double max_vel, max_acc;
  int per_axis, allow_out_of_map;
};
struct SelPartial {
  double cost;   // +inf: no passing row
  int idx, count;
};

__device__ __forceinline__ bool sel_better(double c, int i, double oc, int oi) { return oc < c || (oc == c && oi < i); }

// (cost, index) lexicographic min and the sum of the counts over a 256-thread workgroup; the result in thread 0
__device__ __forceinline__ void sel_block_reduce(double &c, int &i, int &n) {
  __shared__ double sc[4];
  __shared__ int si[4], sn[4];
  for (int off = 32; off > 0; off >>= 1) {
    const double oc = __shfl_xor(c, off);
    const int oi = __shfl_xor(i, off);
    n += __shfl_xor(n, off);
    if (sel_better(c, i, oc, oi)) {
      c = oc; i = oi;
    }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sc[w] = c; si[w] = i; sn[w] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < 4; ++k) {
      n += sn[k];
      if (sel_better(c, i, sc[k], si[k])) {
        c = sc[k]; i = si[k];
      }
    }
}

constexpr int kSelBlocks = GTOP_SELECT_PARTIALS;

__global__ void __launch_bounds__(256)
select_kernel(int B, const double *__restrict__ report, const double *__restrict__ cost, SelLimits lim,
              const double *__restrict__ cert /* NULL: no certificate asked for */,
              const double *__restrict__ kin /* NULL: no kinematic certificate asked for */, int require,
              unsigned char *__restrict__ pass, SelPartial *__restrict__ part) {
  double c = INFINITY;
  int i = 0x7fffffff, n = 0;
  for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {   // rising b per thread: `<` keeps the first
    const double *r = report + (size_t)b * GTOP_TRAJ_REPORT;
    const double cb = cost[b];
    const double vel = lim.per_axis ? r[9] : r[7], acc = lim.per_axis ? r[10] : r[8];
    bool ok = r[4] == 0.0;
    ok &= lim.allow_out_of_map || r[6] == 0.0;
    ok &= lim.max_vel <= 0.0 || vel <= lim.max_vel;
    ok &= lim.max_acc <= 0.0 || acc <= lim.max_acc;
    ok &= isfinite(cb);
    if (cert) {                                          // gtop_select_best_certified_device: the verdict, entry 0
      const double verdict = cert[(size_t)b * GTOP_CERT_REPORT];
      ok &= require == GTOP_CERT_REQUIRE_SAFE ? verdict == 1.0 : verdict != -1.0;
    }
    if (kin) {                                           // gtop_select_best_kin_certified_device: likewise, WITHIN = +1
      const double verdict = kin[(size_t)b * GTOP_KIN_REPORT];
      ok &= require == GTOP_CERT_REQUIRE_SAFE ? verdict == 1.0 : verdict != -1.0;
    }
    if (pass) pass[b] = ok ? 1 : 0;
    if (ok) {
      ++n;
      if (cb < c) {
        c = cb; i = b;
      }
    }
  }
  sel_block_reduce(c, i, n);
  if (threadIdx.x == 0) part[blockIdx.x] = {c, i, n};
}

__global__ void __launch_bounds__(256)
select_finish_kernel(int nparts, const SelPartial *__restrict__ part, int *__restrict__ best) {
  double c = INFINITY;
  int i = 0x7fffffff, n = 0;
  if ((int)threadIdx.x < nparts) {
    const SelPartial p = part[threadIdx.x];
    c = p.cost; i = p.idx; n = p.count;
  }
  sel_block_reduce(c, i, n);
  if (threadIdx.x == 0) {
    best[0] = n > 0 ? i : -1;
    best[1] = n;
  }
}

}  // namespace

static_assert(sizeof(SelPartial) == GTOP_SELECT_PARTIAL_BYTES, "the context sizes the selection workspace by this");

hipError_t gtop_launch_traj_report(const GtopGrid &g, const double *rec, const GtopBoxList &boxes, int B, int m,
                                   const double *coeff, const double *T, int t_stride, double dt_sample, const double *t0,
                                   int t0_stride, double margin, double *report, int simds, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  // wavefronts per trajectory: the most of 4, 2, 1 with which the whole launch is still resident at once — B W
  // wavefronts within the kernel's kReportWavesPerSimd on each of the device's SIMDs (`simds`, four per compute unit:
  // 4 096 wavefronts on 256 compute units, i.e. W = 4 up to 1 024 rows and 2 up to 2 048).  Past that point further
  // wavefronts only queue behind the resident ones, and each pays the 64 W dependent additions per chunk that carry
  // its sample time; see the kernel's comment
  const long long resident = (long long)kReportWavesPerSimd * (simds > 0 ? simds : 1);
  const bool poly = boxes.kind == GTOP_BOX_LIST_POLYNOMIAL && boxes.count > 0;
  const int nbox = boxes.count;
  const double *box_p0 = poly ? boxes.rows : boxes.p0, *box_vel = boxes.vel, *box_scale = boxes.scale;
  const int W = nbox > (poly ? kValBoxChunkPoly : kValBoxChunk) ? 1 : (4LL * B <= resident ? 4 : (2LL * B <= resident ? 2 : 1));
#define GTOP_REPORT_LAUNCH(W_, POLY_)                                                                                    \
  hipLaunchKernelGGL((traj_report_kernel<W_, POLY_>), dim3(B), dim3(64 * W_), 0, stream, g, rec, nbox, box_p0, box_vel,  \
                     box_scale, B, m, coeff, T, t_stride, dt_sample, t0, t0_stride, margin, report)
  if (poly) {
    if (W == 4) GTOP_REPORT_LAUNCH(4, true);
    else if (W == 2) GTOP_REPORT_LAUNCH(2, true);
    else GTOP_REPORT_LAUNCH(1, true);
  } else {
    if (W == 4) GTOP_REPORT_LAUNCH(4, false);
    else if (W == 2) GTOP_REPORT_LAUNCH(2, false);
    else GTOP_REPORT_LAUNCH(1, false);
  }
#undef GTOP_REPORT_LAUNCH
  return hipGetLastError();
}

hipError_t gtop_launch_select_best(int B, const double *report, const double *cost, double max_vel, double max_acc,
                                   int per_axis, int allow_out_of_map, const double *cert, const double *kin,
                                   int require, unsigned char *pass, int *best, void *workspace, hipStream_t stream) {
  const int nblocks = B > 0 ? min(kSelBlocks, (B + 255) / 256) : 0;   // (no rows: best = {-1, 0} by the second stage alone)
  const SelLimits lim = {max_vel, max_acc, per_axis, allow_out_of_map};
  SelPartial *part = static_cast<SelPartial *>(workspace);
  if (nblocks > 0) {
    hipLaunchKernelGGL(select_kernel, dim3(nblocks), dim3(256), 0, stream, B, report, cost, lim, cert, kin, require,
                       pass, part);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(256), 0, stream, nblocks, part, best);
  return hipGetLastError();
}
