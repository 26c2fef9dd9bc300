// gtop_segments.hip — the per-segment safety report of a batch of trajectories on gfx950
// (gtop_validate_segments_device of include/gtop.h).  fp64.
//
// The whole-trajectory report (traj_report_kernel, gtop_validate.hip) says THAT a row fails and at which sample its
// clearance is least; a caller who wants to repair the row — insert a waypoint, stretch a time — needs the same figures
// per segment.  The samples, the segment each one belongs to, positions, velocities, accelerations and distances are
// that kernel's: both take them from the one statement of the sample loop in gtop_report_common.h (the accumulated
// eval_t, the segment walk with the last segment extended, poly_eval / poly_vel / poly_acc, the lookup of
// gtop_edt_lookup.h at tau = t0[b] + eval_t with boxes and -1 without), so they are the same bits.  This file holds
// what is done with a sample here: the reduction per segment.
//
// One WAVEFRONT per trajectory, lanes over the samples 64 at a time.  A sample's segment never falls as the sample
// index rises, so the members of one segment are a run of lanes.  Inside a chunk the wavefront loops over the distinct
// segments present: the first unprocessed live lane names the segment, a ballot names its members, and the wavefront
// reductions run with neutral elements for everybody else.  The running partial of the CURRENT segment lives in
// wave-uniform registers from chunk to chunk (a segment longer than 64 samples spans several).  A segment's row is
// stored once, when the walk leaves it — with the empty rows of the segments the walk skipped (times below dt_sample),
// and at the end the rows it never reached.  No LDS accumulators, no atomics, no workgroup barrier in the sample loop
// beyond the restaging of a box list longer than one LDS stage, exactly as the report's W = 1 form does it.
// (distance, sample index) pairs combine lexicographically: a segment's clearance belongs to its first sample that
// attains it.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_device_common.h"
#include "gtop_edt_lookup.h"
#include "gtop_kernels.h"
#include "gtop_report_common.h"

namespace {

constexpr int kNoSample = 0x7fffffff;

// rows s0 .. s1 - 1 of a trajectory's report as segments without samples (wave-uniform bounds; lanes over the entries)
__device__ __forceinline__ void store_empty_rows(double *__restrict__ rows, int s0, int s1, int lane) {
  for (int q = lane; q < (s1 - s0) * GTOP_SEG_REPORT; q += 64) {
    const int e = q % GTOP_SEG_REPORT;
    rows[(size_t)s0 * GTOP_SEG_REPORT + q] = (e == 1 || e == 3) ? -1.0 : (e == 2 ? INFINITY : 0.0);
  }
}

// the running partial of one segment; wave-uniform
struct SegPartial {
  int n, first, n_below, n_out, dmin_i;
  double dmin, dmin_t, vmax2, amax2, vax, aax;
};

__device__ __forceinline__ void seg_reset(SegPartial &r, int first) {
  r.n = 0; r.first = first; r.n_below = 0; r.n_out = 0; r.dmin_i = kNoSample;
  r.dmin = INFINITY; r.dmin_t = -1.0; r.vmax2 = 0.0; r.amax2 = 0.0; r.vax = 0.0; r.aax = 0.0;
}

__device__ __forceinline__ void seg_store(double *__restrict__ rows, int s, const SegPartial &r, int lane) {
  if (lane == 0) {
    double *o = rows + (size_t)s * GTOP_SEG_REPORT;
    o[0] = (double)r.n; o[1] = (double)r.first;
    o[2] = r.dmin; o[3] = r.dmin_t;               // (no sample with a comparable distance: +inf, -1)
    o[4] = (double)r.n_below; o[5] = (double)r.n_out;
    o[6] = sqrt(r.vmax2); o[7] = sqrt(r.amax2); o[8] = r.vax; o[9] = r.aax;
  }
}

template <bool POLY>
__global__ void __launch_bounds__(64)
traj_segments_kernel(const GtopGrid g, const double *__restrict__ rec, int nbox, const double *__restrict__ box_p0,
                     const double *__restrict__ box_vel, const double *__restrict__ box_scale, int B, int m,
                     const double *__restrict__ coeff, const double *__restrict__ T, int t_stride, double dt_sample,
                     const double *__restrict__ t0, int t0_stride, double margin,
                     double *__restrict__ seg_report /*[B][m][GTOP_SEG_REPORT]*/) {
  constexpr int kChunk = kValBoxChunkOf<POLY>;
  __shared__ double bx[kChunk][kBoxRowOf<POLY>];   // p0, vel, scale; POLY: the list's rows
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const double *cf = coeff + (size_t)b * m * 18;   // row s = [cx0..5 | cy0..5 | cz0..5], ascending powers
  const double *ts = T + (size_t)b * t_stride;
  double *rows = seg_report + (size_t)b * m * GTOP_SEG_REPORT;
  double time_sum = 0.0;                            // init(), polynomial_traj.hpp:37-43
  for (int s = 0; s < m; ++s) time_sum += ts[s];
  const bool use_boxes = nbox > 0;                  // (the launcher passes 0 boxes when the limits say static only)
  const double start = (use_boxes && t0) ? t0[(size_t)b * t0_stride] : 0.0;

  // the one chunk of boxes nearly every list is: staged once
  if (use_boxes) stage_boxes<POLY>(bx, box_p0, box_vel, box_scale, 0, min(kChunk, nbox), lane, 64);

  int cur = -1;                                     // the segment whose partial `run` holds; -1: none yet
  SegPartial run;
  seg_reset(run, -1);

  double base_t = 0.0;                              // the time of the chunk's sample 0
  int first = 0;                                    // its index
  while (base_t <= time_sum) {                      // wave-uniform
    const auto [eval_t, next_base, live] = chunk_times(base_t, dt_sample, lane, 64, time_sum);   // sample first + lane
    double p[3] = {0, 0, 0};
    int seg = -1;
    double v2 = 0.0, a2 = 0.0, vax = 0.0, aax = 0.0;   // this sample's; squared norms: sqrt is monotone, taken at the store
    if (live) {
      double t = eval_t;
      const unsigned idx = segment_of(ts, m, t);
      seg = idx;
      sample_motion(cf + idx * 18, t, p, vax, aax, v2, a2);
    }
    const auto [d, out] = sample_distance<POLY, true>(g, rec, bx, nbox, box_p0, box_vel, box_scale, use_boxes, start,
                                                      eval_t, live, p, lane);

    // ---- the chunk's segments, in rising order ----
    unsigned long long todo = __ballot(live);
    while (todo) {                                    // wave-uniform
      const int leader = __builtin_ctzll(todo);
      const int s = __shfl(seg, leader);
      const bool mem = live && seg == s;
      const unsigned long long members = __ballot(mem);
      todo &= ~members;
      if (s != cur) {                                 // the walk has left `cur`: its row, and the rows it jumped over
        if (cur >= 0) seg_store(rows, cur, run, lane);
        store_empty_rows(rows, cur + 1, s, lane);
        cur = s;
        seg_reset(run, first + leader);
      }
      run.n += __popcll(members);
      run.n_below += __popcll(__ballot(mem && d <= margin));   // the reference's comparison, kinodynamic_astar.cpp:207
      run.n_out += __popcll(__ballot(mem && out));
      // lexicographic min of (distance, sample index) over the members with a comparable distance, as the report's
      // per-lane `d < dmin` admits them (a NaN or +inf distance never becomes a clearance)
      const bool cand = mem && d < INFINITY;
      double gd = cand ? d : INFINITY;
      int gi = cand ? first + lane : kNoSample;
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(gd, off);
        const int oi = __shfl_xor(gi, off);
        if (od < gd || (od == gd && oi < gi)) {
          gd = od; gi = oi;
        }
      }
      if (gi != kNoSample && gd < run.dmin) {         // (this chunk's indices lie behind the partial's: `<` keeps the first)
        run.dmin = gd; run.dmin_i = gi;
        run.dmin_t = __shfl(eval_t, gi - first);
      }
      run.vmax2 = fmax(run.vmax2, wave_max(mem ? v2 : 0.0));
      run.amax2 = fmax(run.amax2, wave_max(mem ? a2 : 0.0));
      run.vax = fmax(run.vax, wave_max(mem ? vax : 0.0));
      run.aax = fmax(run.aax, wave_max(mem ? aax : 0.0));
    }
    first += 64;
    base_t = next_base;
  }
  if (cur >= 0) seg_store(rows, cur, run, lane);
  store_empty_rows(rows, cur + 1, m, lane);           // the segments no sample reached
}

}  // namespace

hipError_t gtop_launch_traj_segments(const GtopGrid &g, const double *rec, const GtopBoxList &boxes, int B, int m,
                                     const double *coeff, const double *T, int t_stride, double dt_sample,
                                     const double *t0, int t0_stride, double margin, double *seg_report,
                                     hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int nbox = boxes.count;
  if (boxes.kind == GTOP_BOX_LIST_POLYNOMIAL && nbox > 0)
    hipLaunchKernelGGL(traj_segments_kernel<true>, dim3(B), dim3(64), 0, stream, g, rec, nbox, boxes.rows, nullptr, nullptr,
                       B, m, coeff, T, t_stride, dt_sample, t0, t0_stride, margin, seg_report);
  else
    hipLaunchKernelGGL(traj_segments_kernel<false>, dim3(B), dim3(64), 0, stream, g, rec, nbox, boxes.p0, boxes.vel,
                       boxes.scale, B, m, coeff, T, t_stride, dt_sample, t0, t0_stride, margin, seg_report);
  return hipGetLastError();
}
