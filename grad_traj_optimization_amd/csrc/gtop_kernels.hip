// gtop_kernels.hip — hand-written gfx950 (CDNA4) kernels for the batched
// cost/gradient callback of GTOP.  No MFMA: this is a stencil/gather path.
//
// What one launch computes, per trajectory b (reference lines are file:line
// into EpicOne1/grad_traj_optimization):
//   cost_b, grad_b = GradTrajOptimizer::getCostAndGradient(x_b)
//                    (src/grad_traj_optimizer.cpp:281-432)
// with the distance query SDFMap::getDistWithGradTrilinear
// (src/sdf_map.cpp:185-242) inlined.
//
// Formulation.  The reference multiplies dense L (6m x 3m+3)
// and R ((3m+3)^2) that it built once from segment_time
// (src/qp_generator.cpp:357-405).  A is block diagonal, so L's row-block s is
// A_s^-1 (quintic Hermite, closed form) scattered onto the columns of
// waypoints s and s+1, and d'Rd = sum_s c_s' Q_s c_s.  The kernel therefore
// takes (x, Df, T) and works per segment.  ONE kernel family serves every
// launch, gtop_eval_wave_kernel: a wavefront owns one or two
// whole trajectories — or as many as fit —, a segment is sampled by LPS = 30/SPL
// adjacent lanes with SPL samples each (SPL = 3: ten lanes, up to 6 segments;
// SPL = 6: five lanes, up to 12 segments at a time; SPL = 10 / 30: three lanes /
// one lane, 21 / 64 segment slots shared by 21/m / 64/m trajectories), and the
// evaluation is one dependent chain:
//   * every lane of a segment forms the segment's 18 polynomial coefficients
//     c_{s,k} = A_s^-1 d_{s,k} in registers;
//   * per sample: position/velocity (float round trip), trilinear field lookup
//     with analytic gradient, exp penalty; each sample adds
//     w1_k*[t^j] + w2_k*[j t^(j-1)] to the lane's 18-entry coefficient-space
//     gradient, which lane 0 of the segment STARTED at the jerk term ws*2Qc;
//   * after its samples the lane applies A_s^-T (linear, commutes with the
//     sums); the lanes write to an LDS tile, and each free variable = end of
//     segment w-1 + start of segment w, +1e-5, is summed from it; the scalar
//     cost is summed the same way, +1e-3;
//   * with the optimizer state as template argument the same wavefront then
//     runs the CCSA-MMA update and evaluates again (the whole loop, one launch).
// All structural zeros the reference multiplies through are skipped; nothing
// else is approximated.

#include "gtop_wave_kernel.h"

// This file is compiled TWICE (csrc/Makefile): as it stands — every reference-mode body and the launchers
// the C-ABI layer calls — and with -DGTOP_CONSISTENT_TU into an object of its own that holds the consistent-gradient
// bodies (MM wrapped in GtopConsistent) behind launchers named *_consistent, which the launchers of the first object
// forward to when the plan asks for that mode.  Two objects so that the two sets of bodies compile side by side and
// the reference-mode object is the same code, instruction for instruction, as before the mode existed.
#ifdef GTOP_CONSISTENT_TU
template <typename MM> using GtopModeOf = GtopConsistent<MM>;
#define GTOP_LAUNCHER(name) name##_consistent
constexpr bool kReferenceObject = false;
#else
template <typename MM> using GtopModeOf = MM;
#define GTOP_LAUNCHER(name) name
constexpr bool kReferenceObject = true;
#endif

namespace {

constexpr int kWaveMinw3From = 3072;   // batches that put a third wavefront on a SIMD (1 024 SIMDs)

template <typename R, typename MM>
using WaveKernelFn = void (*)(const R *, const R *, const R *, int, int, int, int, int, unsigned, unsigned, const R *,
                              const GtopKernelArgs<R>, const GtopWaveConsts<R>, const MM, const GtopSetupConsts<R>);

// one geometry: the collision-free, the ordinary and the DYN instantiation (DYN: one sample at a time, MINW >= 3)
template <typename R, bool WIDE, int SPL, int NT, int MINW, typename MM, bool LONG, int NW = 1>
static WaveKernelFn<R, MM> pick_body(bool colli, bool dyn) {
  if (!colli) {   // (:346: no sample loop, no DYN — and no consistent-gradient body: the launchers run the reference one)
    if constexpr (kIsCons<MM>) return nullptr;
    else return gtop_eval_wave_kernel<R, WIDE, SPL, NT, false, MINW, MM, false, LONG, NW>;
  }
  if (dyn) return gtop_eval_wave_kernel<R, WIDE, SPL, NT, true, (MINW < 3 ? 3 : MINW), MM, true, LONG, NW>;
  return gtop_eval_wave_kernel<R, WIDE, SPL, NT, true, MINW, MM, false, LONG, NW>;
}

template <typename R, bool WIDE, typename MM>
static WaveKernelFn<R, MM> pick_geometry(const GtopEvalPlan &p, int B, bool colli, bool dyn) {
  constexpr bool MMA = kIsMma<MM>;
  if (p.is_long) return pick_body<R, WIDE, 6, 1, 3, MM, true>(colli, dyn);
  if (p.spl == 30) {
    if constexpr (MMA) return nullptr;   // (the optimizer loop: one or two trajectories per wavefront)
    else return pick_body<R, WIDE, 30, 1, 3, MM, false>(colli, dyn);
  }
  if (p.spl == 10) {
    if constexpr (MMA) return nullptr;
    else return pick_body<R, WIDE, 10, 1, 3, MM, false>(colli, dyn);
  }
  if constexpr (!MMA) {
    if (p.nw == 2) return pick_body<R, WIDE, 3, 1, 2, MM, false, 2>(colli, dyn);   // (small batches only: the latency structure)
  }
  if (p.spl == 3) {
    // latency variant (every corner load of a lane in flight, 252 VGPRs) up to the batch that puts a third wavefront
    // on a SIMD; the optimizer loop at every size (its update's working set spills a 168-VGPR budget); 64-bit field
    // indices cost the 168-VGPR fp64 body 14 spilled registers: those stay on the two-wavefront budget too
    if constexpr (!MMA && !(WIDE && sizeof(R) == 8)) {
      if (B >= kWaveMinw3From) return pick_body<R, WIDE, 3, 1, 3, MM, false>(colli, dyn);
    }
    return pick_body<R, WIDE, 3, 1, 2, MM, false>(colli, dyn);
  }
  if (p.nt == 2) {
    if constexpr (MMA) {   // (the loop never takes two trajectories per wavefront with DYN: gtop_optimize_device_ex)
      if (dyn) return nullptr;
      if constexpr (kIsCons<MM>) {
        return colli ? gtop_eval_wave_kernel<R, WIDE, 6, 2, true, 3, MM, false, false, 1> : nullptr;
      } else {
        return colli ? gtop_eval_wave_kernel<R, WIDE, 6, 2, true, 3, MM, false, false, 1>
                     : gtop_eval_wave_kernel<R, WIDE, 6, 2, false, 3, MM, false, false, 1>;
      }
    } else {
      return pick_body<R, WIDE, 6, 2, 3, MM, false>(colli, dyn);
    }
  }
  return pick_body<R, WIDE, 6, 1, 3, MM, false>(colli, dyn);
}

// The moving-obstacle bodies (MM = GtopMoving<...>, or GtopMovingPoly<...> for a polynomial box list; fp64): one sample at a time on the two-wavefront budget, with and without the
// velocity / acceleration block, for ten lanes per segment (up to 6 segments), five lanes per segment with one
// trajectory (up to 12) or — plain evaluations — two (up to 6 each), and the chunked body past 12 segments.  Three
// lanes or one lane per segment and two wavefronts per trajectory have no such body: nullptr (gtop_eval_plan_moving
// never picks them).
template <bool WIDE, int SPL, int NT, typename MM, bool LONG>
static WaveKernelFn<double, MM> pick_body_moving(bool dyn) {
  if (dyn) return gtop_eval_wave_kernel<double, WIDE, SPL, NT, true, 3, MM, true, LONG, 1>;
  return gtop_eval_wave_kernel<double, WIDE, SPL, NT, true, 3, MM, false, LONG, 1>;
}
template <bool WIDE, typename MM>
static WaveKernelFn<double, MM> pick_geometry_moving(const GtopEvalPlan &p, bool dyn) {
  constexpr bool MMA = kIsMma<MM>;
  if (p.nw != 1 || (p.spl != 3 && p.spl != 6)) return nullptr;
  if (p.is_long) return pick_body_moving<WIDE, 6, 1, MM, true>(dyn);
  if (p.spl == 3) return pick_body_moving<WIDE, 3, 1, MM, false>(dyn);
  if (p.nt == 2) {
    if constexpr (MMA) return nullptr;   // (the loop keeps one trajectory per wavefront, as with DYN)
    else return pick_body_moving<WIDE, 6, 2, MM, false>(dyn);
  }
  return pick_body_moving<WIDE, 6, 1, MM, false>(dyn);
}

// one launch covers up to 2^25 wavefronts (grid x 64 threads stays below 2^32); a larger batch goes in slices
constexpr int kMaxGroupsPerLaunch = 1 << 25;

template <typename MM> struct MovingBase { using type = MM; };
template <typename Base> struct MovingBase<GtopMoving<Base>> { using type = Base; };
template <typename Base> struct MovingBase<GtopMovingPoly<Base>> { using type = Base; };

// the collision term is in force (:346), as launch_wave decides it
template <typename R> static bool has_collision_term(const GtopKernelArgs<R> &args) {
  return !((args.wc < (R)0 ? -args.wc : args.wc) < (R)1e-4);
}
// the launch's MM argument in this object's gradient mode
template <typename MM> static GtopModeOf<MM> mode_args(const MM &st) {
  GtopModeOf<MM> w;
  static_cast<MM &>(w) = st;
  return w;
}

template <typename R, typename MM>
static hipError_t launch_wave(const GtopKernelArgs<R> &args, const MM &st, const GtopEvalPlan &plan, bool dyn,
                              hipStream_t stream) {
  constexpr bool MMA = kIsMma<MM>;
  constexpr bool MOV = kIsMov<MM>;
  if (args.B <= 0) return hipSuccess;
  GtopKernelArgs<R> wa = args;
  if (wa.step == 1) wa.ws = (R)0;   // :412-415, applied here so that the kernel need not fetch `step`
  const bool colli = has_collision_term(wa);   // :346
  dyn = dyn && wa.step == 2;        // the commented-out block's own test (:383)
  const bool wide = !gtop_field_is_narrow(wa.nx, wa.ny, wa.nz, sizeof(R));
  WaveKernelFn<R, MM> kern;
  if constexpr (MOV) {   // the moving-obstacle term lives in the sample loop: without a collision term there is none
    if constexpr (!kIsCons<MM>) {   // (the consistent-gradient launchers are only called with a collision term)
      using Base = typename MovingBase<MM>::type;
      if (!colli) return launch_wave<R, Base>(args, static_cast<const Base &>(st), plan, dyn, stream);
    }
    kern = wide ? pick_geometry_moving<true, MM>(plan, dyn) : pick_geometry_moving<false, MM>(plan, dyn);
  } else if constexpr (MMA && sizeof(R) == 4) {   // (the optimizer loop with fp32 evaluations: no 64-bit-index bodies — a field past 4 GiB in fp32)
    if (wide) return hipErrorInvalidValue;
    kern = pick_geometry<R, false, MM>(plan, wa.B, colli, dyn);
  } else {
    kern = wide ? pick_geometry<R, true, MM>(plan, wa.B, colli, dyn) : pick_geometry<R, false, MM>(plan, wa.B, colli, dyn);
  }
  if (!kern) return hipErrorInvalidValue;
  const size_t smem = gtop_wave_lds_bytes(plan, wa.m, MMA ? sizeof(double) : sizeof(R), MMA);   // (the optimizer's state is fp64)
  if (smem > 160u * 1024u) return hipErrorInvalidValue;
  if (smem > 64u * 1024u) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)smem);
    if (e != hipSuccess) return e;
  }
  const int n = 9 * (wa.m - 1);
  const long long per_launch = (long long)kMaxGroupsPerLaunch * plan.nt;
  if (MMA && wa.B > per_launch) return hipErrorInvalidValue;   // (the optimizer's state for 2^25 trajectories is 90 GB)
  for (long long b0 = 0; b0 < args.B; b0 += per_launch) {
    GtopKernelArgs<R> s = wa;
    s.B = (int)((args.B - b0) < per_launch ? (args.B - b0) : per_launch);
    s.x = wa.x + (size_t)b0 * n;
    s.Df = wa.Df + (size_t)b0 * 18;
    s.T = wa.T + (size_t)b0 * wa.t_stride;
    s.cost = wa.cost ? wa.cost + b0 : nullptr;
    s.grad = wa.grad ? wa.grad + (size_t)b0 * n : nullptr;
    const int groups = (s.B + plan.nt - 1) / plan.nt;
    const int per_xcd = (groups + 7) / 8;
    const int grid = 8 * per_xcd;   // the kernel deals its workgroups over 8 XCD-contiguous ranges
    // what every wavefront would otherwise work out in front of its first load: the groups per XCD, the last group
    // (the padding workgroups shadow it) and the bytes from one group's rows of x / T to the next's (the optimizer loop
    // reads x from its state and Df, T as fp64 rows by its own indices: it does not use the strides)
    const unsigned x_grp_bytes = (unsigned)((size_t)plan.nt * (size_t)n * sizeof(R));
    const unsigned T_grp_bytes = (unsigned)((size_t)plan.nt * (size_t)wa.t_stride * sizeof(R));
    MM sst = st;
    if constexpr (MOV) {   // the slice's rows of the start times
      if (sst.mk.t0) sst.mk.t0 += (size_t)b0 * (size_t)sst.mk.t0_stride;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * plan.nw), smem, stream, s.x, s.Df, s.T, s.B, s.m, s.t_stride, per_xcd,
                       groups - 1, x_grp_bytes, T_grp_bytes, s.sdf, s, GtopWaveConsts<R>{}, sst, GtopSetupConsts<R>{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

// The launchers.  In the reference-mode object (kReferenceObject) a plan that asks for the consistent gradient goes to
// the other object's launcher of the same name + _consistent — unless the launch has no collision term (:346): the two
// modes are then the same function and the reference body serves both.

template <typename R>
hipError_t GTOP_LAUNCHER(gtop_launch_eval)(const GtopKernelArgs<R> &args, const GtopEvalPlan &plan, bool dyn, hipStream_t stream) {
  if (kReferenceObject && plan.consistent && has_collision_term(args)) return gtop_launch_eval_consistent<R>(args, plan, dyn, stream);
  return launch_wave<R, GtopModeOf<GtopNoMma>>(args, mode_args(GtopNoMma{}), plan, dyn, stream);
}

// (Moving: GtopMoving, or GtopMovingPoly for a polynomial list — mov.poly, a launch argument: the bodies differ)
template <template <typename> class Moving = GtopMoving, typename Base>
static Moving<Base> moving_kernel_args(const Base &st, const GtopMovingArgs &mov) {
  Moving<Base> mm;
  static_cast<Base &>(mm) = st;
  mm.mk = GtopMovK{mov.rows, mov.t0, mov.nbox, mov.t0_stride};
  return mm;
}
hipError_t GTOP_LAUNCHER(gtop_launch_eval_moving)(const GtopKernelArgs<double> &args, const GtopEvalPlan &plan, bool dyn,
                                                  const GtopMovingArgs &mov, hipStream_t stream) {
  if (!mov.rows || mov.nbox < 1 || mov.nbox > GTOP_MOVING_MAX_BOXES) return hipErrorInvalidValue;
  if (kReferenceObject && plan.consistent && has_collision_term(args)) return gtop_launch_eval_moving_consistent(args, plan, dyn, mov, stream);
  if (mov.poly)
    return launch_wave<double, GtopModeOf<GtopMovingPoly<GtopNoMma>>>(args, mode_args(moving_kernel_args<GtopMovingPoly>(GtopNoMma{}, mov)), plan, dyn, stream);
  return launch_wave<double, GtopModeOf<GtopMoving<GtopNoMma>>>(args, mode_args(moving_kernel_args(GtopNoMma{}, mov)), plan, dyn, stream);
}
hipError_t GTOP_LAUNCHER(gtop_launch_eval_mma_moving)(const GtopKernelArgs<double> &args, const GtopMmaState &st,
                                                      const GtopEvalPlan &plan, bool dyn, const GtopMovingArgs &mov,
                                                      hipStream_t stream) {
  if (!mov.rows || mov.nbox < 1 || mov.nbox > GTOP_MOVING_MAX_BOXES) return hipErrorInvalidValue;
  if (plan.nt != 1) return hipErrorInvalidValue;
  if (kReferenceObject && plan.consistent && has_collision_term(args)) return gtop_launch_eval_mma_moving_consistent(args, st, plan, dyn, mov, stream);
  if (mov.poly)
    return launch_wave<double, GtopModeOf<GtopMovingPoly<GtopMmaState>>>(args, mode_args(moving_kernel_args<GtopMovingPoly>(st, mov)), plan, dyn, stream);
  return launch_wave<double, GtopModeOf<GtopMoving<GtopMmaState>>>(args, mode_args(moving_kernel_args(st, mov)), plan, dyn, stream);
}

// the optimizer loop: st.iters evaluations at st.xcur, each followed by the CCSA-MMA update, in one launch (fp64)
hipError_t GTOP_LAUNCHER(gtop_launch_eval_mma)(const GtopKernelArgs<double> &args, const GtopMmaState &st,
                                               const GtopEvalPlan &plan, bool dyn, hipStream_t stream) {
  if (plan.nw != 1 || plan.spl == 30 || plan.spl == 10 || (plan.nt != 1 && !(plan.nt == 2 && plan.spl == 6 && !plan.is_long))) return hipErrorInvalidValue;
  if (kReferenceObject && plan.consistent && has_collision_term(args)) return gtop_launch_eval_mma_consistent(args, st, plan, dyn, stream);
  return launch_wave<double, GtopModeOf<GtopMmaState>>(args, mode_args(st), plan, dyn, stream);
}
// the same loop with the evaluations in fp32 on the fp32 field: args.Df / args.T still point at fp64 rows (the state,
// the bounds, the update and the results are fp64; see the kernel's `In`), args.x / cost / grad are not read
hipError_t GTOP_LAUNCHER(gtop_launch_eval_mma)(const GtopKernelArgs<float> &args, const GtopMmaState &st,
                                               const GtopEvalPlan &plan, bool dyn, hipStream_t stream) {
  if (plan.nw != 1 || plan.spl == 30 || plan.spl == 10 || (plan.nt != 1 && !(plan.nt == 2 && plan.spl == 6 && !plan.is_long))) return hipErrorInvalidValue;
  if (kReferenceObject && plan.consistent && has_collision_term(args)) return gtop_launch_eval_mma_consistent(args, st, plan, dyn, stream);
  return launch_wave<float, GtopModeOf<GtopMmaState>>(args, mode_args(st), plan, dyn, stream);
}

#ifdef GTOP_STAMPS   // (the reference-mode object's: gtop_wave_kernel.h)
extern "C" int gtop_debug_read_stamps(unsigned long long *out /*4096*16*/) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gtop_stamps), sizeof(unsigned long long) * 4096 * 16);
}
#endif

template hipError_t GTOP_LAUNCHER(gtop_launch_eval)<double>(const GtopKernelArgs<double> &, const GtopEvalPlan &, bool, hipStream_t);
template hipError_t GTOP_LAUNCHER(gtop_launch_eval)<float>(const GtopKernelArgs<float> &, const GtopEvalPlan &, bool, hipStream_t);

// (here, not in gtop_push.hip, its other user: built with this file's KERNEL_FLAGS the kernel takes its argument preloaded)
#ifndef GTOP_CONSISTENT_TU
// Device-side clock stamp (gtop_device_clock_stamp): one lane reads the constant-rate wall clock (the counter the
// optimizer loop's maxtime rule uses) and folds it into minmax[0] = earliest, minmax[1] = latest stamp.  Captured as
// the first and the last node of a graph of evaluation launches, latest - earliest is the GPU's own time for the
// launches in between — no host clock, no profiler instrumentation in the measured interval.
namespace {
__global__ void __launch_bounds__(64) gtop_clock_stamp_kernel(unsigned long long *minmax) {
  if (threadIdx.x == 0) {
    const unsigned long long t = wall_clock64();
    atomicMin(minmax, t);
    atomicMax(minmax + 1, t);
  }
}
}  // namespace

hipError_t gtop_launch_clock_stamp(unsigned long long *minmax, hipStream_t stream) {
  hipLaunchKernelGGL(gtop_clock_stamp_kernel, dim3(1), dim3(64), 0, stream, minmax);
  return hipGetLastError();
}
#endif  // GTOP_CONSISTENT_TU
