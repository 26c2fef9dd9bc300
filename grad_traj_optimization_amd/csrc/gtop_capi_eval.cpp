// gtop_capi_eval.cpp — what launches the evaluation kernels: the evaluation entry points (host buffers, the NLopt
// callback, device buffers) and the batched optimizer (gtop_optimize_*).
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "gtop_ctx.h"

namespace {

constexpr size_t kPollDoubles = 16384;                   // outputs per call the completion poll scans (B <= 356 at m = 6)
constexpr double kPollSeconds = 2e-3;
constexpr size_t kZeroCopyDoubles = 1u << 17;   // (measured: 2x faster at B = 1, 1.5x at B = 1024, on par at B = 4096 x 45)
  // host-buffer batches up to this many free variables skip the staged copies

template <typename R>
void fill_args(const gtop_ctx *c, GtopKernelArgs<R> &a) {
  const GtopGrid &g = c->field.grid;
  a.nx = g.nx; a.ny = g.ny; a.nz = g.nz;
  for (int i = 0; i < 3; ++i) {
    a.origin[i] = (R)g.origin[i];
    a.lo[i] = (R)g.min_range[i] + (R)1e-4;   // sdf_map.cpp:56-57
    a.hi[i] = (R)g.max_range[i] - (R)1e-4;   // sdf_map.cpp:62-63
    // the same bounds for positions that are float values (the reference keeps pos in `float` locals): the smallest
    // float >= lo and the largest <= hi decide `p < lo` / `p > hi` exactly for every float p
    float lf = (float)a.lo[i], hf = (float)a.hi[i];
    if ((double)lf < (double)a.lo[i]) lf = std::nextafterf(lf, INFINITY);
    if ((double)hf > (double)a.hi[i]) hf = std::nextafterf(hf, -INFINITY);
    a.lo_f[i] = lf;
    a.hi_f[i] = hf;
  }
  a.res = (R)g.res;
  a.res_inv = (R)g.res_inv;
  for (int i = 0; i < 3; ++i) a.idx_origin[i] = g.origin[i];
  a.idx_half = 0.5 * g.res;
  a.idx_rinv = g.res_inv;
  const gtop_params &p = c->prm;
  a.ws = (R)p.ws; a.wc = (R)p.wc; a.alpha = (R)p.alpha; a.d0 = (R)p.d0;
  a.inv_r = (R)1 / (R)p.r;
  a.alpha_over_r = (R)p.alpha / (R)p.r;
  a.alpha_v = (R)p.alpha_v; a.r_v = (R)p.r_v; a.v0 = (R)p.v0;
  a.alpha_a = (R)p.alpha_a; a.r_a = (R)p.r_a; a.a0 = (R)p.a0;
  a.inv_r_v = p.r_v != 0.0 ? (R)1 / (R)p.r_v : (R)0;   // (r_v, r_a are only read with enable_dyn, which requires them non-zero)
  a.inv_r_a = p.r_a != 0.0 ? (R)1 / (R)p.r_a : (R)0;
  a.gv_scale = (R)p.alpha_v * a.inv_r_v;
  a.ga_scale = (R)p.alpha_a * a.inv_r_a;
  a.step = p.step;
}

// The kernel arguments of one launch: the context's field geometry and parameters in the arithmetic type R, and the
// call's own pointers and shape.
template <typename R>
GtopKernelArgs<R> kernel_args(const gtop_ctx *c, const R *sdf, int B, int m, const void *d_x, const void *d_Df,
                              const void *d_T, int t_stride, void *d_cost, void *d_grad) {
  GtopKernelArgs<R> a;
  fill_args(c, a);
  a.sdf = sdf;
  a.x = static_cast<const R *>(d_x);
  a.Df = static_cast<const R *>(d_Df);
  a.T = static_cast<const R *>(d_T);
  a.cost = static_cast<R *>(d_cost);
  a.grad = static_cast<R *>(d_grad);
  a.B = B; a.m = m; a.t_stride = t_stride;
  return a;
}

// One evaluation launch, with the moving-obstacle term or without as the context stands.  optimizer_plan: the geometry
// the optimizer's fused forms run (same bits); problem_B: the batch of gtop_set_problem when the evaluation is of its
// first B rows (gtop_eval_batch: a per-trajectory start-time list of that length serves them), 0 otherwise.
template <typename R>
int launch_eval(gtop_ctx *c, const R *sdf, int B, int m, const void *d_x, const void *d_Df, const void *d_T, int t_stride,
                void *d_cost, void *d_grad, hipStream_t stream, const GtopEvalPlan *optimizer_plan = nullptr,
                int problem_B = 0) {
  const bool moving = gtop_moving_active(c);
  GtopMovingArgs mov{};
  if (moving) {
    if (sizeof(R) == 4)
      return fail(c, GTOP_ERR_STATE, "fp32 evaluation with the moving-obstacle cost on and boxes set: the term is fp64 only");
    if (int rc = gtop_moving_args(c, B, problem_B, &mov)) return rc;
  }
  const GtopKernelArgs<R> a = kernel_args<R>(c, sdf, B, m, d_x, d_Df, d_T, t_stride, d_cost, d_grad);
  GtopEvalPlan plan;
  if (optimizer_plan) plan = *optimizer_plan;   // the geometry the optimizer's fused forms run: same bits
  else if (moving && !gtop_eval_plan_moving(B, m, c->spl, false, &plan))
    return fail(c, GTOP_ERR_INVALID, "moving-obstacle cost: no body for this launch geometry / length (samples_per_lane "
                                     "10 and 30, 3 with more than 6 segments; one wavefront's LDS: 227 segments)");
  else if (!moving && !gtop_eval_plan(B, m, sizeof(R), c->spl, false, &plan))
    return fail(c, GTOP_ERR_INVALID, "this many segments cannot be served (ten lanes per segment: up to 6 segments; "
                                     "one wavefront's LDS: 227)");
  plan.consistent = c->grad_mode == GTOP_GRADIENT_CONSISTENT;
  if constexpr (sizeof(R) == 8) {
    if (moving) {
      HIPCHK(c, gtop_launch_eval_moving(a, plan, c->prm.enable_dyn != 0, mov, stream));
      return GTOP_OK;
    }
  }
  HIPCHK(c, gtop_launch_eval<R>(a, plan, c->prm.enable_dyn != 0, stream));
  return GTOP_OK;
}

int check_eval_state(gtop_ctx *c) {
  if (!c->have_params) return fail(c, GTOP_ERR_STATE, "gtop_set_params has not been called");
  if (!c->field.have_grid) return fail(c, GTOP_ERR_STATE, "no distance field set");
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_eval_batch(gtop_ctx *c, int B, const double *x, double *cost, double *grad) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc = check_eval_state(c);
  if (rc) return rc;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem has not been called");
  if ((rc = c->field.need_records64(c))) return rc;
  if (B < 1 || B > c->B || !x || !cost || !grad)
    return fail(c, GTOP_ERR_INVALID, "eval_batch: 1 <= B <= problem batch, non-NULL buffers");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(c->m - 1);
  if ((size_t)B * n <= kZeroCopyDoubles) {
    // Small batches (the NLopt callback is B = 1): three staged copies cost more than the
    // evaluation.  The kernel reads x from, and writes cost and gradient to, pinned host
    // memory it can address directly — one launch and one synchronisation.
    const size_t bn = (size_t)B * n, need = 2 * bn + (size_t)B;
    // coherent (fine-grained) memory: the kernel's stores must reach host memory as they retire, not at the end of the
    // kernel — the completion poll below reads them while the kernel is still "running" for the runtime
    if (need > c->pin.capacity()) {
      HIPCHK(c, c->pin.reserve(need < 4096 ? 4096 : need));
      HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&c->pin_dev), c->pin.data(), 0));
    }
    double *pin = c->pin.data(), *dpin = c->pin_dev;
    std::memcpy(pin, x, bn * sizeof(double));
    // The serial caller's round trip (the NLopt callback, B = 1) is launch + 3.5 us of kernel + completion, and
    // most of the completion is the end-of-kernel protocol (cache release, completion signal, the runtime's wait).
    // Every output is stored exactly once, 8 bytes at a time, into coherent host memory: the slots are preset to a
    // NaN pattern no evaluation produces, and the call returns when none is left.  A kernel that does not finish
    // within kPollSeconds falls back to the stream synchronisation (which also reports a fault).
    const size_t nout = (size_t)B + bn;
    const bool poll = c->poll_completion && nout <= kPollDoubles;
    volatile uint64_t *out = reinterpret_cast<volatile uint64_t *>(pin + bn);
    if (poll)
      for (size_t i = 0; i < nout; ++i) out[i] = c->poll_sentinel;
    if ((rc = launch_eval<double>(c, c->field.rec64.data(), B, c->m, dpin, c->d_Df.data(), c->d_T.data(), c->t_stride, dpin + bn,
                                  dpin + bn + B, c->stream, nullptr, c->B)))
      return rc;
    bool done = false;
    if (poll) {
      const auto t0 = std::chrono::steady_clock::now();
      size_t i = 0;
      unsigned spins = 0;
      // A slot has landed when BOTH of its 32-bit halves differ from the sentinel's: an 8-byte store that reached
      // host memory as two dwords is then never taken half-written.  A genuine result that shares a half with the
      // sentinel (2^-32 per half) is merely never "seen": the call falls back to the stream wait, never returns a
      // wrong value.
      const uint32_t kLo = (uint32_t)c->poll_sentinel, kHi = (uint32_t)(c->poll_sentinel >> 32);
      while (i < nout) {
        const uint64_t v = out[i];
        if ((uint32_t)v != kLo && (uint32_t)(v >> 32) != kHi) { ++i; continue; }
        __builtin_ia32_pause();
        if ((++spins & 255u) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kPollSeconds)
          break;
      }
      done = i == nout;
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!done) HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(cost, pin + bn, (size_t)B * sizeof(double));
    std::memcpy(grad, pin + bn + B, bn * sizeof(double));
    return GTOP_OK;
  }
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_eval<double>(c, c->field.rec64.data(), B, c->m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride,
                                c->d_cost.data(), c->d_grad.data(), c->stream, nullptr, c->B)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(cost, c->d_cost.data(), (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(grad, c->d_grad.data(), (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

double gtop_cost_nlopt(unsigned n, const double *x, double *grad, void *vctx) try {
  gtop_ctx *c = static_cast<gtop_ctx *>(vctx);
  if (!c) return HUGE_VAL;
  const auto tb1 = std::chrono::steady_clock::now();
  c->iter_num++;   // grad_traj_optimizer.cpp:284
  if (c->B == 0 || n != 9u * (unsigned)(c->m - 1) || !x) {
    fail(c, GTOP_ERR_INVALID, "cost_nlopt: n does not match the problem (9(m-1)) or x is NULL");
    return HUGE_VAL;
  }
  double cost = HUGE_VAL;
  std::vector<double> gtmp;
  double *g = grad;
  if (!g) {   // the reference always computes the gradient (:426)
    gtmp.resize(n);
    g = gtmp.data();
  }
  if (gtop_eval_batch(c, 1, x, &cost, g) != GTOP_OK) return HUGE_VAL;
  const auto te1 = std::chrono::steady_clock::now();
  c->total_time += std::chrono::duration<double>(te1 - tb1).count();   // :436
  // best-so-far cost curve, :439-447
  c->vec_time.push_back(std::chrono::duration<double>(te1 - c->time_start).count());
  if (c->vec_cost.empty() || c->vec_cost.back() > cost)
    c->vec_cost.push_back(cost);
  else
    c->vec_cost.push_back(c->vec_cost.back());
  return cost;
} GTOP_CATCH_HUGE(static_cast<gtop_ctx *>(vctx))

int gtop_eval_device(gtop_ctx *c, int dtype, int B, int m, const void *d_x, const void *d_Df,
                     const void *d_T, int time_stride, void *d_cost, void *d_grad, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc = check_eval_state(c);
  if (rc) return rc;
  if (B < 0 || m < 2 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "eval_device: need B >= 0, m >= 2, time_stride in {0, m}");
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_cost || !d_grad) return fail(c, GTOP_ERR_INVALID, "eval_device: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (dtype == GTOP_F64) {
    if ((rc = c->field.need_records64(c))) return rc;
    return launch_eval<double>(c, c->field.rec64.data(), B, m, d_x, d_Df, d_T, time_stride, d_cost, d_grad, s);
  } else if (dtype == GTOP_F32) {
    if (gtop_moving_active(c))
      return fail(c, GTOP_ERR_STATE, "fp32 evaluation with the moving-obstacle cost on and boxes set: the term is fp64 only");
    if ((rc = c->field.need_records32(c, s))) return rc;
    return launch_eval<float>(c, c->field.rec32.data(), B, m, d_x, d_Df, d_T, time_stride, d_cost, d_grad, s);
  }
  return fail(c, GTOP_ERR_INVALID, "bad dtype");
} GTOP_CATCH_STATUS(c)


// Batched optimizer: max_evals rounds of {cost/gradient, MMA update} per trajectory on
// `stream` — one launch for the whole loop (fusion mode 2), one per round (1), or two
// per round (0); no host synchronisation inside.
// (problem_B: see moving_args — gtop_optimize_batch_ex runs the first B rows of the problem set)
// (hook: gtop_ctx.h, GtopRoundHook — the two-launch form whatever the fusion knob says, the hook between its launches)
static int optimize_device_impl(gtop_ctx *c, int B, int m, void *d_x, const void *d_Df, const void *d_T,
                                int time_stride, const void *d_lb, const void *d_ub, const gtop_stop *stop, void *d_minf,
                                int32_t *d_nevals, int32_t *d_code, void *hip_stream, int problem_B,
                                const GtopRoundHook *hook = nullptr) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc = check_eval_state(c);
  if (rc) return rc;
  if (!stop || stop->max_evals < 1 || stop->ftol_rel < 0 || stop->xtol_rel < 0 || stop->maxtime < 0)
    return fail(c, GTOP_ERR_INVALID, "optimize: stop rules need max_evals >= 1 and non-negative tolerances / maxtime");
  const int max_evals = stop->max_evals;
  if (B < 0 || m < 2 || (time_stride != 0 && time_stride != m))
    return fail(c, GTOP_ERR_INVALID, "optimize_device: need B >= 0, m >= 2, time_stride in {0, m}");
  if (B == 0) return GTOP_OK;
  if (!d_x || !d_Df || !d_T || !d_lb || !d_ub) return fail(c, GTOP_ERR_INVALID, "optimize_device: NULL buffer");
  if ((rc = c->field.need_records64(c))) return rc;
  // the moving-obstacle cost: fp64 evaluations only, and its own checks before anything is allocated or launched
  const bool moving = gtop_moving_active(c);
  GtopMovingArgs mov{};
  if (moving) {
    if (c->opt_dtype == GTOP_F32)
      return fail(c, GTOP_ERR_STATE, "optimize: fp32 evaluations with the moving-obstacle cost on and boxes set: the term is fp64 only");
    if ((rc = gtop_moving_args(c, B, problem_B, &mov))) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const size_t n = 9 * (size_t)(m - 1), bn = (size_t)B * n;
  HIPCHK(c, c->mma_vec.reserve(6 * bn));
  HIPCHK(c, c->mma_scal.reserve(5 * (size_t)B));
  HIPCHK(c, c->mma_int.reserve(3 * (size_t)B));
  HIPCHK(c, c->mma_f.reserve((size_t)B));
  HIPCHK(c, c->mma_g.reserve(bn));
  GtopMmaState st;
  st.x = c->mma_vec.data(); st.xcur = st.x + bn; st.xprev = st.xcur + bn; st.xprevprev = st.xprev + bn;
  st.dfdx = st.xprevprev + bn; st.sigma = st.dfdx + bn;
  st.lb = static_cast<const double *>(d_lb);
  st.ub = static_cast<const double *>(d_ub);
  st.rho = c->mma_scal.data(); st.minf = st.rho + B; st.gval = st.minf + B; st.wval = st.gval + B; st.fprev = st.wval + B;
  st.k = c->mma_int.data(); st.state = st.k + B; st.nevals = st.state + B;
  st.ftol_rel = stop->ftol_rel;
  st.xtol_rel = stop->xtol_rel;
  st.max_ticks = (long long)(stop->maxtime * 1e8);   // wall_clock64(): 100 MHz
  st.x0_init = nullptr;
  st.out_x = st.out_minf = nullptr;
  st.out_code = st.out_nevals = nullptr;
  // one geometry in every launch form; the whole loop in one launch by default (fusion mode 2)
  GtopEvalPlan plan;
  const bool f32 = c->opt_dtype == GTOP_F32;   // gtop_set_optimizer_precision: see below
  const size_t eval_elem = f32 ? sizeof(float) : sizeof(double);
  const int opt_spl = (c->spl == 30 || c->spl == 10) ? 0 : c->spl;   // (three lanes / one lane per segment: plain-evaluation geometries)
  bool planned = moving ? gtop_eval_plan_moving(B, m, opt_spl, /*for_optimizer=*/true, &plan)
                        : gtop_eval_plan(B, m, eval_elem, opt_spl, /*for_optimizer=*/true, &plan);
  // (two trajectories per wavefront with the velocity / acceleration block compiled in: the fp32 loop would spill —
  // enable_dyn keeps the loop at ten lanes per segment, one trajectory per wavefront)
  if (!moving && planned && plan.nt == 2 && c->prm.enable_dyn != 0) planned = gtop_eval_plan(B, m, eval_elem, 3, true, &plan);
  if (!planned)
    return fail(c, GTOP_ERR_INVALID, "optimize: this many segments cannot be served (ten lanes per segment: up to 6; "
                                     "one wavefront's LDS with the optimizer's state: 118)");
  plan.consistent = c->grad_mode == GTOP_GRADIENT_CONSISTENT;   // (the separate-update form's evaluations take the plan too)
  const bool fused = !hook && c->fuse_mma != 0;
  const bool resident = !hook && c->fuse_mma == 2;   // one launch runs all max_evals evaluations of every trajectory
  st.iters = resident ? max_evals : 1;
  st.max_evals = max_evals;
  GtopKernelArgs<double> a =
      kernel_args<double>(c, c->field.rec64.data(), B, m, st.xcur, d_Df, d_T, time_stride, c->mma_f.data(), c->mma_g.data());
  const bool dyn = c->prm.enable_dyn != 0;
  // gtop_set_optimizer_precision(GTOP_F32): the same loop with its evaluations in fp32 on the fp32 field; the state,
  // the bounds, Df, T, the update and every result stay fp64 (the kernel converts as it reads its inputs from LDS)
  GtopKernelArgs<float> a32;
  if (f32) {
    if (!fused) return fail(c, GTOP_ERR_INVALID, "optimize: fp32 evaluations need a fused launch form (gtop_set_optimizer_fusion 1 or 2)");
    if ((rc = c->field.need_records32(c, s))) return rc;
    // (the loop reads its trial point from LDS; Df and T are fp64 rows, staged by the kernel as such)
    a32 = kernel_args<float>(c, c->field.rec32.data(), B, m, nullptr, d_Df, d_T, time_stride, nullptr, nullptr);
  }
  auto launch_loop = [&]() -> hipError_t {
    if (moving) return gtop_launch_eval_mma_moving(a, st, plan, dyn, mov, s);
    return f32 ? gtop_launch_eval_mma(a32, st, plan, dyn, s) : gtop_launch_eval_mma(a, st, plan, dyn, s);
  };
  // The whole optimisation as ONE launch: the loop initialises the state from d_x itself and writes the results where
  // they are wanted — no init kernel in front, no copies and no finish kernel behind (each a stream operation of its
  // own: 75 -> ~25 us of fixed cost per call).
  if (resident) {
    st.x0_init = static_cast<const double *>(d_x);
    // the kernel reads the start points row by row before it writes anything there, and a row is read and written
    // by the same wavefront: d_x can be the output as well
    st.out_x = static_cast<double *>(d_x);
    st.out_minf = static_cast<double *>(d_minf);
    st.out_code = d_code;
    st.out_nevals = d_nevals;
    HIPCHK(c, launch_loop());
    return GTOP_OK;
  }
  HIPCHK(c, gtop_launch_mma_init(st, B, (int)n, static_cast<const double *>(d_x), s));
  for (int it = 0; it < max_evals; ++it) {
    if (fused) {
      // one launch per iteration: the evaluation kernel runs the MMA update as its epilogue
      HIPCHK(c, launch_loop());
    } else {
      if ((rc = launch_eval<double>(c, a.sdf, B, m, st.xcur, d_Df, d_T, time_stride, a.cost, a.grad, s, &plan,
                                    problem_B)))   // the geometry the fused modes run: same bits
        return rc;
      if (hook && (rc = hook->round(hook->user, c, st.xcur, c->mma_f.data(), c->mma_g.data(), s))) return rc;
      HIPCHK(c, gtop_launch_mma_update(st, B, (int)n, c->mma_f.data(), c->mma_g.data(), s));
    }
  }
  HIPCHK(c, hipMemcpyAsync(d_x, st.x, bn * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (d_minf) HIPCHK(c, hipMemcpyAsync(d_minf, st.minf, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIPCHK(c, gtop_launch_mma_finish(st, B, d_code, d_nevals, s));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_optimize_device_ex(gtop_ctx *c, int B, int m, void *d_x, const void *d_Df, const void *d_T,
                            int time_stride, const void *d_lb, const void *d_ub, const gtop_stop *stop, void *d_minf,
                            int32_t *d_nevals, int32_t *d_code, void *hip_stream) {
  return optimize_device_impl(c, B, m, d_x, d_Df, d_T, time_stride, d_lb, d_ub, stop, d_minf, d_nevals, d_code, hip_stream, 0);
}

}  // extern "C"

// (gtop_ctx.h)
int gtop_optimize_rounds(gtop_ctx *c, int B, int m, void *d_x, const void *d_Df, const void *d_T, int time_stride,
                         const void *d_lb, const void *d_ub, int evals, void *d_minf, void *hip_stream, int problem_B,
                         const GtopRoundHook *hook) {
  const gtop_stop stop = {evals, 0.0, 0.0, 0.0};
  return optimize_device_impl(c, B, m, d_x, d_Df, d_T, time_stride, d_lb, d_ub, &stop, d_minf, nullptr, nullptr,
                              hip_stream, problem_B, hook);
}

extern "C" {

int gtop_optimize_device(gtop_ctx *c, int B, int m, void *d_x, const void *d_Df, const void *d_T,
                         int time_stride, const void *d_lb, const void *d_ub, int max_evals, void *d_minf,
                         void *hip_stream) try {
  const gtop_stop stop = {max_evals, 0.0, 0.0, 0.0};
  return gtop_optimize_device_ex(c, B, m, d_x, d_Df, d_T, time_stride, d_lb, d_ub, &stop, d_minf, nullptr, nullptr,
                                 hip_stream);
} GTOP_CATCH_STATUS(c)

int gtop_optimize_batch_ex(gtop_ctx *c, int B, double *x, const double *lb, const double *ub, const gtop_stop *stop,
                           double *min_cost, int32_t *nevals, int32_t *code) try {
  if (!c) return GTOP_ERR_INVALID;
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem has not been called");
  if (B < 1 || B > c->B || !x || !lb || !ub || !stop)
    return fail(c, GTOP_ERR_INVALID, "optimize_batch: 1 <= B <= problem batch, non-NULL buffers and stop rules");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = 9 * (size_t)(c->m - 1), bn = (size_t)B * n;
  int rc;
  HIPCHK(c, c->mma_lb.reserve(bn));
  HIPCHK(c, c->mma_ub.reserve(bn));
  HIPCHK(c, c->mma_res.reserve(2 * (size_t)B));
  HIPCHK(c, hipMemcpyAsync(c->d_x.data(), x, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->mma_lb.data(), lb, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->mma_ub.data(), ub, bn * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int *res = c->mma_res.data();
  if ((rc = optimize_device_impl(c, B, c->m, c->d_x.data(), c->d_Df.data(), c->d_T.data(), c->t_stride, c->mma_lb.data(),
                                 c->mma_ub.data(), stop, c->d_cost.data(), res, res + B, c->stream, c->B)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(x, c->d_x.data(), bn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (min_cost)
    HIPCHK(c, hipMemcpyAsync(min_cost, c->d_cost.data(), (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (nevals)
    HIPCHK(c, hipMemcpyAsync(nevals, res, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (code)
    HIPCHK(c, hipMemcpyAsync(code, res + B, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_optimize_batch(gtop_ctx *c, int B, double *x, const double *lb, const double *ub, int max_evals,
                        double *min_cost) try {
  const gtop_stop stop = {max_evals, 0.0, 0.0, 0.0};
  return gtop_optimize_batch_ex(c, B, x, lb, ub, &stop, min_cost, nullptr, nullptr);
} GTOP_CATCH_STATUS(c)

}  // extern "C"
