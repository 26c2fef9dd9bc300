// gtop_ctx.h — the context behind the C-ABI of include/gtop.h and what the files that implement it share: the error
// helpers, the distance field's state, and the few functions one file's entry points need from another's.  Private to
// the gtop_capi*.cpp files:
//   gtop_capi.cpp          the context's life, parameters, knobs, statistics, device clock, push, shared memory
//   gtop_capi_field.cpp    the distance field: uploads, the ESDF builder, window updates, the corner records
//   gtop_capi_problem.cpp  the problem set, path set-up, trajectory post-processing, default bounds
//   gtop_capi_eval.cpp     the evaluation entry points and the batched optimizer
//   gtop_capi_boxes.cpp    moving boxes (both list kinds), the cost switch, start times, distance queries
//   gtop_capi_report.cpp   the sampled reports (whole and per segment), both selections, both certificates
//   gtop_capi_remedy.cpp   the remedies for a row that fails: segment-time reallocation, waypoint insertion
//   gtop_capi_kinematics.cpp  the companion header include/gtop_kinematics.h: the kinematic certificate, its selection
//   gtop_capi_separation.cpp  the companion header include/gtop_separation.h: pairwise separation, distinct candidates
//   gtop_capi_separation_certificate.cpp  include/gtop_separation_certificate.h: the certificate of pairwise separation
//   gtop_capi_prediction.cpp  include/gtop_prediction.h: predictions fitted from histories, the box list's refresh
//   gtop_capi_time.cpp        include/gtop_time.h: the segment-time gradient, the optimizer of the time allocation
//   gtop_capi_swarm.cpp       include/gtop_swarm.h: the swarm separation cost, its gradient, the swarm optimizer
//   gtop_capi_joint.cpp       include/gtop_joint.h: the joint gradient over x and T, the joint optimizer
// Host-side only: they own device buffers, fill kernel arguments, launch.  There is deliberately no CPU code path:
// without a gfx950 device every entry point fails (GTOP_ERR_NO_DEVICE).
#ifndef GTOP_CTX_H_
#define GTOP_CTX_H_

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "gtop.h"
#include "gtop_devbuf.h"
#include "gtop_guard.h"
#include "gtop_kernels.h"

struct gtop_ctx;

// The distance field and everything derived from it.  sdf64 is the BOUNDARY copy, z fastest (src/sdf_map.cpp:172-173):
// what gtop_set_sdf uploads, the ESDF builder writes, gtop_get_sdf returns and the coarse voxel query reads; `own`'s
// buffer, or borrowed from gtop_set_sdf_device(GTOP_F64).  sdf32b is a borrowed fp32 field (gtop_set_sdf_device(GTOP_F32);
// no fp64 copy then).  What the lookups of every kernel read are the CORNER RECORDS derived from it (gtop_records.hip,
// DESIGN.md §4), always owned: rec64 and rec32.  rec64 is rebuilt wherever the field changes.  The fp32 records of a
// rebuilt field: gtop_update_sdf_map (host points, synchronous) defers them to the first fp32 evaluation unless one has
// been seen on this context (`fp32_in_use`, sticky), because they are a third of the pass's writes;
// gtop_update_sdf_map_device (asynchronous, capturable into a hipGraph) always builds them behind the fp64 ones, so
// that a REPLAY of the captured rebuild — which never passes through this host code again — leaves both current.
// The entry points go through the operations below and read `grid`, `sdf64`, the records and the signs; the flags are
// the operations' own.
struct GtopField {
  GtopGrid grid{};
  bool have_grid = false;
  GtopDevBuf<double> own;
  double *sdf64 = nullptr;
  const float *sdf32b = nullptr;
  GtopDevBuf<double> rec64;   // 4 values per record
  GtopDevBuf<float> rec32;
  // gtop_set_field_sign: the sign of the NEXT whole-map build (sign_next, depth_next) and of the resident field
  int sign_next = 0, sign = 0;
  double depth_next = 0.0, depth = 0.0;   // max_depth as given (0 = 10000)

  bool owned() const { return sdf64 && sdf64 == own.data(); }
  bool records64_current() const { return have_grid && rec64_ok; }
  // a window is built in the resident field's sign: one changed since needs a whole-map build first
  bool sign_pending() const { return sign_next != sign || (sign_next && depth_next != depth); }

  // the two questions an entry point asks before it launches; each sets its error text
  int need_records64(gtop_ctx *c) const;   // the fp64 corner records hold the current field
  int need_boundary(gtop_ctx *c) const;    // an fp64 boundary copy is resident

  // the geometry of the field to come (checked); nothing else changes
  int set_grid(gtop_ctx *c, int nx, int ny, int nz, const double origin[3], const double *map_size, double res);
  // an owned boundary copy and the records of `grid`, allocated up front: a captured map rebuild must not allocate, and
  // the first fp32 evaluation may come from inside a capture.  A failure leaves no grid.
  int make_owned(gtop_ctx *c);
  // a new fp64 field is in sdf64 as of stream `s`, whole (it takes the sign in force) or in the voxel box [vlo, vhi]:
  // the fp64 records follow on `s`, the fp32 ones with them where this context's rule says so (convert_now: the
  // capturable device entries), otherwise they go stale and the first fp32 use builds them
  int arrived(gtop_ctx *c, hipStream_t s, bool convert_now, const int *vlo = nullptr, const int *vhi = nullptr);
  // a caller's device buffer becomes the field in place (GTOP_F64: the boundary copy; GTOP_F32: fp32 records only)
  int borrow(gtop_ctx *c, int dtype, const void *dist_dev, hipStream_t s);
  // the fp32 records, current, before an fp32 use enqueued on stream `s`
  int need_records32(gtop_ctx *c, hipStream_t s);
  void keep_fp32(bool keep);   // gtop_set_field_precisions: 0 = fp64 records only (fp32 evaluations refused)
  void release();              // no field resident (the record buffers stay: grow-only)

 private:
  int reserve_records(gtop_ctx *c, hipError_t e = hipSuccess);
  bool rec64_ok = false;   // the records hold the current field
  // the fp32 records: none of this field, to be rebuilt from sdf64 before the next fp32 use, or holding the field
  enum class Rec32 { absent, stale, current } rec32_state = Rec32::absent;
  bool fp32_in_use = false;
  bool fp32_wanted = true;
};

struct gtop_ctx {
  int device = 0;
  int simds = 0;   // 4 per compute unit: sizes the trajectory report's launch
  std::string err;
  hipStream_t stream = nullptr;   // used by the host-pointer entry points

  gtop_params prm{};
  bool have_params = false;

  GtopField field;

  // ESDF construction workspace
  GtopDevBuf<uint8_t> occ;
  GtopDevBuf<int> tmp1, tmp2, rows;
  GtopDevBuf<uint8_t> win_occ;    // gtop_update_sdf_map_window: the window's occupancy / distances as a compact grid
  GtopDevBuf<double> win_dist;
  GtopDevBuf<double> d_pts;       // obstacle points of the host-pointer map updates; gtop_set_paths stages its waypoints here

  GtopDevBuf<double> boxes;  // moving boxes: p0 | vel | scale, nbox x 3 each; a polynomial list: its [nbox][kBoxRowPoly] rows
  int nbox = 0;
  int box_kind = GTOP_BOXES_CONST_VEL;   // which of the two the one list is (gtop_set_moving_box_polynomials)
  // the moving-obstacle cost (gtop_set_moving_cost): the box list as the evaluation kernels read it — [nbox][9] rows
  // p0, vel, scale / 2, or the [nbox][kBoxRowPoly] rows of a polynomial list, in a buffer of GTOP_MOVING_COST_MAX_BOXES
  // rows of the wider form allocated once (its address is what a captured launch holds) and rewritten by
  // gtop_set_moving_boxes / gtop_set_moving_box_polynomials — and the start times on the boxes' clock
  int moving_cost = 0;
  int grad_mode = GTOP_GRADIENT_REFERENCE;   // gtop_set_gradient_mode: read by every evaluation / optimizer call as it is made
  GtopDevBuf<double> box_rows;
  bool box_rows_ok = false;        // the list fits and every box is finite with a non-negative extent
  const double *t0_dev = nullptr;  // count > 0: t0_own's buffer, or borrowed
  GtopDevBuf<double> t0_own;
  int t0_count = 0;
  GtopDevBuf<unsigned char> sel_part;  // gtop_select_best_device: the partial results of its first stage (allocated at
                                       // gtop_create: the entry point itself must not allocate)
  GtopDevBuf<double> val_rep;  // gtop_validate_batch staging: report | cost, then pass and best behind them
  GtopDevBuf<double> seg_rep;  // gtop_validate_segments / gtop_reallocate_times staging: segment report | T_out;
                               // gtop_insert_waypoints': when | lb | ub | x_out | T_out | lb_out | ub_out | info;
                               // gtop_time_gradient_batch's: cost | gT | parts; gtop_optimize_times': T_lo | T_out | info
  GtopDevBuf<double> sep_stage;  // gtop_separation_batch staging: pair_min | pair_max | rows | the launches' workspace
  GtopDevBuf<double> swarm_stage;  // gtop_swarm_gradient_batch staging: the frozen rows' coefficients | S | grad | active |
                                   // the launches' workspace; gtop_optimize_swarm's: joint | the workspace
  GtopDevBuf<double> sepcert_stage;  // gtop_certify_separation_batch staging: pairs | rows | the launches' workspace
  GtopDevBuf<double> d_q;      // host-API staging of gtop_edt_query: pos | time | dist | grad; gtop_trajectory_samples'
                               // sample scratch too
  GtopPinnedBuf<double> pin;   // device-visible host staging for small host-buffer evaluations: x | cost | grad
  double *pin_dev = nullptr;   // its device address
  bool poll_completion = true;   // GTOP_POLL_COMPLETION=0: always wait through the stream (gtop_eval_batch)
  uint64_t poll_sentinel = 0;    // preset of the polled output slots (GTOP_POLL_SENTINEL=<hex> overrides: tests)

  // problem set by gtop_set_problem
  int B = 0, m = 0, t_stride = 0;
  GtopDevBuf<double> d_T, d_Df, d_x, d_cost, d_grad;

  // batched optimizer workspace (gtop_optimize_*)
  GtopDevBuf<double> mma_vec;    // 6 x [B][n]
  GtopDevBuf<double> mma_scal;   // 5 x [B]
  GtopDevBuf<int> mma_int;       // 3 x [B]
  GtopDevBuf<double> mma_f, mma_lb, mma_ub;
  GtopDevBuf<double> mma_g;      // the optimizer's gradients; the coefficient scratch of the post-processing entries too
  GtopDevBuf<int> mma_res;       // nevals | code of gtop_optimize_batch_ex, 2 x [B]

  int spl = 0;     // samples per lane: 0 = auto, 3, 6, 10 or 30 (gtop_set_launch_geometry)
  int opt_dtype = GTOP_F64;   // gtop_set_optimizer_precision: the arithmetic of the evaluations inside the batched optimizer
  int fuse_mma = 2;         // optimizer: 0 separate update launch, 1 update fused into the evaluation kernel,
                            //            2 (default) the whole loop in one launch (tuning/debug knob)

  // bookkeeping of the callback (grad_traj_optimizer.cpp:284, :436, :439-447)
  int64_t iter_num = 0;
  double total_time = 0.0;
  std::vector<double> vec_cost, vec_time;
  std::chrono::steady_clock::time_point time_start = std::chrono::steady_clock::now();

  // (the buffers free themselves behind this: destroyed with the context's device current)
  ~gtop_ctx() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// error text of a failed gtop_create (there is no context to hold it yet); defined in gtop_capi.cpp
extern thread_local std::string gtop_create_err;

static inline int fail(gtop_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  else gtop_create_err = msg;
  return code;
}

// what an exception caught at the boundary leaves behind (gtop_guard.h); must not throw itself
static inline void gtop_note_exception(gtop_ctx *c, const char *what) noexcept {
  try {
    fail(c, GTOP_ERR_INTERNAL, std::string("exception caught at the C boundary: ") + what);
  } catch (...) {
  }
}
#define GTOP_CATCH_STATUS(c) GTOP_CATCH_WITH(gtop_note_exception, c, GTOP_ERR_INTERNAL)
#define GTOP_CATCH_HUGE(c) GTOP_CATCH_WITH(gtop_note_exception, c, HUGE_VAL)

#define HIPCHK(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(ctx, GTOP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// ---- the moving boxes, as the evaluation launches of gtop_capi_eval.cpp see them (gtop_capi_boxes.cpp) ----
// The moving-obstacle cost is in force: switched on and at least one box set (without boxes the static kernels run).
static inline bool gtop_moving_active(const gtop_ctx *c) { return c->moving_cost != 0 && c->nbox > 0; }
// The start-time list serves a launch of B trajectories: one shared value, one per trajectory, or — problem_B: the
// batch of gtop_set_problem when the launch is of its first B rows, 0 otherwise — one per row of the problem set.
static inline bool gtop_start_times_fit(const gtop_ctx *c, int B, int problem_B) {
  return c->t0_count <= 1 || c->t0_count == B || c->t0_count == problem_B;
}
// The start times as a launch takes them: NULL when none are set (or the launch reads no boxes), else the list and its
// stride (0: one value shared by the batch).
struct GtopStartTimes {
  const double *t0;
  int stride;
};
static inline GtopStartTimes gtop_start_times(const gtop_ctx *c, bool boxes = true) {
  return {(boxes && c->t0_count > 0) ? c->t0_dev : nullptr, c->t0_count > 1 ? 1 : 0};
}
// What a moving-mode launch of B trajectories hands the kernels; the checks every road shares.
int gtop_moving_args(gtop_ctx *c, int B, int problem_B, GtopMovingArgs *mov);
// the first `count` boxes of the list as the query, report and certificate launchers take it (gtop_kernels.h)
static inline GtopBoxList gtop_box_list(const gtop_ctx *c, int count) {
  const double *b = c->boxes.data();
  const size_t n3 = (size_t)c->nbox * 3;
  if (c->box_kind == GTOP_BOXES_POLYNOMIAL) return {GTOP_BOX_LIST_POLYNOMIAL, count, nullptr, nullptr, nullptr, b};
  return {GTOP_BOX_LIST_CONST_VEL, count, b, b + n3, b + 2 * n3, nullptr};
}

// ---- the host forms over the problem set (gtop_capi_problem.cpp, _report.cpp, _remedy.cpp) ----
// How every one of them opens: a problem is set ...
static inline int gtop_problem_set(gtop_ctx *c) {
  if (c->B == 0) return fail(c, GTOP_ERR_STATE, "gtop_set_problem / gtop_set_paths has not been called");
  return GTOP_OK;
}
// ... and the call is of its first B rows with the buffers the form requires (`given`); `what`: the entry's own text.
static inline int gtop_problem_rows(gtop_ctx *c, int B, bool given, const char *what) {
  if (int rc = gtop_problem_set(c)) return rc;
  if (B < 1 || B > c->B || !given) return fail(c, GTOP_ERR_INVALID, what);
  return GTOP_OK;
}
// x of the problem's first B rows -> d_x -> their coefficients, left in mma_g (the coefficient scratch); no
// synchronisation (gtop_capi_problem.cpp)
int gtop_stage_coefficients(gtop_ctx *c, int B, const double *x);
// What a sampled report of B rows asks of its arguments and of the context, before anything is staged or launched;
// problem_B as gtop_start_times_fit's (gtop_capi_report.cpp)
int gtop_validate_ready(gtop_ctx *c, int B, int m, int time_stride, double dt_sample, const gtop_limits *lim, int problem_B);
// x of the problem's first B rows -> their coefficients -> the segment report in seg_rep (room for T_out behind it); no
// synchronisation (gtop_capi_report.cpp)
int gtop_segments_staged(gtop_ctx *c, int B, const double *x, double dt_sample, const gtop_limits *limits);
// The selection of every family (gtop_capi_report.cpp): 0 the rows that pass the report, 1 with the clearance
// certificate's `require`, 2 with the kinematic certificate's too (d_cert optional then); the checks, then two launches
int gtop_select_on_stream(gtop_ctx *c, int family, int B, const void *d_report, const void *d_cert, const void *d_kin,
                          const void *d_cost, const gtop_limits *limits, int require, void *d_pass, void *d_best,
                          void *hip_stream);
// The ONE host path of the certificates (gtop_capi_report.cpp): the problem's first B rows at x -> their coefficients
// -> `launch` on the context's stream into val_rep -> rows [B][row_cols] and, where segs is given, segs
// [B][m][seg_cols] on the host.  `ready` states the entry's rules before anything is staged; `job` is the entry's own
// (its options); rows_text: its opening refusal; given: the host buffers the form requires are there.
typedef int (*gtop_certificate_ready_fn)(gtop_ctx *c, int B, const void *job);
typedef int (*gtop_certificate_launch_fn)(gtop_ctx *c, int B, const void *job, double *d_rows, double *d_segs);
int gtop_certificate_host(gtop_ctx *c, const char *rows_text, int B, const double *x, bool given, const void *job,
                          gtop_certificate_ready_fn ready, gtop_certificate_launch_fn launch, int row_cols, double *rows,
                          int seg_cols, double *segs);


// ---- the batched optimizer with a term of the caller's between its two launches (gtop_capi_eval.cpp) ----
// Called once per round of the two-launch form, after the context's evaluation has written f [B] and grad [B][n] at the
// trial points xcur [B][n] and before the MMA update reads them: it may enqueue launches on `stream` that ADD to f and
// grad.  A status other than GTOP_OK ends the call with it.
struct GtopRoundHook {
  int (*round)(void *user, gtop_ctx *c, const double *d_xcur, double *d_f, double *d_grad, hipStream_t stream);
  void *user;
};
// gtop_optimize_device_ex with {evals, 0, 0, 0} as its stop rules; with a hook it takes the two-launch form whatever
// gtop_set_optimizer_fusion says (the context's state, mma_f and mma_g included, grows as for that call).  Without a
// hook it enqueues exactly what gtop_optimize_device_ex enqueues.
int gtop_optimize_rounds(gtop_ctx *c, int B, int m, void *d_x, const void *d_Df, const void *d_T, int time_stride,
                         const void *d_lb, const void *d_ub, int evals, void *d_minf, void *hip_stream, int problem_B,
                         const GtopRoundHook *hook);

#endif  // GTOP_CTX_H_
