// gtop_capi.cpp — the C-ABI of include/gtop.h on top of the gfx950 kernels, first part: the context's life, its
// parameters, knobs and statistics, the device clock, the push and the buffers another process can map.  The other
// parts and what they share: gtop_ctx.h.
#include <cstdlib>
#include <cstring>
#include <new>

#include "gtop_ctx.h"

#define GTOP_ABI_VERSION 12  // 12: gtop_insert_waypoints_device, gtop_insert_waypoints
                             // 11: gtop_certify_moving_device, gtop_certify_moving_batch
                             // 10: gtop_certify_trajectories_device, gtop_certify_batch, gtop_select_best_certified_device
                             // 9: gtop_validate_segments[_device], gtop_reallocate_times[_device]
                             // 8: gtop_min_jerk_start_device, gtop_min_jerk_start
                             // 7: gtop_set_moving_box_polynomials, gtop_get_moving_box_kind, gtop_box_polynomial_centres
                             // 6: gtop_set_gradient_mode, gtop_get_gradient_mode, gtop_group_set_gradient_mode
                             // 5: gtop_validate_trajectories_device, gtop_select_best_device, gtop_validate_batch
                             // 4: gtop_set_moving_cost, gtop_get_moving_cost, gtop_set_start_times, gtop_set_start_times_device
                             // 3: gtop_set_field_sign, gtop_get_field_sign, gtop_group_set_field_sign
                             // 2: gtop_update_sdf_map_window*, gtop_set_field_precisions, gtop_device_clock_*, gtop_group_gather_note, GTOP_ERR_INTERNAL

thread_local std::string gtop_create_err;

static constexpr uint64_t kPollSentinel = 0x7ff8dead5eed0badull;   // a quiet NaN with a payload the hardware never generates

extern "C" {

int gtop_abi_version(void) { return GTOP_ABI_VERSION; }

int gtop_create(gtop_ctx **out, int device) try {
  if (!out) return fail(nullptr, GTOP_ERR_INVALID, "gtop_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, GTOP_ERR_NO_DEVICE,
                std::string("gtop_create: no HIP device (hipGetDeviceCount: ") + hipGetErrorString(e) + ")");
  if (device < 0 || device >= ndev) return fail(nullptr, GTOP_ERR_INVALID, "gtop_create: device ordinal out of range");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
    return fail(nullptr, GTOP_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)   // the code objects are gfx950 only
    return fail(nullptr, GTOP_ERR_NO_DEVICE, std::string("gtop_create: device is ") + prop.gcnArchName + ", need gfx950");
  if ((e = hipSetDevice(device)) != hipSuccess)
    return fail(nullptr, GTOP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  gtop_ctx *c = new (std::nothrow) gtop_ctx();   // (its destructor undoes whatever of the rest was made)
  if (!c) return fail(nullptr, GTOP_ERR_INVALID, "gtop_create: out of memory");
  c->device = device;
  c->simds = 4 * prop.multiProcessorCount;
  if (const char *pc = std::getenv("GTOP_POLL_COMPLETION")) c->poll_completion = std::atoi(pc) != 0;
  c->poll_sentinel = kPollSentinel;
  if (const char *ps = std::getenv("GTOP_POLL_SENTINEL")) c->poll_sentinel = std::strtoull(ps, nullptr, 16);
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
    delete c;
    return fail(nullptr, GTOP_ERR_HIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
  }
  if ((e = c->sel_part.reserve((size_t)GTOP_SELECT_PARTIALS * GTOP_SELECT_PARTIAL_BYTES)) != hipSuccess) {
    delete c;
    return fail(nullptr, GTOP_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  *out = c;
  return GTOP_OK;
} GTOP_CATCH_STATUS(nullptr)

int gtop_destroy(gtop_ctx *c) try {
  if (!c) return GTOP_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;   // the stream, then every buffer
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

const char *gtop_last_error(const gtop_ctx *c) { return c ? c->err.c_str() : gtop_create_err.c_str(); }

int gtop_set_params(gtop_ctx *c, const gtop_params *p) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!p) return fail(c, GTOP_ERR_INVALID, "params is NULL");
  if (p->step < 0 || p->step > 2)   // grad_traj_optimizer.cpp:129-131
    return fail(c, GTOP_ERR_INVALID, "step number error, step should be 0, 1 or 2");
  if (p->r == 0.0) return fail(c, GTOP_ERR_INVALID, "r must be non-zero");
  if (p->enable_dyn && (p->r_v == 0.0 || p->r_a == 0.0))
    return fail(c, GTOP_ERR_INVALID, "r_v and r_a must be non-zero when enable_dyn is set");
  c->prm = *p;
  c->have_params = true;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_set_gradient_mode(gtop_ctx *c, int mode) {
  if (!c) return GTOP_ERR_INVALID;
  if (mode != GTOP_GRADIENT_REFERENCE && mode != GTOP_GRADIENT_CONSISTENT)
    return fail(c, GTOP_ERR_INVALID, "gradient mode: must be GTOP_GRADIENT_REFERENCE (0) or GTOP_GRADIENT_CONSISTENT (1)");
  c->grad_mode = mode;
  return GTOP_OK;
}

int gtop_get_gradient_mode(const gtop_ctx *c, int *mode) {
  if (!c || !mode) return GTOP_ERR_INVALID;
  *mode = c->grad_mode;
  return GTOP_OK;
}

int gtop_get_stats(const gtop_ctx *c, int64_t *iter_num, double *total_time) {
  if (!c) return GTOP_ERR_INVALID;
  if (iter_num) *iter_num = c->iter_num;
  if (total_time) *total_time = c->total_time;
  return GTOP_OK;
}

int gtop_reset_stats(gtop_ctx *c) try {
  if (!c) return GTOP_ERR_INVALID;
  c->iter_num = 0;
  c->total_time = 0.0;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_get_cost_curve(const gtop_ctx *c, double *cost, double *time, int cap, int *count) {
  if (!c) return GTOP_ERR_INVALID;
  const int nn = (int)c->vec_cost.size();
  if (count) *count = nn;
  const int k = cap < nn ? cap : nn;
  for (int i = 0; i < k; ++i) {
    if (cost) cost[i] = c->vec_cost[i];
    if (time) time[i] = c->vec_time[i];
  }
  return GTOP_OK;
}

int gtop_clear_cost_curve(gtop_ctx *c) try {
  if (!c) return GTOP_ERR_INVALID;
  c->vec_cost.clear();   // grad_traj_optimizer.cpp:192-194
  c->vec_time.clear();
  c->time_start = std::chrono::steady_clock::now();
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- measurement aid: the device's own clock around enqueued work ----
int gtop_device_clock_stamp(gtop_ctx *c, void *d_minmax, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!d_minmax) return fail(c, GTOP_ERR_INVALID, "device_clock_stamp: NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_clock_stamp(static_cast<unsigned long long *>(d_minmax), static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// ---- SURVEY 8e's collective as point-to-point stores (gtop_push.hip) ----
int gtop_push_rows(gtop_ctx *c, const void *d_src, size_t bytes, void *const *d_dsts, int n_dsts, void *d_clock_minmax,
                   void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (n_dsts < 0 || n_dsts > GTOP_PUSH_MAX_DSTS || (bytes > 0 && n_dsts > 0 && (!d_src || !d_dsts)))
    return fail(c, GTOP_ERR_INVALID, "push_rows: 0 .. 16 destinations, non-NULL buffers");
  if ((bytes == 0 || n_dsts == 0) && !d_clock_minmax) return GTOP_OK;
  GtopPushDsts dsts{};
  if (reinterpret_cast<uintptr_t>(d_src) & 15u) return fail(c, GTOP_ERR_INVALID, "push_rows: source not 16-byte aligned");
  for (int k = 0; k < n_dsts; ++k) {
    if (!d_dsts[k] || (reinterpret_cast<uintptr_t>(d_dsts[k]) & 15u))
      return fail(c, GTOP_ERR_INVALID, "push_rows: a destination is NULL or not 16-byte aligned");
    dsts.p[k] = d_dsts[k];
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtop_launch_push_rows(d_src, bytes, dsts, n_dsts, static_cast<unsigned long long *>(d_clock_minmax),
                                  static_cast<hipStream_t>(hip_stream)));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

// Buffers another process can map: plain hipMalloc allocations (an IPC handle names a whole allocation: a
// sub-allocation of a caching allocator would not do) exported / opened with HIP's IPC calls.  A peer's buffer is
// opened with THIS context's device current and lazy peer access: the mapping is made for the device whose kernels
// will store into it (what RCCL's own point-to-point transport does).
int gtop_shared_alloc(gtop_ctx *c, size_t bytes, void **d_ptr, unsigned char handle[GTOP_IPC_HANDLE_BYTES]) try {
  if (!c) return GTOP_ERR_INVALID;
  static_assert(sizeof(hipIpcMemHandle_t) <= GTOP_IPC_HANDLE_BYTES, "handle size");
  if (!d_ptr || !handle || bytes == 0) return fail(c, GTOP_ERR_INVALID, "shared_alloc: bytes > 0, non-NULL outputs");
  *d_ptr = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  void *p = nullptr;
  HIPCHK(c, hipMalloc(&p, bytes));
  hipError_t e = hipMemset(p, 0, bytes);
  hipIpcMemHandle_t h;
  if (e == hipSuccess) e = hipIpcGetMemHandle(&h, p);
  if (e != hipSuccess) {
    (void)hipFree(p);
    HIPCHK(c, e);
  }
  std::memset(handle, 0, GTOP_IPC_HANDLE_BYTES);
  std::memcpy(handle, &h, sizeof(h));
  *d_ptr = p;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_shared_open(gtop_ctx *c, const unsigned char handle[GTOP_IPC_HANDLE_BYTES], int owner_device, void **d_ptr) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!d_ptr || !handle) return fail(c, GTOP_ERR_INVALID, "shared_open: NULL argument");
  *d_ptr = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  // The owner's device, when the caller knows it: no mapping is made unless this device can reach that one (a kernel
  // storing through a mapping its GPU cannot reach faults the whole process), and peer access is switched on here
  // rather than left to the lazy flag alone.
  if (owner_device >= 0 && owner_device != c->device) {
    int ndev = 0, can = 0;
    HIPCHK(c, hipGetDeviceCount(&ndev));
    if (owner_device >= ndev) return fail(c, GTOP_ERR_INVALID, "shared_open: the owner's device ordinal is not visible to this process");
    HIPCHK(c, hipDeviceCanAccessPeer(&can, c->device, owner_device));
    if (!can) return fail(c, GTOP_ERR_STATE, "shared_open: this device has no peer access to the owner's device");
    const hipError_t pe = hipDeviceEnablePeerAccess(owner_device, 0);
    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) HIPCHK(c, pe);
    (void)hipGetLastError();   // (already enabled: not an error to keep)
  }
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle, sizeof(h));
  void *p = nullptr;
  HIPCHK(c, hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  *d_ptr = p;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_shared_close(gtop_ctx *c, void *d_ptr) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!d_ptr) return GTOP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipIpcCloseMemHandle(d_ptr));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_shared_free(gtop_ctx *c, void *d_ptr) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!d_ptr) return GTOP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipFree(d_ptr));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_device_clock_hz(gtop_ctx *c, double *hz) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!hz) return fail(c, GTOP_ERR_INVALID, "device_clock_hz: NULL");
  int khz = 0;
  HIPCHK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
  if (khz <= 0) return fail(c, GTOP_ERR_HIP, "hipDeviceAttributeWallClockRate reports no wall clock");
  *hz = 1e3 * (double)khz;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_set_optimizer_fusion(gtop_ctx *c, int fused) try {
  if (!c) return GTOP_ERR_INVALID;
  if (fused < 0 || fused > 2) return fail(c, GTOP_ERR_INVALID, "optimizer fusion mode is 0, 1 or 2");
  c->fuse_mma = fused;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_set_optimizer_precision(gtop_ctx *c, int dtype) try {
  if (!c) return GTOP_ERR_INVALID;
  if (dtype != GTOP_F64 && dtype != GTOP_F32) return fail(c, GTOP_ERR_INVALID, "optimizer precision is GTOP_F64 or GTOP_F32");
  c->opt_dtype = dtype;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_set_launch_geometry(gtop_ctx *c, int waves, int samples_per_lane) try {
  if (!c) return GTOP_ERR_INVALID;
  // one kernel family: a workgroup is one wavefront; the lanes-per-segment choice is what is left to pin
  if (waves != 0 && waves != 1) return fail(c, GTOP_ERR_INVALID, "waves per workgroup must be 0 (auto) or 1");
  const int s = samples_per_lane;
  if (s != 0 && s != 3 && s != 6 && s != 10 && s != 30)
    return fail(c, GTOP_ERR_INVALID, "samples per lane must be 0 (auto), 3 (ten lanes per segment, up to 6 segments), "
                                     "6 (five lanes per segment), 10 (three lanes per segment, up to 10 segments) or 30 "
                                     "(one lane per segment, up to 12 segments); 10 and 30 serve plain evaluations only: "
                                     "the optimizer loop keeps its own rule");
  c->spl = s;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
