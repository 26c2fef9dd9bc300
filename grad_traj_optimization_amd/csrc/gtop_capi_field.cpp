// gtop_capi_field.cpp — the distance field of a context (GtopField, gtop_ctx.h) and the entry points that make it:
// uploads, borrowed device fields, the ESDF builder over the whole map and over a window, the corner records behind
// each of them.
#include <algorithm>
#include <cmath>

#include "gtop_ctx.h"

int GtopField::need_records64(gtop_ctx *c) const {
  return records64_current() ? GTOP_OK : fail(c, GTOP_ERR_STATE, "no fp64 distance field resident");
}

int GtopField::need_boundary(gtop_ctx *c) const {
  return have_grid && sdf64 ? GTOP_OK : fail(c, GTOP_ERR_STATE, "no fp64 distance field resident");
}

int GtopField::set_grid(gtop_ctx *c, int nx, int ny, int nz, const double origin[3], const double *map_size, double res) {
  if (!origin || nx < 2 || ny < 2 || nz < 2 || !(res > 0.0))
    return fail(c, GTOP_ERR_INVALID, "SDF geometry: need origin, grid >= 2 per axis, resolution > 0");
  if ((double)nx * ny * nz >= 2147483648.0)
    return fail(c, GTOP_ERR_INVALID, "SDF geometry: nx*ny*nz must be < 2^31");
  GtopGrid &g = grid;
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.res = res;
  g.res_inv = 1 / res;   // sdf_map.cpp:7
  const int gs[3] = {nx, ny, nz};
  for (int i = 0; i < 3; ++i) {
    g.origin[i] = origin[i];
    g.min_range[i] = origin[i];                                            // sdf_map.cpp:11
    g.max_range[i] = origin[i] + (map_size ? map_size[i] : gs[i] * res);   // sdf_map.cpp:12
  }
  have_grid = true;
  return GTOP_OK;
}

void GtopField::release() {
  own.release();
  sdf64 = nullptr;
  sdf32b = nullptr;
  rec64_ok = false;
  rec32_state = Rec32::absent;
}

// room for the corner records of the grid, both precisions (e: what an allocation in front of them returned)
int GtopField::reserve_records(gtop_ctx *c, hipError_t e) {
  const size_t n = 4 * gtop_record_count(grid);
  if (e == hipSuccess) e = rec64.reserve(n);
  if (e == hipSuccess) e = rec32.reserve(n);
  if (e == hipSuccess) return GTOP_OK;
  have_grid = false;
  return fail(c, GTOP_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
}

int GtopField::make_owned(gtop_ctx *c) {
  const hipError_t e = own.reserve((size_t)grid.nx * grid.ny * grid.nz);
  sdf64 = own.data();
  sdf32b = nullptr;
  return reserve_records(c, e);
}

int GtopField::arrived(gtop_ctx *c, hipStream_t s, bool convert_now, const int *vlo, const int *vhi) {
  if (!vlo) {   // (the library cannot tell what uploaded values mean: the mode in force names them)
    sign = sign_next;
    depth = depth_next;
  }
  const bool follow = (convert_now || fp32_in_use) && fp32_wanted;
  // Both precisions in one pass over the field when both are wanted.  Of a voxel box only the records that hold one of
  // its voxels change: fp32 records that are current stay current (their part is rebuilt in the same pass); stale
  // ones cannot be made current by a box: they are rebuilt whole behind it where fp32 must follow, and stay stale —
  // to be rebuilt at the first fp32 use — otherwise.
  const bool both = vlo ? rec32_state == Rec32::current : follow;
  HIPCHK(c, (gtop_launch_build_records<double, double>(grid, sdf64, rec64.data(), both ? rec32.data() : nullptr, vlo, vhi, s)));
  rec64_ok = true;
  rec32_state = both ? Rec32::current : Rec32::stale;
  return vlo && !both && follow ? need_records32(c, s) : GTOP_OK;
}

int GtopField::borrow(gtop_ctx *c, int dtype, const void *dist_dev, hipStream_t s) {
  release();
  if (int rc = reserve_records(c)) return rc;
  // The buffer is borrowed as the boundary copy (gtop_get_sdf and the coarse voxel query read it in place); the
  // corner records the lookups read are derived from it HERE — a caller that rewrites the buffer calls again.
  if (dtype == GTOP_F64) {
    sdf64 = const_cast<double *>(static_cast<const double *>(dist_dev));
    return arrived(c, s, false);
  }
  sign = sign_next;
  depth = depth_next;
  sdf32b = static_cast<const float *>(dist_dev);
  HIPCHK(c, (gtop_launch_build_records<float, float>(grid, sdf32b, rec32.data(), nullptr, nullptr, nullptr, s)));
  rec32_state = Rec32::current;
  return GTOP_OK;
}

int GtopField::need_records32(gtop_ctx *c, hipStream_t s) {
  if (!fp32_wanted)
    return fail(c, GTOP_ERR_STATE, "fp32 evaluation on a context whose fp32 records are switched off (gtop_set_field_precisions)");
  fp32_in_use = true;
  if (rec32_state == Rec32::current) return GTOP_OK;
  if (rec32_state != Rec32::stale || !sdf64) return fail(c, GTOP_ERR_STATE, "no fp32 distance field resident");
  // only a synchronous entry point (gtop_set_sdf, gtop_init_sdf_map, gtop_update_sdf_map) leaves the records stale,
  // and it has synchronised: the fp64 field is complete whatever stream `s` is
  HIPCHK(c, (gtop_launch_build_records<double, float>(grid, sdf64, rec32.data(), nullptr, nullptr, nullptr, s)));
  rec32_state = Rec32::current;
  return GTOP_OK;
}

void GtopField::keep_fp32(bool keep) {
  fp32_wanted = keep;
  // (switched on again: rebuilt from the fp64 field at the first fp32 use)
  if (!keep) rec32_state = sdf64 ? Rec32::stale : Rec32::absent;
}

namespace {

// what a signed build clamps occupied voxels to: max_depth, 0 meaning the reference's 10000
double field_depth(double max_depth) { return max_depth == 0.0 ? 10000.0 : max_depth; }

// The builder's workspace for the current grid (gtop_set_sdf may have moved the context to a larger grid since
// gtop_init_sdf_map sized the occupancy).  window: the compact path's scratch too, sized for the whole grid whatever
// the window is: the first window update of a map allocates, later ones of any size do not — capturable, and no
// implicit device synchronisation from a reallocation between two enqueued updates.
int reserve_workspace(gtop_ctx *c, bool window) {
  const GtopGrid &g = c->field.grid;
  const size_t nvox = (size_t)g.nx * g.ny * g.nz;
  HIPCHK(c, c->occ.reserve(nvox));
  HIPCHK(c, c->tmp1.reserve(nvox));
  HIPCHK(c, c->tmp2.reserve(nvox));
  HIPCHK(c, c->rows.reserve(gtop_esdf_rows_ints(g)));
  if (window) {
    HIPCHK(c, c->win_occ.reserve(nvox));
    HIPCHK(c, c->win_dist.reserve(nvox));
  }
  return GTOP_OK;
}

// the build proper: obstacle points already in HBM, launches on `s`, no synchronisation
int update_sdf_map_on_stream(gtop_ctx *c, const double *d_pts, int npts, hipStream_t s, bool convert_now) {
  GtopField &f = c->field;
  const GtopGrid &g = f.grid;
  const size_t nvox = (size_t)g.nx * g.ny * g.nz;
  if (int rc = reserve_workspace(c, false)) return rc;
  uint8_t *occ = c->occ.data();
  int *tmp1 = c->tmp1.data(), *tmp2 = c->tmp2.data(), *rows = c->rows.data();
  if (!gtop_esdf_supported(g))
    return fail(c, GTOP_ERR_INVALID, "updateSDFMap: grid too large for the device builder (nz <= 4096, nx, ny <= 32768)");
  // resetBuffer (sdf_map.cpp:26-53): the occupancy; the distances need no reset of their own, the x sweep
  // writes every voxel (10000 where the line holds no obstacle, as the reset would have left it)
  HIPCHK(c, gtop_launch_esdf_reset(occ, nullptr, nvox, s));
  HIPCHK(c, gtop_launch_esdf_mark(g, d_pts, npts, occ, s));         // setOccupancy
  if (f.sign_next)   // the signed field (gtop_set_field_sign): a second transform fills the occupied voxels
    HIPCHK(c, gtop_launch_esdf_build_signed(g, occ, tmp1, tmp2, rows, f.sdf64, field_depth(f.depth_next), s));
  else
    HIPCHK(c, gtop_launch_esdf_build(g, occ, tmp1, tmp2, rows, f.sdf64, s));   // updateESDF3d
  // the corner records behind it, on the same stream (device-side: holds for graph replays too); the fp32 ones now
  // when they are wanted now, otherwise at the first fp32 evaluation (host-synchronous caller only, see GtopField)
  return f.arrived(c, s, convert_now);
}

// The window of (min_pos, max_pos) in voxel indices, as resetBuffer(min, max) and setUpdateRange compute it
// (sdf_map.cpp:28-45, :244-260): both positions clamped to [min_range, max_range], then posToIndex(min_pos) and
// posToIndex(max_pos - res/2).  Indices are clipped into the grid (memory safety only: they are inside already).
void window_ids(const GtopGrid &g, const double min_pos[3], const double max_pos[3], int lo[3], int hi[3]) {
  const int n[3] = {g.nx, g.ny, g.nz};
  for (int i = 0; i < 3; ++i) {
    const double a = std::max(min_pos[i], g.min_range[i]), b = std::min(max_pos[i], g.max_range[i]);
    lo[i] = (int)std::floor((a - g.origin[i]) * g.res_inv);                      // posToIndex, :71-74
    hi[i] = (int)std::floor(((b - g.res / 2) - g.origin[i]) * g.res_inv);
    lo[i] = std::max(lo[i], 0);
    hi[i] = std::min(hi[i], n[i] - 1);
  }
}

// resetBuffer(min, max) + setOccupancy per point + setUpdateRange(min, max) + updateESDF3d, then the corner records of
// the voxels that changed; launches on `s`, no synchronisation
int update_window_on_stream(gtop_ctx *c, const double min_pos[3], const double max_pos[3], const double *d_pts, int npts,
                            hipStream_t s, bool convert_now) {
  GtopField &f = c->field;
  const GtopGrid &g = f.grid;
  // (never a field that is signed in some boxes only)
  if (f.sign_pending())
    return fail(c, GTOP_ERR_STATE, "update window: whole-map update needed after changing the field sign "
                                   "(gtop_update_sdf_map*, gtop_init_sdf_map or gtop_set_sdf*)");
  int lo[3], hi[3];
  window_ids(g, min_pos, max_pos, lo, hi);
  if (int rc = reserve_workspace(c, true)) return rc;
  uint8_t *occ = c->occ.data(), *win_occ = c->win_occ.data();
  int *tmp1 = c->tmp1.data(), *tmp2 = c->tmp2.data(), *rows = c->rows.data();
  double *win_dist = c->win_dist.data();
  const int wx = hi[0] - lo[0] + 1, wy = hi[1] - lo[1] + 1, wz = hi[2] - lo[2] + 1;
  if (wx <= 0 || wy <= 0 || wz <= 0) {   // empty: no voxel changes its distance, the points are still marked
    HIPCHK(c, gtop_launch_esdf_window_reset(g, lo, hi, occ, f.sdf64, s));
    HIPCHK(c, gtop_launch_esdf_mark(g, d_pts, npts, occ, s));
    return GTOP_OK;
  }
  // the window is the map: the whole-grid builder (same results: every distance is 10000 after the reset)
  if (wx == g.nx && wy == g.ny && wz == g.nz) return update_sdf_map_on_stream(c, d_pts, npts, s, convert_now);
  // The sweeps over the window see nothing outside it: the update IS the whole-grid transform of the window taken alone.
  // A window of at least 12 x 12 x 3 voxels therefore goes through the whole-grid builder (gtop_esdf.hip: packed 16-bit
  // scans, candidate lists, slab skipping) on a compact copy of its occupancy, and the result is written back into the
  // window — 10x less time per voxel than the plain window kernels, which serve the slivers.
  GtopGrid sub = g;
  sub.nx = wx; sub.ny = wy; sub.nz = wz;
  if (wx >= 12 && wy >= 12 && wz >= 3 && gtop_esdf_supported(sub)) {
    // reset + marking of the map's occupancy and of the compact copy in two kernels, no gather; the window's distances
    // need no reset: the scatter below rewrites every voxel of it
    HIPCHK(c, gtop_launch_esdf_window_reset_mark_compact(g, lo, hi, d_pts, npts, occ, win_occ, s));
    if (f.sign)
      HIPCHK(c, gtop_launch_esdf_build_signed(sub, win_occ, tmp1, tmp2, rows, win_dist, field_depth(f.depth), s));
    else
      HIPCHK(c, gtop_launch_esdf_build(sub, win_occ, tmp1, tmp2, rows, win_dist, s));
    HIPCHK(c, gtop_launch_esdf_window_scatter(g, lo, hi, win_dist, f.sdf64, s));
  } else {   // a sliver
    HIPCHK(c, gtop_launch_esdf_window_reset(g, lo, hi, occ, f.sdf64, s));
    HIPCHK(c, gtop_launch_esdf_mark(g, d_pts, npts, occ, s));   // (anywhere in the map: setOccupancy does not look at the window)
    if (f.sign)
      HIPCHK(c, gtop_launch_esdf_window_build_signed(g, lo, hi, occ, tmp1, tmp2, f.sdf64, field_depth(f.depth), s));
    else
      HIPCHK(c, gtop_launch_esdf_window_build(g, lo, hi, occ, tmp1, tmp2, f.sdf64, s));
  }
  return f.arrived(c, s, convert_now, lo, hi);
}

// What the four map-update entries ask first (window: gtop_update_sdf_map_window*, which also need current records);
// args_ok: the entry's own arguments are usable.  Leaves the context's device current.
int map_update_ready(gtop_ctx *c, bool window, bool args_ok) {
  if (!args_ok) return fail(c, GTOP_ERR_INVALID, window ? "update window: bad arguments" : "bad obstacle list");
  const GtopField &f = c->field;
  if (!f.have_grid || !f.owned() || !c->occ.data() || (window && !f.records64_current()))
    return fail(c, GTOP_ERR_STATE, window ? "update window: call gtop_init_sdf_map first"
                                          : "updateSDFMap: call gtop_init_sdf_map first");
  HIPCHK(c, hipSetDevice(c->device));
  return GTOP_OK;
}
bool points_ok(const void *pts, int npts) { return npts >= 0 && (npts == 0 || pts); }

// the obstacle points of a host-pointer update, on their way to d_pts on the context's stream
int upload_points(gtop_ctx *c, const double *pts, int npts) {
  if (npts <= 0) return GTOP_OK;
  HIPCHK(c, c->d_pts.reserve((size_t)npts * 3));
  HIPCHK(c, hipMemcpyAsync(c->d_pts.data(), pts, (size_t)npts * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return GTOP_OK;
}

}  // namespace

extern "C" {

int gtop_set_sdf(gtop_ctx *c, const double *dist_host, int nx, int ny, int nz,
                 const double origin[3], const double *map_size, double resolution) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!dist_host) return fail(c, GTOP_ERR_INVALID, "dist_host is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  GtopField &f = c->field;
  int rc = f.set_grid(c, nx, ny, nz, origin, map_size, resolution);
  if (rc) return rc;
  if ((rc = f.make_owned(c))) return rc;
  HIPCHK(c, hipMemcpyAsync(f.sdf64, dist_host, (size_t)nx * ny * nz * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = f.arrived(c, c->stream, false))) return rc;   // the upload transform
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_set_sdf_device(gtop_ctx *c, int dtype, const void *dist_dev, int nx, int ny, int nz,
                        const double origin[3], const double *map_size, double resolution) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!dist_dev) return fail(c, GTOP_ERR_INVALID, "dist_dev is NULL");
  if (dtype != GTOP_F64 && dtype != GTOP_F32) return fail(c, GTOP_ERR_INVALID, "bad dtype");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = c->field.set_grid(c, nx, ny, nz, origin, map_size, resolution);
  if (rc) return rc;
  if ((rc = c->field.borrow(c, dtype, dist_dev, c->stream))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_init_sdf_map(gtop_ctx *c, const double map_size[3], const double origin[3], double resolution) try {
  if (!c) return GTOP_ERR_INVALID;
  if (!map_size || !origin || !(resolution > 0.0))
    return fail(c, GTOP_ERR_INVALID, "initSDFMap: need map_size, origin, resolution > 0");
  HIPCHK(c, hipSetDevice(c->device));
  int gs[3];
  for (int i = 0; i < 3; ++i) gs[i] = (int)std::ceil(map_size[i] / resolution);   // sdf_map.cpp:9
  GtopField &f = c->field;
  int rc = f.set_grid(c, gs[0], gs[1], gs[2], origin, map_size, resolution);
  if (rc) return rc;
  const size_t nvox = (size_t)gs[0] * gs[1] * gs[2];
  if ((rc = f.make_owned(c))) return rc;
  HIPCHK(c, c->occ.reserve(nvox));
  // sdf_map.cpp:22-23: distance 10000, occupancy 0
  HIPCHK(c, gtop_launch_esdf_reset(c->occ.data(), f.sdf64, nvox, c->stream));
  if ((rc = f.arrived(c, c->stream, false))) return rc;   // a whole-map build: the all-free field is the same in both modes
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_update_sdf_map(gtop_ctx *c, const double *pts, int npts) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc = map_update_ready(c, false, points_ok(pts, npts));
  if (!rc) rc = upload_points(c, pts, npts);
  if (!rc) rc = update_sdf_map_on_stream(c, c->d_pts.data(), npts, c->stream, /*convert_now=*/false);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_update_sdf_map_device(gtop_ctx *c, const void *d_pts, int npts, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = map_update_ready(c, false, points_ok(d_pts, npts))) return rc;
  return update_sdf_map_on_stream(c, static_cast<const double *>(d_pts), npts, static_cast<hipStream_t>(hip_stream),
                                  /*convert_now=*/true);
} GTOP_CATCH_STATUS(c)

int gtop_update_sdf_map_window(gtop_ctx *c, const double min_pos[3], const double max_pos[3], const double *pts,
                               int npts) try {
  if (!c) return GTOP_ERR_INVALID;
  int rc = map_update_ready(c, true, min_pos && max_pos && points_ok(pts, npts));
  if (!rc) rc = upload_points(c, pts, npts);
  if (!rc) rc = update_window_on_stream(c, min_pos, max_pos, c->d_pts.data(), npts, c->stream, /*convert_now=*/false);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_update_sdf_map_window_device(gtop_ctx *c, const double min_pos[3], const double max_pos[3], const void *d_pts,
                                      int npts, void *hip_stream) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = map_update_ready(c, true, min_pos && max_pos && points_ok(d_pts, npts))) return rc;
  return update_window_on_stream(c, min_pos, max_pos, static_cast<const double *>(d_pts), npts,
                                 static_cast<hipStream_t>(hip_stream), /*convert_now=*/true);
} GTOP_CATCH_STATUS(c)

int gtop_set_field_sign(gtop_ctx *c, int signed_mode, double max_depth) try {
  if (!c) return GTOP_ERR_INVALID;
  if (signed_mode != 0 && signed_mode != 1)
    return fail(c, GTOP_ERR_INVALID, "field sign: signed_mode must be 0 (unsigned) or 1 (signed)");
  if (!std::isfinite(max_depth) || max_depth < 0.0)
    return fail(c, GTOP_ERR_INVALID, "field sign: max_depth must be finite and >= 0 (0 = 10000)");
  c->field.sign_next = signed_mode;
  c->field.depth_next = max_depth;
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_get_field_sign(const gtop_ctx *c, int *signed_mode, double *max_depth) {
  if (!c) return GTOP_ERR_INVALID;
  if (signed_mode) *signed_mode = c->field.sign;
  if (max_depth) *max_depth = c->field.depth;
  return GTOP_OK;
}

int gtop_set_field_precisions(gtop_ctx *c, int keep_fp32) try {
  if (!c) return GTOP_ERR_INVALID;
  if (keep_fp32 != 0 && keep_fp32 != 1) return fail(c, GTOP_ERR_INVALID, "field precisions: 0 (fp64 records only) or 1 (fp32 records too)");
  c->field.keep_fp32(keep_fp32 != 0);
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

int gtop_get_sdf(gtop_ctx *c, double *dist_host, int grid_out[3]) try {
  if (!c) return GTOP_ERR_INVALID;
  if (int rc = c->field.need_boundary(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const GtopGrid &g = c->field.grid;
  if (grid_out) { grid_out[0] = g.nx; grid_out[1] = g.ny; grid_out[2] = g.nz; }
  if (dist_host) {
    const size_t nvox = (size_t)g.nx * g.ny * g.nz;
    HIPCHK(c, hipMemcpyAsync(dist_host, c->field.sdf64, nvox * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GTOP_OK;
} GTOP_CATCH_STATUS(c)

}  // extern "C"
