// gtop_edt.hip — batched distance queries against the static field plus moving
// boxes, on gfx950.
//
// Replaces EDTEnvironment::evaluateEDTWithGrad / distToBox / minDistToAllBox
// (src/edt_environment.cpp:26-122 of EpicOne1/grad_traj_optimization; SURVEY §8f
// row f4: the other consumer of the trilinear stencil): value and gradient by
// trilinear interpolation over the 8 corner voxels, each corner's value being
// min(static distance, distance to the nearest box at the query's time); a
// negative time means "static only" (:91-94).  A box is {p0, vel, scale}, its
// centre at time t the constant-velocity prediction p0 + vel t
// (obj_predictor.h:57-66) — or, from gtop_set_moving_box_polynomials, a quintic
// per axis on a validity interval (obj_predictor.h:26-55; gtop_edt_lookup.h).
// That file is outside the reference's build and uses
// an SDFMap API the in-tree class lacks, so the interpolation data are the
// in-tree ones (sdf_map.cpp:201-219: base index, diff, per-axis clamped corner
// loads — with time < 0 the result IS getDistWithGradTrilinear), a corner's
// position is the centre of its voxel, and a query outside the map returns -1
// with a zero gradient (sdf_map.cpp:187).
//
// One lane per query; the boxes (a few dozen at most) sit in LDS and are walked
// by every lane in step, so their reads are broadcasts.  The N x 3 query
// positions and gradients cross HBM as whole rows of the workgroup (768
// consecutive doubles, transposed through LDS at an odd stride), not as
// stride-3 accesses.  fp64.  Gather-bound: the 8 corners are 64 contiguous bytes of
// the corner records + 64 B of query/result per lane; algorithmic bytes per query
// 8*8 + 4*8 + 4*8 = 128.
// COARSE = EDTEnvironment::evaluateCoarseEDT (src/edt_environment.cpp:124-136):
// the distance of the voxel holding the position (SDFMap::getDistance(pos),
// src/sdf_map.cpp:155-164), min'ed with the box distance from the position
// itself; no interpolation, no gradient.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtop_edt_lookup.h"
#include "gtop_kernels.h"

namespace {

// boxes staged in LDS per pass: 9 KiB of rows for either kind of list (constant velocity: rows of 9; polynomial: rows of 24)
constexpr int kBoxChunk = 128, kBoxChunkPoly = 48;

// (POLY, a polynomial list: box_p0 is the list's [nbox][kBoxRowPoly] rows, box_vel and box_scale are not read)
template <bool COARSE, bool POLY>
__global__ void __launch_bounds__(256)
edt_query_kernel(const GtopGrid g, const double *__restrict__ field, const double *__restrict__ rec, int nbox,
                 const double *__restrict__ box_p0,
                 const double *__restrict__ box_vel, const double *__restrict__ box_scale, int N,
                 const double *__restrict__ pos, const double *__restrict__ time, double *__restrict__ dist,
                 double *__restrict__ grad) {
  constexpr int kChunk = POLY ? kBoxChunkPoly : kBoxChunk;
  __shared__ double bx[kChunk][kBoxRowOf<POLY>];   // p0, vel, scale; POLY: the list's rows as they are
  __shared__ double xyz[3 * 256];       // the workgroup's positions, later its gradients, as they lie in HBM
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * 256;   // first query of the workgroup
  const int i = (int)row0 + tid;
  const bool live = i < N;
  const size_t n3 = 3 * (size_t)N;
  for (int k = 0; k < 3; ++k) {
    const size_t e = 3 * row0 + tid + 256 * k;
    xyz[tid + 256 * k] = e < n3 ? pos[e] : 0.0;
  }
  __syncthreads();
  double p[3] = {xyz[3 * tid], xyz[3 * tid + 1], xyz[3 * tid + 2]};
  const double t = live ? time[i] : -1.0;
  const bool out = gtop_edt_out_of_map(g, p);   // isInMap, sdf_map.cpp:55-69
  const bool dyn = live & (COARSE || !out) & (t >= 0.0);
  int idx[3];
  double diff[3] = {0, 0, 0};
  double values[2][2][2];
  double coarse = -1.0;   // COARSE: SDFMap::getDistance(pos)
  if constexpr (COARSE) {
    // posToIndex, sdf_map.cpp:71-74 (clamped for memory safety only: an in-map position indexes inside the grid)
    for (int k = 0; k < 3; ++k) idx[k] = (int)floor((p[k] - g.origin[k]) * g.res_inv);
    const int cx = min(max(idx[0], 0), g.nx - 1), cy = min(max(idx[1], 0), g.ny - 1), cz = min(max(idx[2], 0), g.nz - 1);
    const double v = field[((size_t)cx * g.ny + cy) * g.nz + cz];
    coarse = out ? -1.0 : v;
  } else {
    // base index, diff and the 8 corner values from the corner records: gtop_edt_lookup.h
    gtop_edt_corners(g, rec, p, idx, diff, values);
  }
  // min over the boxes (edt_environment.cpp:26-73): at the 8 corner centres (:96-98), or at the position (:131)
  double dbox = 10000000.0;   // :64
  double vmax = 0.0;          // the largest of the 8 corner values so far
  if constexpr (!COARSE) vmax = gtop_edt_vmax(values);
  for (int b0 = 0; b0 < nbox; b0 += kChunk) {
    const int nb = min(kChunk, nbox - b0);
    stage_boxes<POLY>(bx, box_p0, box_vel, box_scale, b0, nb, tid, 256);
    if (dyn) {
      for (int b = 0; b < nb; ++b) {
        double bmin[3], bmax[3];
        gtop_edt_box_faces_of<POLY>(bx[b], t, bmin, bmax);
        if constexpr (COARSE) {
          double d2 = 0.0;
          for (int k = 0; k < 3; ++k) {
            const double dk = (p[k] >= bmin[k] && p[k] <= bmax[k]) ? 0.0 : fmin(fabs(p[k] - bmin[k]), fabs(p[k] - bmax[k]));
            d2 += dk * dk;
          }
          const double d = sqrt(d2);   // dist.norm()
          dbox = d < dbox ? d : dbox;
        } else {
          gtop_edt_box_min(g, bmin, bmax, idx, values, vmax);   // with the exact skip
        }
      }
    }
  }
  if constexpr (COARSE) {
    if (live) dist[i] = (t < 0.0) ? coarse : (coarse < dbox ? coarse : dbox);   // :125-135
    return;
  }
  // trilinear value and gradient, edt_environment.cpp:104-121 (= sdf_map.cpp:221-239)
  const GtopTrilinear tl = gtop_edt_trilinear(diff, values);
  double gr[3];
  gtop_edt_gradient(g, diff, values, tl, gr);   // the reference's unfused arithmetic: gtop_edt_lookup.h
  if (live) dist[i] = out ? -1.0 : tl.d;
  __syncthreads();   // every lane has read its position: the tile now carries the gradients out
  xyz[3 * tid] = out ? 0.0 : gr[0];
  xyz[3 * tid + 1] = out ? 0.0 : gr[1];
  xyz[3 * tid + 2] = out ? 0.0 : gr[2];
  __syncthreads();
  for (int k = 0; k < 3; ++k) {
    const size_t e = 3 * row0 + tid + 256 * k;
    if (e < n3) grad[e] = xyz[tid + 256 * k];
  }
}

}  // namespace

hipError_t gtop_launch_edt_query(const GtopGrid &g, const double *field, const double *rec, const GtopBoxList &boxes, int N,
                                 const double *pos, const double *time, double *dist, double *grad, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const bool poly = boxes.kind == GTOP_BOX_LIST_POLYNOMIAL && boxes.count > 0;
  const int nbox = boxes.count;
  const double *box_p0 = poly ? boxes.rows : boxes.p0, *box_vel = boxes.vel, *box_scale = boxes.scale;
#define GTOP_QUERY_LAUNCH(COARSE_, POLY_)                                                                                 \
  hipLaunchKernelGGL((edt_query_kernel<COARSE_, POLY_>), dim3((N + 255) / 256), dim3(256), 0, stream, g, field, rec, nbox, \
                     box_p0, box_vel, box_scale, N, pos, time, dist, grad)
  if (grad) {
    if (poly) GTOP_QUERY_LAUNCH(false, true);
    else GTOP_QUERY_LAUNCH(false, false);
  } else {   // evaluateCoarseEDT: no interpolation, no gradient
    if (poly) GTOP_QUERY_LAUNCH(true, true);
    else GTOP_QUERY_LAUNCH(true, false);
  }
#undef GTOP_QUERY_LAUNCH
  return hipGetLastError();
}
