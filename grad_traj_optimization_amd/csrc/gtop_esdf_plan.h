// gtop_esdf_plan.h — the launch plan of the distance-field builder (gtop_esdf.hip) and the ONE statement of its
// thresholds: which z sweep serves a column length, when the y sweep needs esdf_rows_kernel's lists, how many voxels a
// lane of the y and x sweeps owns, every grid size, the layout of the row workspace — and the maps from (workgroup,
// thread) to voxels that those grid sizes are made for.  The launcher takes every decision from gtop_esdf_plan, the
// kernels their lane from the functions below.  No HIP header: gtop_esdf_plan.cpp builds with a host compiler alone
// (tests/test_esdf_plan.py).
#ifndef GTOP_ESDF_PLAN_H_
#define GTOP_ESDF_PLAN_H_

#include <stddef.h>

#include "gtop_launch_rule.h"   // GTOP_HD

#ifdef __HIPCC__
#define GTOP_HD_INLINE __host__ __device__ inline __attribute__((always_inline))
#else
#define GTOP_HD_INLINE inline
#endif

// ---- the thresholds
constexpr int kEsdfMaxChunks = 64;       // z sweep: 64-voxel chunks per column, i.e. columns up to 4096 voxels ...
constexpr int kEsdfZSmallChunks = 8;     // ... up to 8 of them with the ballots in scalar registers, past that in LDS
constexpr int kEsdfMaxLine = 32768;      // x and y lines: d^2 + kInf stays below 2^31 for d < 2^15
constexpr int kEsdfZMaxBlocks = 65536;   // z sweep: workgroups (4 columns each) before its grid-stride loop takes over
constexpr int kEsdfZBlock = 256;         // z sweep: one wavefront per column, four columns per workgroup
constexpr int kEsdfRowsMaxBlocks = 65536;
constexpr int kEsdfYLocalMax = 2048;     // y sweep: candidate lists in LDS up to this many columns per row
constexpr int kEsdfYBlock = 256;
constexpr int kEsdfSlabMax = 2048;       // x sweep: empty-slab tables (in LDS) for lines of up to this many slabs
constexpr int kEsdfXB = 4;               // x sweep: consecutive slabs per lane
constexpr int kEsdfXBlock = 256;         // the 32-bit x sweep's workgroup
constexpr int kEsdfX16Block = 128;       // the packed x sweep's

struct GtopEsdfPlan {
  bool supported;      // false: the builder refuses the grid (everything below is still filled in)
  // z sweep
  int z_chunks;        // ceil(nz / 64): the scalar-mask instantiation for 1 .. 8
  bool z_lds;          // more than 8: the LDS-mask sweep
  unsigned z_blocks;   // workgroups of kEsdfZBlock threads
  bool z_strided;      // fewer wavefronts than columns: the sweep goes round its grid-stride loop
  // candidate lists of the y sweep
  bool rows_kernel;    // esdf_rows_kernel builds them in global memory (false: the y sweep's workgroup, in LDS)
  unsigned rows_blocks;
  // y sweep
  int y_vox;           // voxels per lane: 8 (packed 16-bit), 4 or 1
  unsigned y_blocks;   // workgroups of kEsdfYBlock threads
  // x sweep
  int x_vox;           // voxels per lane: 8 (packed 16-bit), 4 or 1
  int x_lanes;         // lanes per slab block: ny * nz / x_vox
  int x_block;         // threads per workgroup: kEsdfX16Block for the packed sweep, else kEsdfXBlock
  unsigned x_blocks;
  bool slab_tables;    // the line is short enough for the empty-slab tables (the kernel builds them only where a
                       // quarter of the slabs is empty: esdf_stage_slab_runs)
  bool y_writes_16;    // the y sweep leaves the 16-bit copy the packed x sweep reads
  // the row workspace, in ints from its start: cols [ncol] | rank [ncol] | cnt [nx + 1] | colany (ncol bytes) | padding
  // to 16 bytes | the y sweep's 16-bit output | the z sweep's 16-bit output (nvox 16-bit words each, 16-byte multiples)
  size_t off_rank, off_cnt, off_colany, off_y16, off_z16, rows_ints;
};

// The plan of an nx x ny x nz grid; returns plan->supported.
bool gtop_esdf_plan(int nx, int ny, int nz, GtopEsdfPlan *plan);

// x sweep: the empty-slab tables hold up to kEsdfSlabMax slabs
GTOP_HD constexpr bool gtop_esdf_slab_tables_possible(int nx) { return nx <= kEsdfSlabMax; }

// ---- y sweep: workgroup wg, thread tid of a grid of 8 * ceil(nx / 8) * bps workgroups, bps = ceil(nyz / V / 256)
// workgroups per slab, V voxels per lane.  Workgroups are dealt round-robin over the 8 XCDs, each with its own L2: slab
// x (whose voxels only read slab x) goes to XCD x mod 8, so a slab is fetched into ONE L2 instead of all eight.
struct GtopEsdfYLane {
  int x;        // slab (>= nx: a padding workgroup)
  int r;        // first of the lane's V voxels within the slab (>= nyz: a lane past the slab's end)
  bool first;   // the slab's first workgroup
};
static_assert(kEsdfYBlock == 256, "the y sweep's workgroups per slab are computed with >> 8");
GTOP_HD constexpr int gtop_esdf_y_blocks_per_slab(int nyz, int V) { return (nyz / V + 255) >> 8; }
GTOP_HD constexpr unsigned gtop_esdf_y_blocks(int nx, int nyz, int V) {
  return 8u * (unsigned)((nx + 7) / 8) * (unsigned)gtop_esdf_y_blocks_per_slab(nyz, V);
}
GTOP_HD_INLINE GtopEsdfYLane gtop_esdf_y_lane(unsigned wg, int tid, int nyz, int V) {
  const int bps = gtop_esdf_y_blocks_per_slab(nyz, V);
  const int xcd = wg & 7, j = wg >> 3;
  GtopEsdfYLane l{};
  l.x = xcd + 8 * (j / bps);
  l.r = ((j % bps) * kEsdfYBlock + tid) * V;
  l.first = j % bps == 0;
  return l;
}

// ---- x sweep: workgroup wg, thread tid of a grid of 8 * ceil(nx / kEsdfXB) * bpp workgroups of `block` threads; nl
// lanes per slab block.  A lane of the yz plane belongs to ONE XCD for every slab block, block after block — the rows a
// lane reads are then shared, in one L2, with the lanes of the neighbouring slab blocks that run at the same time (dealt
// linearly, every XCD walked every slab: 1.44 ms -> 0.96 ms at 400^3 with this order).  64-lane chunks of the plane are
// dealt round-robin over the XCDs: the same lanes of every slab block still meet in one L2, and every XCD gets an even
// sample of the map (with one contiguous eighth each, the XCD that owned the most open space finished 10 us after the
// others at 200^3).
struct GtopEsdfXLane {
  int fl;      // lane of the yz plane, 0 .. nl - 1
  int q0;      // first slab of the lane's block
  bool work;   // false: the thread has nothing to do and leaves
};
// lanes of one XCD's share of the plane, whole 64-lane chunks
GTOP_HD constexpr int gtop_esdf_x_lanes_per_xcd(int nl) { return ((((nl + 63) >> 6) + 7) >> 3) * 64; }
GTOP_HD constexpr unsigned gtop_esdf_x_blocks(int nx, int nl, int block) {
  return 8u * (unsigned)((nx + kEsdfXB - 1) / kEsdfXB) * (unsigned)((gtop_esdf_x_lanes_per_xcd(nl) + block - 1) / block);
}
// shadow: a wavefront with any work keeps all its lanes — those past the end of the plane shadow the last lane with
// work (fl = nl - 1) and report work = true; the caller stores nothing for them
GTOP_HD_INLINE GtopEsdfXLane gtop_esdf_x_lane(unsigned wg, int tid, int nl, int block, bool shadow) {
  const int cpx = (((nl + 63) >> 6) + 7) >> 3, bpp = (cpx * 64 + block - 1) / block;   // chunks, workgroups per XCD
  const int xcd = wg & 7, j = wg >> 3;
  const int li = (j % bpp) * block + tid;
  GtopEsdfXLane l{};
  l.q0 = (j / bpp) * kEsdfXB;
  l.fl = (((li >> 6) << 3) + xcd) * 64 + (li & 63);
  if (shadow) {
    const int wave_first = l.fl - (li & 63);
    if ((li >> 6) >= cpx || wave_first >= nl) return l;   // (work = false)
    if (l.fl >= nl) l.fl = nl - 1;
    l.work = true;
    return l;
  }
  l.work = (li >> 6) < cpx && l.fl < nl;
  return l;
}

#endif  // GTOP_ESDF_PLAN_H_
