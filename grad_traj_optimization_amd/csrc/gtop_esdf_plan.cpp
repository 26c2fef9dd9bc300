// gtop_esdf_plan.cpp — the launch plan of the distance-field builder (gtop_esdf_plan.h): every decision
// esdf_build_pass (gtop_esdf.hip) takes from a grid's three sizes.  Host only, no HIP.
#include "gtop_esdf_plan.h"

bool gtop_esdf_plan(int nx, int ny, int nz, GtopEsdfPlan *plan) {
  GtopEsdfPlan p{};
  const size_t ncol = (size_t)nx * ny;
  const size_t nvox = ncol * (size_t)nz;
  const int nyz = ny * nz;
  // Whole-grid limits: the LDS-mask z sweep holds kEsdfMaxChunks ballots per column; the y and x scans add a squared
  // distance along the line to kInf = 2^30 - 1 in int32.
  p.supported = nz <= 64 * kEsdfMaxChunks && nx <= kEsdfMaxLine && ny <= kEsdfMaxLine;
  // z sweep: one wavefront per column, four columns per workgroup
  p.z_chunks = (nz + 63) >> 6;
  p.z_lds = p.z_chunks > kEsdfZSmallChunks;
  const size_t zwant = (ncol + 3) / 4;
  p.z_strided = zwant > (size_t)kEsdfZMaxBlocks;
  p.z_blocks = (unsigned)(p.z_strided ? (size_t)kEsdfZMaxBlocks : zwant);
  // the y sweep's candidate lists: in LDS up to kEsdfYLocalMax columns per row
  p.rows_kernel = ny > kEsdfYLocalMax;
  p.rows_blocks = (unsigned)(nx < kEsdfRowsMaxBlocks ? nx : kEsdfRowsMaxBlocks);
  // Voxels per lane.  The 32-bit scans: 4 adjacent in z where nz % 4 == 0 (16-byte loads), else 1.  The packed 16-bit
  // x sweep (8 per lane) wherever the plane splits into eights of such fours; the packed y sweep (8 per lane) where a
  // lane's eight voxels share a y as well.
  const int V = nz % 4 == 0 ? 4 : 1;
  const bool x16 = V == 4 && nyz % 8 == 0;
  const bool y16 = nz % 8 == 0;
  p.y_vox = y16 ? 8 : V;
  p.y_blocks = gtop_esdf_y_blocks(nx, nyz, p.y_vox);
  p.y_writes_16 = x16;
  p.x_vox = x16 ? 8 : V;
  p.x_lanes = nyz / p.x_vox;
  p.x_block = x16 ? kEsdfX16Block : kEsdfXBlock;
  p.x_blocks = gtop_esdf_x_blocks(nx, p.x_lanes, p.x_block);
  p.slab_tables = gtop_esdf_slab_tables_possible(nx);
  // the row workspace
  const size_t half = ((nvox + 1) / 2 + 3) & ~(size_t)3;   // nvox 16-bit words in ints, a multiple of 16 bytes
  p.off_rank = ncol;
  p.off_cnt = 2 * ncol;                        // cnt[nx] = the number of empty slabs
  p.off_colany = 2 * ncol + (size_t)nx + 1;
  p.off_y16 = (p.off_colany + (ncol + 3) / 4 + 3) & ~(size_t)3;
  p.off_z16 = p.off_y16 + half;
  p.rows_ints = p.off_z16 + half;
  *plan = p;
  return p.supported;
}
