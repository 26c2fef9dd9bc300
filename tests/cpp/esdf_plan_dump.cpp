// The distance-field builder's launch plan (csrc/gtop_esdf_plan.{h,cpp}) as text, and its lane-to-voxel maps walked on
// the host: tests/test_esdf_plan.py and the GPU tests of the builder's limits (tests/esdf_plan.py) read the output.
// Plain C++, no HIP.
//   esdf_plan_dump plan NX NY NZ [NX NY NZ ...]   one line of key=value per grid
//   esdf_plan_dump consts                          the thresholds
//   esdf_plan_dump xown                            the x sweep's map over its planned grid: one line per violation
//   esdf_plan_dump yown                            the y sweep's
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gtop_esdf_plan.h"

namespace {

int plans(int argc, char **argv) {
  if (argc < 5 || (argc - 2) % 3) return 2;
  for (int i = 2; i + 2 < argc; i += 3) {
    const int nx = atoi(argv[i]), ny = atoi(argv[i + 1]), nz = atoi(argv[i + 2]);
    GtopEsdfPlan p;
    const bool ok = gtop_esdf_plan(nx, ny, nz, &p);
    if (ok != p.supported) return 3;
    printf("nx=%d ny=%d nz=%d supported=%d z_chunks=%d z_lds=%d z_blocks=%u z_strided=%d rows_kernel=%d rows_blocks=%u "
           "y_vox=%d y_blocks=%u y_writes_16=%d x_vox=%d x_lanes=%d x_block=%d x_blocks=%u slab_tables=%d off_rank=%zu "
           "off_cnt=%zu off_colany=%zu off_y16=%zu off_z16=%zu rows_ints=%zu\n",
           nx, ny, nz, (int)p.supported, p.z_chunks, (int)p.z_lds, p.z_blocks, (int)p.z_strided, (int)p.rows_kernel,
           p.rows_blocks, p.y_vox, p.y_blocks, (int)p.y_writes_16, p.x_vox, p.x_lanes, p.x_block, p.x_blocks,
           (int)p.slab_tables, p.off_rank, p.off_cnt, p.off_colany, p.off_y16, p.off_z16, p.rows_ints);
  }
  return 0;
}

// Every (lane of the plane, slab block) is owned by exactly one thread of the planned grid; with shadows on, the extra
// lanes sit only in wavefronts whose first lane has work, and alias that wavefront's last lane with work.
int x_ownership() {
  int bad = 0;
  auto fail = [&](const char *what, int block, int nx, int nl, int wg, int tid) {
    if (++bad <= 50) printf("x block=%d nx=%d nl=%d wg=%d tid=%d: %s\n", block, nx, nl, wg, tid, what);
  };
  for (int block : {128, 256})
    for (int nx : {1, 3, 4, 5, 8, 13})
      for (int nl = 1; nl <= 1100; ++nl) {
        const int nblk = (nx + kEsdfXB - 1) / kEsdfXB;
        const unsigned grid = gtop_esdf_x_blocks(nx, nl, block);
        std::vector<int> owners((size_t)nl * nblk, 0), owners_shadow((size_t)nl * nblk, 0);
        for (unsigned wg = 0; wg < grid; ++wg)
          for (int tid = 0; tid < block; ++tid) {
            const GtopEsdfXLane a = gtop_esdf_x_lane(wg, tid, nl, block, false);
            const GtopEsdfXLane b = gtop_esdf_x_lane(wg, tid, nl, block, true);
            if (a.work) {
              if (a.fl < 0 || a.fl >= nl || a.q0 < 0 || a.q0 >= nx || a.q0 % kEsdfXB) {
                fail("a lane with work outside the plane or the line", block, nx, nl, (int)wg, tid);
                continue;
              }
              ++owners[(size_t)(a.q0 / kEsdfXB) * nl + a.fl];
              if (!b.work || b.fl != a.fl || b.q0 != a.q0) fail("shadows change a lane with work", block, nx, nl, (int)wg, tid);
              else ++owners_shadow[(size_t)(b.q0 / kEsdfXB) * nl + b.fl];
            } else if (b.work) {   // a shadow lane
              const GtopEsdfXLane f = gtop_esdf_x_lane(wg, tid & ~63, nl, block, false);
              if (!f.work) fail("a shadow in a wavefront whose first lane has no work", block, nx, nl, (int)wg, tid);
              else if (b.q0 != f.q0) fail("a shadow in another slab block than its wavefront", block, nx, nl, (int)wg, tid);
              else if (b.fl != nl - 1 || nl - 1 < f.fl || nl - 1 > f.fl + 63)
                fail("a shadow that is not its wavefront's last lane with work", block, nx, nl, (int)wg, tid);
            }
          }
        for (size_t i = 0; i < owners.size(); ++i)
          if (owners[i] != 1 || owners_shadow[i] != 1) {
            if (++bad <= 50)
              printf("x block=%d nx=%d nl=%d: lane %zu of slab block %zu owned %d times (%d with shadows)\n", block, nx, nl,
                     i % nl, i / nl, owners[i], owners_shadow[i]);
          }
      }
  return bad ? 1 : 0;
}

int y_ownership() {
  int bad = 0;
  for (int V : {1, 4, 8})
    for (int nx : {1, 7, 8, 9, 17})
      for (int k = 1; k <= 700; ++k) {
        // lanes per slab 1 .. 600 one by one, then strides that cross several workgroups per slab
        const int lanes = k <= 600 ? k : 600 + (k - 600) * 37;
        const int nyz = lanes * V;
        const unsigned grid = gtop_esdf_y_blocks(nx, nyz, V);
        std::vector<int> owners((size_t)nx * nyz, 0), firsts(nx, 0);
        for (unsigned wg = 0; wg < grid; ++wg)
          for (int tid = 0; tid < kEsdfYBlock; ++tid) {
            const GtopEsdfYLane l = gtop_esdf_y_lane(wg, tid, nyz, V);
            if (l.x < 0 || l.r < 0 || l.r % V) {
              if (++bad <= 50) printf("y V=%d nx=%d nyz=%d wg=%u tid=%d: x=%d r=%d\n", V, nx, nyz, wg, tid, l.x, l.r);
              continue;
            }
            if (l.x >= nx) continue;            // a padding workgroup
            if (tid == 0 && l.first) ++firsts[l.x];
            if (l.r >= nyz) continue;           // past the slab's end
            for (int e = 0; e < V; ++e) ++owners[(size_t)l.x * nyz + l.r + e];
          }
        for (size_t i = 0; i < owners.size(); ++i)
          if (owners[i] != 1 && ++bad <= 50)
            printf("y V=%d nx=%d nyz=%d: voxel %zu of slab %zu owned %d times\n", V, nx, nyz, i % nyz, i / nyz, owners[i]);
        for (int x = 0; x < nx; ++x)
          if (firsts[x] != 1 && ++bad <= 50) printf("y V=%d nx=%d nyz=%d: slab %d has %d first workgroups\n", V, nx, nyz, x, firsts[x]);
      }
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "plan")) return plans(argc, argv);
  if (argc > 1 && !strcmp(argv[1], "xown")) return x_ownership();
  if (argc > 1 && !strcmp(argv[1], "yown")) return y_ownership();
  if (argc > 1 && !strcmp(argv[1], "consts")) {
    printf("max_chunks=%d z_small_chunks=%d max_line=%d z_max_blocks=%d y_local_max=%d slab_max=%d xb=%d x_block=%d "
           "x16_block=%d\n",
           kEsdfMaxChunks, kEsdfZSmallChunks, kEsdfMaxLine, kEsdfZMaxBlocks, kEsdfYLocalMax, kEsdfSlabMax, kEsdfXB,
           kEsdfXBlock, kEsdfX16Block);
    return 0;
  }
  return 2;
}
