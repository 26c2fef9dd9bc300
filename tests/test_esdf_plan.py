"""The launch plan of the distance-field builder (csrc/gtop_esdf_plan.{h,cpp}: gtop_esdf_plan and the lane-to-voxel maps
gtop_esdf_y_lane / gtop_esdf_x_lane) on the CPU: plain C++ that a host compiler builds without any HIP header
(tests/esdf_plan.py, tests/cpp/esdf_plan_dump.cpp).

The expectations below were written by hand from esdf_build_pass, gtop_esdf_supported and gtop_esdf_rows_ints as they
stood when the decisions were still inline in csrc/gtop_esdf.hip (commit e8ff497) — not generated from the plan:
  supported    nz <= 64 * 64 and nx <= 32768 and ny <= 32768
  z sweep      switch ((nz + 63) >> 6): 1 .. 8 the scalar-mask instantiations, default the LDS-mask kernel;
               min((nx*ny + 3) / 4, 65536) workgroups — fewer than (nx*ny + 3) / 4 means the grid-stride loop runs
  rows kernel  ny > 2048
  y sweep      8 voxels per lane if nz % 8 == 0, else 4 if nz % 4 == 0, else 1; 8 * ceil(nx/8) * ceil(ny*nz/V/256)
  x sweep      8 per lane (128-thread workgroups) if nz % 4 == 0 and ny*nz % 8 == 0, else 4 if nz % 4 == 0, else 1
               (256); 8 * ceil(nx/4) * ceil(per_xcd / block), per_xcd = ceil(ceil(lanes/64) / 8) * 64
  slab tables  nx <= 2048 (esdf_stage_slab_runs)
The GPU side of the same limits is tests/test_gpu_esdf_limits.py."""
import shutil
import subprocess

import pytest

from tests import esdf_plan

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")

# grid -> (supported, z variant, z strided, rows kernel, y voxels per lane, x voxels per lane, slab tables)
T, F = True, False
EXPECTED = {
    # nz across every z variant: ceil(nz / 64) = 1 .. 8 scalar masks, past 512 the LDS-mask sweep, past 4096 refused.
    # nz % 64 == 0 is a multiple of 8 (8 | 8 voxels per lane); nz % 64 == 1 is odd (1 | 1)
    (6, 10, 64): (T, 1, F, F, 8, 8, T), (6, 10, 65): (T, 2, F, F, 1, 1, T),
    (6, 10, 128): (T, 2, F, F, 8, 8, T), (6, 10, 129): (T, 3, F, F, 1, 1, T),
    (6, 10, 192): (T, 3, F, F, 8, 8, T), (6, 10, 193): (T, 4, F, F, 1, 1, T),
    (6, 10, 256): (T, 4, F, F, 8, 8, T), (6, 10, 257): (T, 5, F, F, 1, 1, T),
    (6, 10, 320): (T, 5, F, F, 8, 8, T), (6, 10, 321): (T, 6, F, F, 1, 1, T),
    (6, 10, 384): (T, 6, F, F, 8, 8, T), (6, 10, 385): (T, 7, F, F, 1, 1, T),
    (6, 10, 448): (T, 7, F, F, 8, 8, T), (6, 10, 449): (T, 8, F, F, 1, 1, T),
    (6, 10, 512): (T, 8, F, F, 8, 8, T), (6, 10, 513): (T, "lds", F, F, 1, 1, T),
    (4, 6, 4095): (T, "lds", F, F, 1, 1, T),
    (4, 6, 4096): (T, "lds", F, F, 8, 8, T), (4, 6, 4097): (F, "lds", F, F, 1, 1, T),
    (4, 6, 1): (T, 1, F, F, 1, 1, T),
    # nz % 8: 0, 4, neither; ny*nz % 8 with nz % 4 == 0
    (6, 10, 16): (T, 1, F, F, 8, 8, T),
    (6, 10, 12): (T, 1, F, F, 4, 8, T),      # nz % 8 == 4, ny*nz = 120: 32-bit y sweep, packed x sweep
    (6, 10, 10): (T, 1, F, F, 1, 1, T),
    (20, 5, 4): (T, 1, F, F, 4, 4, T),       # ny*nz = 20: no packed sweep at all
    (20, 6, 4): (T, 1, F, F, 4, 8, T),       # ny*nz = 24
    (20, 5, 8): (T, 1, F, F, 8, 8, T),
    # ny: the in-LDS candidate list, the longest line
    (4, 2047, 8): (T, 1, F, F, 8, 8, T), (4, 2048, 8): (T, 1, F, F, 8, 8, T), (4, 2049, 8): (T, 1, F, T, 8, 8, T),
    (2, 32768, 8): (T, 1, F, T, 8, 8, T), (2, 32769, 8): (F, 1, F, T, 8, 8, T),
    (4, 2049, 6): (T, 1, F, T, 1, 1, T), (4, 2049, 4): (T, 1, F, T, 4, 4, T),
    # nx: the slab tables, the longest line
    (2048, 8, 8): (T, 1, F, F, 8, 8, T), (2049, 8, 8): (T, 1, F, F, 8, 8, F), (4100, 16, 8): (T, 1, F, F, 8, 8, F),
    (32768, 2, 4): (T, 1, F, F, 4, 8, F), (32768, 4, 8): (T, 1, F, F, 8, 8, F), (32765, 2, 4): (T, 1, F, F, 4, 8, F),
    (32769, 2, 4): (F, 1, F, F, 4, 8, F),
    # nx*ny: (nx*ny + 3) / 4 = 65536 workgroups serve 262 141 .. 262 144 columns without a second trip
    (512, 512, 4): (T, 1, F, F, 4, 8, T),    # 262 144 columns
    (511, 513, 4): (T, 1, F, F, 4, 4, T),    # 262 143 (ny*nz % 8 == 4)
    (545, 481, 4): (T, 1, T, F, 4, 4, T),    # 262 145: 65 537 wanted
    (1040, 260, 4): (T, 1, T, F, 4, 8, T),
    (520, 520, 8): (T, 1, T, F, 8, 8, T),
    (520, 520, 65): (T, 2, T, F, 1, 1, T),
}

# grid -> (z workgroups, rows-kernel workgroups or None, y workgroups, x threads per workgroup, x workgroups, ints of
# row workspace), worked out by hand:
#   (6, 10, 64)     z (60+3)/4; y 8 * 1 * ceil(80/256); x 80 lanes: 2 chunks -> 1 per XCD -> 64 lanes -> 1 workgroup of
#                   128, 8 * 2 * 1; rows ((120 + 7 + 15 + 3) & ~3) + 2 * 1920
#   (20, 5, 4)      z 103/4; y 5 lanes: 8 * 3 * 1; x 5 lanes, 256 threads: 8 * 5 * 1; rows ((200 + 21 + 25 + 3) & ~3) + 2 * 200
#   (520, 520, 8)   z capped; y 520 lanes: 8 * 65 * 3; x 520 lanes: 9 chunks -> 2 per XCD -> 128 lanes: 8 * 130 * 1;
#                   rows ((540800 + 521 + 67600 + 3) & ~3) + 2 * 1081600
#   (2, 32768, 8)   z 65536/4; rows kernel one workgroup per slab; y 32768 lanes: 8 * 1 * 128; x 32768 lanes: 512 chunks
#                   -> 64 per XCD -> 4096 lanes: 8 * 1 * 32
#   (32768, 2, 4)   z 65536/4; y 2 lanes: 8 * 4096 * 1; x 1 lane: 8 * 8192 * 1
#   (17, 10, 6)     z 173/4; y 60 lanes: 8 * 3 * 1; x 60 lanes: 8 * 5 * 1; rows ((340 + 18 + 43 + 3) & ~3) + 2 * 512
GRIDS_BY_HAND = {
    (6, 10, 64): (15, None, 8, 128, 16, 3984),
    (20, 5, 4): (25, None, 24, 256, 40, 648),
    (520, 520, 8): (65536, None, 1560, 128, 1040, 2772124),
    (2, 32768, 8): (16384, 2, 1024, 128, 256, None),
    (32768, 2, 4): (16384, None, 32768, 128, 65536, None),
    (17, 10, 6): (43, None, 24, 256, 40, 1428),
}


def launcher_before(nx, ny, nz):
    """esdf_build_pass's grid arithmetic and gtop_esdf_rows_ints, transcribed from csrc/gtop_esdf.hip at e8ff497."""
    ncol = nx * ny
    nvox = ncol * nz
    nyz = ny * nz
    zblocks = (ncol + 3) // 4 if (ncol + 3) // 4 < 65536 else 65536
    V = 4 if nz % 4 == 0 else 1
    nl = nyz // V

    def x_blocks(lanes, block):
        per_xcd = ((((lanes + 63) >> 6) + 7) >> 3) * 64
        return 8 * ((nx + 4 - 1) // 4) * ((per_xcd + block - 1) // block)

    if nz % 8 == 0:
        yblocks = 8 * ((nx + 7) // 8) * ((nyz // 8 + 255) // 256)
    else:
        yblocks = 8 * ((nx + 7) // 8) * ((nl + 255) // 256)
    x16 = V == 4 and nyz % 8 == 0
    xb, xblocks = (128, x_blocks(nyz >> 3, 128)) if x16 else (256, x_blocks(nl, 256))
    rows = ((2 * ncol + nx + 1 + (ncol + 3) // 4 + 3) & ~3) + 2 * (((nvox + 1) // 2 + 3) & ~3)
    return zblocks, (nx if nx < 65536 else 65536), yblocks, xb, xblocks, rows


@pytest.fixture(scope="module")
def table():
    grids = list(EXPECTED)
    return dict(zip(grids, esdf_plan.plans(grids)))


def test_thresholds_both_sides(table):
    """Every decision of the plan at each threshold and on both sides of it."""
    for grid, (supported, zvar, strided, rows, yv, xv, slab) in EXPECTED.items():
        p = table[grid]
        assert bool(p["supported"]) == supported, grid
        assert esdf_plan.cell(p) == (zvar, strided, rows, yv, xv, slab), grid
        assert p["z_chunks"] == (grid[2] + 63) // 64, grid
        assert bool(p["y_writes_16"]) == (xv == 8), grid   # the 16-bit copy is written exactly where the packed x sweep reads it


def test_the_thresholds_are_the_documented_ones():
    assert esdf_plan.constants() == dict(max_chunks=64, z_small_chunks=8, max_line=32768, z_max_blocks=65536,
                                         y_local_max=2048, slab_max=2048, xb=4, x_block=256, x16_block=128)


def test_grid_sizes_and_workspace(table):
    """Workgroups of every sweep and the ints of row workspace: a handful worked out by hand, the whole table against
    the launcher's arithmetic as it stood before the plan was cut out of it."""
    for grid, (z, rows_b, y, xb, x, ints) in GRIDS_BY_HAND.items():
        p = esdf_plan.plan(grid)
        assert (p["z_blocks"], p["y_blocks"], p["x_block"], p["x_blocks"]) == (z, y, xb, x), grid
        if rows_b is not None:
            assert p["rows_kernel"] and p["rows_blocks"] == rows_b, grid
        if ints is not None:
            assert p["rows_ints"] == ints, grid
    for grid, p in table.items():
        z, rows_b, y, xb, x, ints = launcher_before(*grid)
        assert (p["z_blocks"], p["rows_blocks"], p["y_blocks"], p["x_block"], p["x_blocks"], p["rows_ints"]) == \
            (z, rows_b, y, xb, x, ints), grid
        assert p["x_lanes"] == grid[1] * grid[2] // p["x_vox"], grid
        # the layout esdf_build_pass carved out of the workspace
        ncol, nvox = grid[0] * grid[1], grid[0] * grid[1] * grid[2]
        half = ((nvox + 1) // 2 + 3) & ~3
        assert (p["off_rank"], p["off_cnt"], p["off_colany"]) == (ncol, 2 * ncol, 2 * ncol + grid[0] + 1), grid
        assert p["off_y16"] == (2 * ncol + grid[0] + 1 + (ncol + 3) // 4 + 3) & ~3, grid
        assert p["off_y16"] % 4 == 0 and p["off_z16"] == p["off_y16"] + half and p["rows_ints"] == p["off_z16"] + half, grid
        assert 4 * (p["off_y16"] - p["off_colany"]) >= ncol, grid                      # colany: one byte per column


def test_z_sweep_covers_every_column(table):
    """Four columns per workgroup: without the loop the grid holds every column, and it never exceeds 65 536."""
    for grid, p in table.items():
        ncol = grid[0] * grid[1]
        assert p["z_blocks"] <= 65536, grid
        assert bool(p["z_strided"]) == (4 * p["z_blocks"] < ncol), grid


def test_workspace_is_monotone(table):
    """gtop_esdf_rows_ints never shrinks when an axis grows: the window path builds sub-grids in a workspace sized for
    the whole grid (gtop_capi_field.cpp update_window_on_stream)."""
    grids = list(table)
    for a in grids:
        for b in grids:
            if all(x <= y for x, y in zip(a, b)):
                assert table[a]["rows_ints"] <= table[b]["rows_ints"], (a, b)
    steps = []
    for g in grids:
        for axis in range(3):
            for inc in (1, 3, 64):
                h = list(g)
                h[axis] += inc
                steps.append((g, tuple(h)))
    grown = esdf_plan.plans([h for _, h in steps])
    for (g, h), ph in zip(steps, grown):
        assert table[g]["rows_ints"] <= ph["rows_ints"], (g, h)


def test_x_sweep_ownership():
    """gtop_esdf_x_lane over the planned grid (gtop_esdf_x_blocks), workgroups of 128 and 256 threads, 1 .. 1100 lanes per
    slab block, lines of 1 .. 13 slabs: every (lane, slab block) is owned by exactly one thread; with shadows on, shadow
    lanes appear only in wavefronts whose first lane has work and alias that wavefront's last lane with work.  The
    dumper prints one line per violation."""
    out = subprocess.run([esdf_plan.dumper(), "xown"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "", out.stdout[:2000] + out.stderr


def test_y_sweep_ownership():
    """gtop_esdf_y_lane over the planned grid (gtop_esdf_y_blocks), 1, 4 and 8 voxels per lane, 1 .. 4300 lanes per slab,
    1 .. 17 slabs: every voxel is owned exactly once, and every slab has exactly one first workgroup (the one that
    counts the slab's obstacle columns)."""
    out = subprocess.run([esdf_plan.dumper(), "yown"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "", out.stdout[:2000] + out.stderr
