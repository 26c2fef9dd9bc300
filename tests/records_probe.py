"""A probe for the corner records (csrc/gtop_records.hip): inputs that read EVERY record of a map, one
cell per row, so that one wrong record is one wrong row — named by its cell — instead of something a random batch may
or may not sample.  A plain helper (tests/test_records_probe.py checks the probe itself on the CPU,
tests/test_gpu_records.py uses it on the device).

  * the field: independent uniform values in [0.05, 0.6] per voxel — all below d0 = 0.8, so every corner of every
    cell carries the collision penalty, and every voxel differs from its neighbours;
  * the cells: every base index (ix, iy, iz) an in-map position can have, -1 .. n-1 per axis (sdf_map.cpp:201-204):
    (nx+1)(ny+1)(nz+1) cells, which between them read every record, the clamped border copies and the two padding
    levels included.  The map size must be grid * res exactly (MapSpec.map_size) for the cells n-1 to be in the map;
  * one trajectory per cell: all m + 1 waypoints inside the cell, zero velocity and acceleration at every one of
    them, so that each segment is a rest-to-rest quintic — monotone per axis, it stays between its end points — and
    the row reads that cell and no other.  The fractional position in the cell (0 = the centre of voxel ix, 1 = of
    ix + 1) is drawn in [0.15, 0.85]; a -1 cell and an n-1 cell are half cells (the map ends at the voxel's middle):
    [0.575, 0.925] and [0.075, 0.425], clear of the 1e-4 map margin and of the fp32 tie band;
  * bare query positions placed the same way, with their cells.
"""
import numpy as np

from grad_traj_optimization_amd import problem

RES = 0.2
# the smallest grids that reach each edge of the builder (tests/test_gpu_records.py says which)
GRIDS = [(2, 2, 2), (3, 8, 2), (9, 7, 5), (8, 15, 4), (17, 16, 33), (25, 24, 7)]

FIELD_LO, FIELD_HI = 0.05, 0.6
SEG_T = 0.5


def geometry(grid, res=RES):
    """(origin, map_size) of a probe map: map_size = grid * res (nudged down by ulps where ceil would add a voxel)."""
    origin = np.array([-grid[0] * res / 2, -grid[1] * res / 2, 0.0])
    return origin, problem.MapSpec(tuple(grid), float(res), origin, None).map_size


def probe_field(grid, seed):
    """(nx, ny, nz) independent uniform values in [FIELD_LO, FIELD_HI]."""
    return np.random.default_rng([int(seed), 20260]).uniform(FIELD_LO, FIELD_HI, size=tuple(grid))


def cells(grid):
    """Every base index of an in-map position: (ncells, 3) int, ix slowest, each axis -1 .. n-1."""
    ax = [np.arange(-1, n) for n in grid]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def _place(grid, origin, res, cell, shape_mid, rng):
    """Positions inside `cell` (k, 3): (k, *shape_mid, 3), fractions drawn per axis in the cell's own range."""
    n = np.asarray(grid)
    lo = np.where(cell == -1, 0.575, np.where(cell == n - 1, 0.075, 0.15))
    hi = np.where(cell == -1, 0.925, np.where(cell == n - 1, 0.425, 0.85))
    ex = (slice(None),) + (None,) * len(shape_mid) + (slice(None),)
    f = rng.uniform(size=(len(cell),) + tuple(shape_mid) + (3,))
    f = lo[ex] + f * (hi[ex] - lo[ex])
    return np.asarray(origin)[None] + (cell[ex] + 0.5 + f) * res


def probe_rows(grid, origin, res, m=2, seed=0, count=None):
    """(T (B, m), Df (B, 3, 6), x (B, 9(m-1))): row r reads cell r (mod the cell count, where `count` asks for more
    rows than there are cells; repeated cells get waypoints of their own) and no other."""
    cl = cells(grid)
    if count is not None:
        cl = cl[np.arange(int(count)) % len(cl)]
    wp = _place(grid, origin, res, cl, (m + 1,), np.random.default_rng([int(seed), m, 20261]))
    Df, Dp = problem.initial_derivatives(wp)          # positions only: velocity and acceleration zero everywhere
    return np.full((len(cl), m), SEG_T), Df, Dp.reshape(len(cl), -1)


def probe_queries(grid, origin, res, per_cell=4, seed=0):
    """(pos (ncells * per_cell, 3), cell (ncells * per_cell, 3)): bare positions placed as the waypoints are."""
    cl = cells(grid)
    pos = _place(grid, origin, res, cl, (per_cell,), np.random.default_rng([int(seed), per_cell, 20262]))
    return pos.reshape(-1, 3), np.repeat(cl, per_cell, axis=0)


def base_index(pos, origin, res):
    """The base index of the trilinear lookup at pos (.., 3) as sdf_map.cpp:201-204 computes it:
    posToIndex(pos - res / 2) = floor((pos - res / 2 - origin) * (1 / res))."""
    return np.floor(((np.asarray(pos) - 0.5 * res * 1.0) - np.asarray(origin)) * (1 / res)).astype(np.int64)


def clamped_corners(grid, cell):
    """The distinct voxels the 8 corners of `cell` read after the per-axis index clamp (sdf_map.cpp:166-174)."""
    n = np.asarray(grid)
    out = set()
    for d in np.ndindex(2, 2, 2):
        out.add(tuple(int(v) for v in np.clip(np.asarray(cell) + d, 0, n - 1)))
    return sorted(out)


def face_neighbours(grid, vox):
    out = []
    for a in range(3):
        for s in (-1, 1):
            v = list(vox)
            v[a] += s
            if 0 <= v[a] < grid[a]:
                out.append(tuple(v))
    return out
