"""The distance-field builder (csrc/gtop_esdf.hip) at every limit of its launch plan (csrc/gtop_esdf_plan.h), bit for
bit against scipy's exact transform: np.minimum(res * distance_transform_edt(occ == 0), 10000), 10000 everywhere on a
map without obstacles.  No tolerance anywhere: every comparison is np.array_equal.

Every row of ROWS names the plan cell it is there for — (z sweep variant, z sweep strided, esdf_rows_kernel runs, voxels
per lane of the y sweep, of the x sweep, slab tables possible) — and the test asserts that cell through the host-only
plan (tests/esdf_plan.py, the statement the launcher itself reads) before it builds: a threshold that moves fails the row
instead of quietly uncovering its variant.  test_rows_cover_every_plan_cell asserts that the rows reach every cell.  The
limit axis of a row is at the limit; the other axes are as thin as the cell allows.  The plan itself is pinned on the CPU
by tests/test_esdf_plan.py.

Not covered ("limits of the builder"): the LDS-mask z sweep's grid-stride loop (nx*ny > 262 144 with nz > 512:
more than 134 M voxels), and squared distances past 2^30 - 1 (smallest grid 32768 x 258 x 4)."""
import functools

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import esdf_plan
from tests.test_gpu_signed_field import signed_reference

ERR_INVALID = 1
T, F = True, False

# (grid, plan cell, patterns).  Patterns:
#   corner   one obstacle at the origin corner: every distance along the long axis, both saturations past 255 voxels, and
#            at 32768 squares up to 32767^2 + small beside kInf = 2^30 - 1
#   empty    no obstacle: 10000 everywhere; at nx = 32768 / 32765 every x scan runs its whole reach with kInf candidates
#            (d^2 + kInf at its largest; 32765: a reach that is no multiple of the batch); the c == 0 branch of the packed
#            y sweep; every wavefront of the packed x sweep falling back
#   ends     obstacles at both ends and the middle of the long axis, plus 2 % random
#   slabs3   the same in three slabs x = 0, nx/2, nx - 1 only: more than a quarter of the slabs empty, so the slab tables
#            are built wherever they are possible (nx = 2048) and cannot be at 2049, 4100, 32768
#   full     every voxel occupied: a candidate list as long as the row
#   floor    obstacles at z = 0 only: z distances past 255 voxels
#   half     corner at res = 0.5: res * sqrt(n) passes 10000 along x and the min with 10000 decides
ROWS = [
    # nx: the longest line, and the slab tables' limit
    ((32768, 2, 4), (1, F, F, 4, 8, F), ("corner", "empty", "slabs3", "half")),
    ((32768, 4, 8), (1, F, F, 8, 8, F), ("corner", "empty", "slabs3")),
    ((32765, 2, 4), (1, F, F, 4, 8, F), ("corner", "empty", "slabs3")),
    ((2048, 8, 8), (1, F, F, 8, 8, T), ("corner", "empty", "slabs3")),
    ((2049, 8, 8), (1, F, F, 8, 8, F), ("corner", "empty", "slabs3")),
    ((4100, 16, 8), (1, F, F, 8, 8, F), ("corner", "empty", "slabs3")),
    # ny: the longest line, and the in-LDS candidate list's limit (s_cols[2047], s_pref[32])
    ((2, 32768, 8), (1, F, T, 8, 8, T), ("corner", "empty", "ends")),
    ((4, 2047, 8), (1, F, F, 8, 8, T), ("corner", "empty", "ends", "full")),
    ((4, 2048, 8), (1, F, F, 8, 8, T), ("corner", "empty", "ends", "full")),
    ((4, 2049, 8), (1, F, T, 8, 8, T), ("corner", "empty", "ends")),
    ((4, 2049, 4), (1, F, T, 4, 4, T), ("corner", "empty", "ends")),     # esdf_rows_kernel's lists, 4 voxels per lane
    ((4, 2049, 6), (1, F, T, 1, 1, T), ("corner", "empty", "ends")),     # ... and 1
    # nz: every z sweep variant on both sides of its threshold, the longest column
    ((6, 10, 64), (1, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 65), (2, F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((6, 10, 128), (2, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 129), (3, F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((6, 10, 192), (3, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 193), (4, F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((6, 10, 256), (4, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 257), (5, F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((6, 10, 320), (5, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 321), (6, F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((6, 10, 384), (6, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 385), (7, F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((6, 10, 448), (7, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 449), (8, F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((6, 10, 512), (8, F, F, 8, 8, T), ("corner", "empty", "ends")),
    ((6, 10, 513), ("lds", F, F, 1, 1, T), ("corner", "empty", "ends", "floor")),
    ((4, 6, 4095), ("lds", F, F, 1, 1, T), ("corner", "empty", "ends")),
    ((4, 6, 4096), ("lds", F, F, 8, 8, T), ("corner", "empty", "ends", "floor")),
    # voxels per lane: nz % 8 == 4 with ny*nz % 8 == 0 (32-bit y sweep, packed x sweep) and with ny*nz % 8 != 0 (neither)
    ((6, 10, 12), (1, F, F, 4, 8, T), ("corner", "empty", "ends")),
    ((20, 5, 4), (1, F, F, 4, 4, T), ("corner", "empty", "ends")),
    # nx*ny > 262 144: the z sweep goes round its grid-stride loop, on two different y / x paths
    ((1040, 260, 4), (1, T, F, 4, 8, T), ("corner", "empty", "ends")),
    ((520, 520, 8), (1, T, F, 8, 8, T), ("corner", "empty", "ends")),
]
CELLS = {grid: cell for grid, cell, _ in ROWS}
CASES = [(grid, kind) for grid, _, kinds in ROWS for kind in kinds]


def _occupancy(grid, kind):
    nx, ny, nz = grid
    rng = np.random.default_rng(nx * 1000 + ny * 10 + nz)
    occ = np.zeros(grid, dtype=np.uint8)
    axis = int(np.argmax(grid))
    n = grid[axis]
    if kind in ("corner", "half", "deep"):
        occ[0, 0, 0] = 1
        if kind == "deep":                 # all occupied but one voxel: the signed field's interior transform
            occ = 1 - occ
    elif kind == "ends":
        occ[rng.random(grid) < 0.02] = 1
        for at in (0, n // 2, n - 1):
            idx = [0, 0, 0]
            idx[axis] = at
            occ[tuple(idx)] = 1
    elif kind == "slabs3":
        assert axis == 0
        for at in (0, nx // 2, nx - 1):
            occ[at][rng.random((ny, nz)) < 0.02] = 1
            occ[at, (at // 7) % ny, (at // 3) % nz] = 1
    elif kind == "full":
        occ[...] = 1
    elif kind == "floor":
        occ[:, :, 0][rng.random((nx, ny)) < 0.3] = 1
        occ[0, 0, 0] = 1
    else:
        assert kind == "empty"
    return occ


@functools.lru_cache(maxsize=None)
def _case(grid, kind):
    """(occupancy, resolution, scipy's field), computed once and shared, read-only."""
    from scipy import ndimage
    occ = _occupancy(grid, kind)
    res = 0.5 if kind == "half" else 0.2
    if occ.any():
        ref = np.minimum(res * ndimage.distance_transform_edt(occ == 0), 10000.0)
    else:
        ref = np.full(grid, 10000.0)
    occ.setflags(write=False)
    ref.setflags(write=False)
    return occ, res, ref


def _mapspec(grid, res, occ):
    return problem.MapSpec(tuple(grid), res, np.array([-grid[0] * res / 2, -grid[1] * res / 2, 0.0]), occ)


def _init(ctx, grid, res):
    mp = _mapspec(grid, res, None)
    ctx.init_sdf_map(mp.map_size, mp.origin, res)
    assert tuple(ctx.grid) == tuple(grid)


def _first_wrong(d, ref):
    bad = np.argwhere(d != ref)
    return (len(bad), tuple(bad[0]), d[tuple(bad[0])], ref[tuple(bad[0])]) if len(bad) else None


def test_rows_cover_every_plan_cell():
    """The rows reach every z sweep variant 1 .. 8 and the LDS-mask one, the z sweep strided and not, esdf_rows_kernel on
    and off, every (y, x) voxels-per-lane pair the plan can produce — with either source of the candidate lists, which
    together select the y sweep's instantiation — and slab tables possible and not.  (The pairs the plan can produce:
    nz % 8 == 0 gives 8 | 8; nz % 8 == 4 gives 4 | 8 or 4 | 4 by ny*nz % 8; anything else 1 | 1.)  The plan is asked for
    every row, so a row whose stated cell has moved fails here as well as in its own test."""
    plans = esdf_plan.plans([g for g, _, _ in ROWS])
    cells = [esdf_plan.cell(p) for p in plans]
    assert cells == [c for _, c, _ in ROWS]
    assert all(p["supported"] for p in plans)
    assert {c[0] for c in cells} == {1, 2, 3, 4, 5, 6, 7, 8, "lds"}
    assert {c[1] for c in cells} == {True, False}
    assert {c[2] for c in cells} == {True, False}
    assert {(c[3], c[4]) for c in cells} == {(8, 8), (4, 8), (4, 4), (1, 1)}
    assert {(c[2], c[3]) for c in cells} == {(r, v) for r in (True, False) for v in (8, 4, 1)}
    assert {c[5] for c in cells} == {True, False}
    # the grid-stride loop on two different y / x paths; the LDS-mask sweep with and without the packed sweeps
    assert len({(c[3], c[4]) for c in cells if c[1]}) >= 2
    assert {(c[3], c[4]) for c in cells if c[0] == "lds"} == {(8, 8), (1, 1)}
    # either side of every limit is a row
    grids = set(CELLS)
    for nz in (64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513):
        assert (6, 10, nz) in grids
    assert {(4, 6, 4095), (4, 6, 4096), (4, 2047, 8), (4, 2048, 8), (4, 2049, 8), (2, 32768, 8), (2048, 8, 8), (2049, 8, 8),
            (32768, 2, 4), (32768, 4, 8), (32765, 2, 4)} <= grids


@pytest.mark.gpu
@pytest.mark.parametrize("grid,kind", CASES, ids=[f"{'x'.join(map(str, g))}-{k}" for g, k in CASES])
def test_esdf_at_the_plans_limits_bit_exact(gtop, grid, kind):
    assert esdf_plan.cell(esdf_plan.plan(grid)) == CELLS[grid]
    occ, res, ref = _case(grid, kind)
    ctx = gtop.GtopContext(device=0)
    _init(ctx, grid, res)
    ctx.update_sdf_map(_mapspec(grid, res, occ).obstacle_points())
    d = ctx.get_sdf()
    ctx.close()
    if kind == "half":
        assert ref[19999, 0, 0] == 9999.5 and ref[20001, 0, 0] == 10000.0 and ref.max() == 10000.0
    assert np.array_equal(d, ref), (grid, kind, _first_wrong(d, ref))


# one shape per z sweep family (scalar masks, LDS masks) and the nx, ny and nz maxima
@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(6, 10, 512), (6, 10, 513), (32768, 2, 4), (2, 32768, 8), (4, 6, 4096)],
                         ids=lambda g: "x".join(map(str, g)))
def test_signed_deep_map_at_the_plans_limits_bit_exact(gtop, grid):
    """All occupied but one voxel: the second transform (the FREE instantiations) carries every distance along the long
    axis, past both saturations."""
    assert esdf_plan.cell(esdf_plan.plan(grid)) == CELLS[grid]
    occ = _occupancy(grid, "deep")
    res = 0.2
    ctx = gtop.GtopContext(device=0)
    ctx.set_field_sign(True, 0.0)
    _init(ctx, grid, res)
    ctx.update_sdf_map(_mapspec(grid, res, occ).obstacle_points())
    d = ctx.get_sdf()
    ctx.close()
    ref = signed_reference(occ, res, 0.0)
    assert ref.min() < -0.2 * 500                       # (deeper than both saturations)
    assert np.array_equal(d, ref), (grid, _first_wrong(d, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(4, 6, 4097), (32769, 2, 4), (2, 32769, 8)], ids=lambda g: "x".join(map(str, g)))
def test_refusals_past_the_whole_grid_limits(gtop, grid):
    """One past each whole-grid limit: the plan says unsupported, gtop_update_sdf_map returns GTOP_ERR_INVALID with the
    builder's message, and the same context then builds a small map correctly."""
    assert not esdf_plan.plan(grid)["supported"]
    res = 0.2
    occ = _occupancy(grid, "corner")
    ctx = gtop.GtopContext(device=0)
    _init(ctx, grid, res)
    with pytest.raises(gtop.GtopError) as e:
        ctx.update_sdf_map(_mapspec(grid, res, occ).obstacle_points())
    assert e.value.code == ERR_INVALID
    assert "grid too large for the device builder (nz <= 4096, nx, ny <= 32768)" in str(e.value)
    small = (20, 5, 4)
    occ, res, ref = _case(small, "ends")
    _init(ctx, small, res)
    ctx.update_sdf_map(_mapspec(small, res, occ).obstacle_points())
    d = ctx.get_sdf()
    ctx.close()
    assert np.array_equal(d, ref), _first_wrong(d, ref)


# large and small alternate, every step on another path of the plan; signed: the two-transform build
CHAIN = [((520, 520, 8), "ends", False), ((6, 10, 513), "floor", True), ((32768, 4, 8), "slabs3", False),
         ((4, 2047, 8), "ends", True), ((1040, 260, 4), "ends", False), ((6, 10, 512), "ends", True),
         ((2, 32768, 8), "ends", True), ((20, 5, 4), "ends", False)]


@pytest.mark.gpu
def test_one_context_rebuilds_across_the_plans_limits(gtop):
    """One context walked through eight of the shapes above.  The workspaces are grow-only and the sweeps leave parts of
    them unwritten on purpose (empty columns of the z sweep, the int32 output of unsaturated wavefronts), so each build
    runs over the previous one's leftovers in a different layout."""
    ctx = gtop.GtopContext(device=0)
    for step, (grid, kind, signed) in enumerate(CHAIN):
        assert esdf_plan.cell(esdf_plan.plan(grid)) == CELLS[grid]
        occ, res, ref = _case(grid, kind)
        ctx.set_field_sign(signed, 0.0)
        _init(ctx, grid, res)
        ctx.update_sdf_map(_mapspec(grid, res, occ).obstacle_points())
        d = ctx.get_sdf()
        if signed:
            ref = signed_reference(occ, res, 0.0)
        assert np.array_equal(d, ref), (step, grid, kind, signed, _first_wrong(d, ref))
    ctx.close()


@pytest.mark.gpu
def test_window_past_the_slab_tables_through_the_compact_path(gtop, oracle_mod):
    """A 2060 x 30 x 12 window of a 2100 x 40 x 16 map: the compact path builds a sub-grid past kEsdfSlabMax (no slab
    tables, although nearly every slab of it is empty) in a workspace laid out for the parent grid.  Bit for bit the
    oracle's window update, as tests/test_window_update.py."""
    grid, res = (2100, 40, 16), 0.2
    sub = (2060, 30, 12)
    assert esdf_plan.cell(esdf_plan.plan(grid)) == (1, False, False, 8, 8, False)
    assert esdf_plan.cell(esdf_plan.plan(sub)) == (1, False, False, 4, 8, False)
    assert esdf_plan.plan(sub)["rows_ints"] <= esdf_plan.plan(grid)["rows_ints"]
    rng = np.random.default_rng(21)
    origin = np.array([-grid[0] * res / 2, -grid[1] * res / 2, 0.0])
    map_size = (np.array(grid) - 0.5) * res
    sdf = oracle_mod.Sdf.from_map_size(origin, res, map_size)
    assert sdf.grid == grid
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(map_size, origin, res)
    assert tuple(ctx.grid) == grid
    first = (np.argwhere(rng.random(grid) < 0.002) + 0.5) * res + origin
    ctx.update_sdf_map(first)
    occ = np.zeros(int(np.prod(grid)))
    occ[:] = sdf.build_from_points(first)
    assert np.array_equal(ctx.get_sdf().reshape(-1), sdf.dist)
    a = origin + (np.array([20, 5, 2]) + 0.25) * res
    b = origin + (np.array([2080, 35, 14]) + 0.25) * res
    lo, hi = sdf.window_ids(a, b)
    assert tuple(np.asarray(hi) - np.asarray(lo) + 1) == sub
    vox = np.array([[20, 5, 2], [2079, 34, 13], [1050, 20, 7], [1051, 6, 13], [400, 33, 2]])   # the window's corners and inside
    pts = (vox + 0.5) * res + origin
    ctx.update_sdf_map_window(a, b, pts)
    sdf.update_window(occ, a, b, pts)
    d = ctx.get_sdf().reshape(-1)
    ctx.close()
    assert np.array_equal(d, sdf.dist), _first_wrong(d, sdf.dist)
