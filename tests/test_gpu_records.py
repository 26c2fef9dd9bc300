"""The corner records (csrc/gtop_records.hip) densely: every cell of the map after every way of building
them.  Every lookup of the library reads the records, a derived copy of the field with clamped border copies and two
padding levels, maintained by five builder forms (whole map fp64, whole map both precisions two rows per lane, the two
restricted to a voxel box, <double,float> and <float,float>) chosen by the context's history (GtopField in
csrc/gtop_ctx.h and gtop_capi_field.cpp: the fp64 records current or not, the fp32 ones absent / stale / current, fp32 in
use, fp32 wanted, the grow-only buffers).  The rest of the suite sees them only where a
random batch happens to pass; here one probe row per cell (tests/records_probe.py; its soundness:
tests/test_records_probe.py) reads every record, the border and padding ones included, after every step.

check_records(ctx, ...) after any step — the records are a function of ctx.get_sdf() and of nothing else:
  (a) field = ctx.get_sdf(); an oracle Sdf of the same geometry holding it;
  (b) gtop_edt_query at 4 positions per cell against the oracle's lookup: distance to rtol = atol = 1e-13, gradient to
      1e-12 (the tolerances of tests/test_gpu_edt.py), never -1; a failure names the cell;
  (c) the fp64 evaluation of the probe rows (ws = 0) at the launch rule and with 3, 6, 10 and 30 samples per lane
      pinned, entry by entry to tests/test_gpu_entrywise.check;
  (d) where fp32 is asked for: the fp32 evaluation (inputs rounded to float) at the same geometries through the same
      check, and BIT FOR BIT against a fresh context without history that was handed (float)field as a borrowed fp32
      tensor — every fp32 builder form must leave (float)D in every record;
  (e) once per module, (c) and (d) on 1024 six-segment rows, which the launch rule (up to 6 segments,
      below 3072 trajectories) sends to the lone-wavefront body with hand-issued loads and the v_med3 index form.

The grids (res 0.2, map_size = grid * res) are the smallest that reach each edge of the builder:
  (2, 2, 2)     the minimum grid; a wavefront spans several row tiles (2 (nz + 2) = 8 lanes per tile row)
  (3, 8, 2)     ny + 1 = 9: a second tile of one row — the two-row path's single-row tail
  (9, 7, 5)     ny + 1 = 8: one full tile; nx + 1 = 10 slabs over 8 XCDs
  (8, 15, 4)    nx + 1 = 9
  (17, 16, 33)  ny + 1 = 17; more than 256 half records per tile row, a partial last block
  (25, 24, 7)   room for compact windows (>= 12 x 12 x 3)

Since the fp32 bound sees 96-97 % of single wrong corners per field (test_records_probe.py), every fp32 check on a
probe field runs on two field seeds.

What it found: the records were right; gtop_edt_query was not where (b) holds it.  test_window_rebuilds[(25, 24, 7)-
no-new-points] sends a box of voxels back to 10000; in the cells across its edge a gradient component cancels (v1 - v0 =
0.03 at |v| = 5750), and the kernel's fused multiply-adds left the oracle's unfused arithmetic by up to 6.5e-11 in a
gradient entry, 1.7e-11 past 1e-12 + 1e-12 |g| (89 of 20 800 positions, cells ix = 3 beside the window's lo_x = 4).
The static lookup is unfused since (gtop_edt_lookup.h): on that field all 20 800 distances and 62 400 gradient entries
now equal the oracle's bit for bit.  The case stays as the regression test.

Measured on an MI355X, largest |err| / (u * mag) over every check of this file (GTOP_ENTRYWISE_LOG): (c) fp64 cost 79,
gradient 0.05 (bound KAPPA64 = 4096); (d) fp32 cost 4.6, gradient 0.42 (KAPPA32 = 1024); the six-segment rows of (e)
fp64 40 / 0.009, fp32 1.9 / 0.001; no tie rows, no overflow.

What a one-line value change of gtop_records.hip does to these checks (each keeps every index inside the buffers):
  * the window's upper record bound b + 1 -> b (x or y): the record row / slab whose LOWER corner is the window's last
    voxel keeps the old field; every window case that does not end at the grid's last voxel leaves it stale, and (b),
    (c), (d) read it — in that case and in every later one on the same context;
  * lo = hiB -> lo = hiA in the two-row loop: the lower corners of the third, fifth and seventh row of every tile repeat
    the row before, in BOTH precisions; every step taken with fp32 in use fails on every grid with ny + 1 >= 3;
  * first = cx0 + ((xcd - cx0) & 7) -> cx0 + (xcd & 7): NOT a value change — over xcd = 0 .. 7 both forms visit every
    slab cx0 .. cx1 exactly once (enumerated for all windows up to 60 slabs); only the slab's XCD changes.  Its value-
    changing neighbour, first = (xcd - cx0) & 7, rebuilds slabs below the window instead of its last ones: the lox-*
    window cases.
"""
import functools

import numpy as np
import pytest

from tests import records_probe as rp
from tests.test_gpu_entrywise import KAPPA32, KAPPA64, U32, U64, check

pytestmark = pytest.mark.gpu

GEOS = [(0, 0), (0, 3), (0, 6), (0, 10), (0, 30)]
LONE_M, LONE_ROWS = 6, 1024            # (e): up to 6 segments, below 3072 trajectories: the lone-wavefront body
PARAMS = dict(ws=0.0)
FAR_PARAMS = dict(ws=0.0, r=4000.0)


class Probe:
    """The probe of one grid: geometry, rows (host, float-rounded, and on the device in both precisions), queries."""

    def __init__(self, grid, m=2, count=None):
        import torch
        self.grid = tuple(int(g) for g in grid)
        self.origin, self.map_size = rp.geometry(self.grid)
        self.cells = rp.cells(self.grid)
        T, Df, x = rp.probe_rows(self.grid, self.origin, rp.RES, m=m, seed=0, count=count)
        self.row_cell = self.cells[np.arange(len(x)) % len(self.cells)]
        self.host = {"f64": (T, Df, x),
                     "f32": tuple(np.asarray(a, dtype=np.float32).astype(np.float64) for a in (T, Df, x))}   # as _f32_batch
        dev = torch.device("cuda:0")
        self.dev = {k: tuple(torch.tensor(a, dtype=td, device=dev) for a in (v[2], v[1].reshape(-1, 18), v[0]))
                    for (k, v), td in zip(self.host.items(), (torch.float64, torch.float32))}
        self.qpos, self.qcell = rp.probe_queries(self.grid, self.origin, rp.RES, per_cell=4, seed=0)


@functools.lru_cache(maxsize=None)
def probe(grid, m=2, count=None):
    return Probe(grid, m, count)


def _eval(ctx, tensors, geo):
    import torch
    ctx.set_launch_geometry(*geo)
    try:
        c, g = ctx.eval_device(*tensors)
        torch.cuda.synchronize()
    finally:
        ctx.set_launch_geometry(0, 0)
    return c, g


def _query_all(oracle_mod, sdf, pos):
    """sdf.query at every position (the same C call, without a Python object per position)."""
    import ctypes as C
    L, dp = oracle_mod.lib(), C.POINTER(C.c_double)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    d, g = np.empty(len(pos)), np.empty((len(pos), 3))
    pa, ga, ref = pos.ctypes.data, g.ctypes.data, C.byref(sdf.c)
    for i in range(len(pos)):
        d[i] = L.oracle_sdf_query(ref, C.cast(pa + 24 * i, dp), C.cast(ga + 24 * i, dp))
    return d, g


def _entrywise(pr, c, g, ref, dtype, what):
    """tests/test_gpu_entrywise.check, its failure extended by the cells of the rows beyond the bound."""
    c, g = c.double().cpu().numpy(), g.double().cpu().numpy()
    try:
        return check(c, g, ref, dtype, what)
    except AssertionError as e:
        c_ref, g_ref, cm, gm, _, cf, gf = ref
        kappa, u = (KAPPA32, U32) if dtype == "f32" else (KAPPA64, U64)
        with np.errstate(invalid="ignore"):
            bad = ~(np.abs(c - c_ref) <= kappa * u * cm + cf) | ~(np.abs(g - g_ref) <= kappa * u * gm + gf).all(axis=1)
        rows = np.flatnonzero(bad)
        raise AssertionError(f"{e}\n{len(rows)} rows beyond the bound; the first read the cells (ix, iy, iz) "
                             f"{pr.row_cell[rows[:8]].tolist()}") from None


def _same_bits(pr, ours, theirs, what):
    same = (ours[0] == theirs[0]) & (ours[1] == theirs[1]).all(dim=1)
    if not bool(same.all()):
        rows = np.flatnonzero(~same.cpu().numpy())
        raise AssertionError(f"{what}: the fp32 evaluation differs from a fresh context's on the same (float) field in "
                             f"{len(rows)} rows; the first read the cells (ix, iy, iz) {pr.row_cell[rows[:8]].tolist()}")


def check_records(ctx, oracle_mod, fp32, what="", field=None, only32=False, pr=None, geos=GEOS):
    """(a)-(d) of the module docstring.  field / only32: a context without an fp64 field (a borrowed fp32 tensor):
    the field it was given, and (d) alone.  pr: another probe of the same grid ((e): the six-segment rows)."""
    import torch
    gtop_mod = __import__("grad_traj_optimization_amd")
    if field is None:
        field = ctx.get_sdf()                                                                            # (a)
    grid = tuple(field.shape)
    pr = pr or probe(grid)
    assert pr.grid == grid
    sdf = oracle_mod.Sdf.from_map_size(pr.origin, rp.RES, pr.map_size)
    assert sdf.grid == grid
    sdf.dist[:] = field.reshape(-1)
    ctx.set_params(**PARAMS)
    prm = oracle_mod.make_params(**PARAMS)
    if not only32:
        d_ref, g_ref = _query_all(oracle_mod, sdf, pr.qpos)                                              # (b)
        d, g = ctx.edt_query(pr.qpos, -1.0)
        assert (d_ref != -1).all()
        bad = (d == -1) | ~np.isclose(d, d_ref, rtol=1e-13, atol=1e-13) | ~np.isclose(g, g_ref, rtol=1e-12, atol=1e-12).all(axis=1)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{what} {grid}: gtop_edt_query differs from the oracle's lookup at {int(bad.sum())} of "
                                 f"{len(bad)} positions, in the cells (ix, iy, iz) {np.unique(pr.qcell[bad], axis=0)[:8].tolist()}; "
                                 f"first: cell {pr.qcell[i].tolist()} at {pr.qpos[i].tolist()}: {d[i]!r} {g[i].tolist()} "
                                 f"against {d_ref[i]!r} {g_ref[i].tolist()}")
        ref = oracle_mod.eval_batch_mag(*pr.host["f64"], sdf, prm, nthreads=8)                          # (c)
        for geo in geos:
            c, g = _eval(ctx, pr.dev["f64"], geo)
            _entrywise(pr, c, g, ref, "f64", ("records", what, grid, geo))
    if not fp32:
        return
    ref32 = oracle_mod.eval_batch_mag(*pr.host["f32"], sdf, prm, nthreads=8)                            # (d)
    f32 = torch.tensor(field, dtype=torch.float32, device="cuda:0").contiguous()
    fresh = gtop_mod.GtopContext(device=0, params=PARAMS)
    try:
        fresh.set_sdf_device(f32, grid, pr.origin, rp.RES, map_size=pr.map_size)
        for geo in geos:
            c, g = _eval(ctx, pr.dev["f32"], geo)
            _entrywise(pr, c, g, ref32, "f32", ("records", what, grid, geo))
            _same_bits(pr, (c, g), _eval(fresh, pr.dev["f32"], geo), f"{what} {grid} {geo}")
        # ... and once with a penalty that still varies at the 10000 of a line or box without obstacles (r = 4000: with
        # the scene's r = 0.5 it underflows past a few metres, and a wrong record among free voxels would not show)
        for c_ in (ctx, fresh):
            c_.set_params(**FAR_PARAMS)
        try:
            _same_bits(pr, _eval(ctx, pr.dev["f32"], geos[0]), _eval(fresh, pr.dev["f32"], geos[0]), f"{what} {grid} r = 4000")
        finally:
            ctx.set_params(**PARAMS)
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------

def _points(grid, origin, seed, density=0.15, lo=None, hi=None):
    """Voxel centres of a random `density` of the voxels of the box [lo, hi] (default: the grid): dense, so that the
    ESDF's values stay near d0 where the penalty sees them, besides the 10000 of a line or box without an obstacle."""
    lo = np.zeros(3, dtype=int) if lo is None else np.asarray(lo)
    hi = np.asarray(grid) - 1 if hi is None else np.asarray(hi)
    shape = tuple(int(v) for v in hi - lo + 1)
    take = np.random.default_rng([int(seed), 20263]).random(shape) < density
    take.flat[int(seed) % take.size] = True              # (never empty, and not the same voxels for two seeds in a row)
    idx = np.argwhere(take) + lo
    return (idx + 0.5) * rp.RES + origin


def _map_context(gtop, grid, seed=0):
    pr = probe(grid)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(pr.map_size, pr.origin, rp.RES)
    assert tuple(ctx.grid) == pr.grid
    ctx.update_sdf_map(_points(grid, pr.origin, seed))
    return ctx, pr


def _run_fp32(ctx, pr):
    """One fp32 evaluation: from here on the context keeps fp32 records."""
    _eval(ctx, pr.dev["f32"], (0, 0))


def _box_positions(pr, lo, hi):
    """Positions whose window (sdf_map.cpp:28-45: posToIndex(min), posToIndex(max - res / 2)) is the voxel box."""
    return pr.origin + (np.asarray(lo) + 0.25) * rp.RES, pr.origin + (np.asarray(hi) + 1.25) * rp.RES


def _window(ctx, pr, oracle_mod, lo, hi, seed, device, with_points=True):
    import torch
    a, b = _box_positions(pr, lo, hi)
    sdf = oracle_mod.Sdf.from_map_size(pr.origin, rp.RES, pr.map_size)
    wlo, whi = sdf.window_ids(a, b)
    assert wlo.tolist() == list(lo) and whi.tolist() == list(hi), (lo, hi, wlo, whi)
    pts = _points(pr.grid, pr.origin, seed, lo=lo, hi=hi) if with_points else np.zeros((0, 3))
    if device:
        ctx.update_sdf_map_window_device(a, b, torch.tensor(pts.reshape(-1, 3), dtype=torch.float64, device="cuda:0"))
        torch.cuda.synchronize()
    else:
        ctx.update_sdf_map_window(a, b, pts)


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", rp.GRIDS, ids=[str(g) for g in rp.GRIDS])
def test_whole_map_builds(gtop, oracle_mod, grid):
    import torch
    pr = probe(grid)
    ctx = gtop.GtopContext(device=0)
    try:
        # fp64 only; the first fp32 use builds <double, float> from stale records
        ctx.set_sdf(rp.probe_field(grid, 0), grid, pr.origin, rp.RES, map_size=pr.map_size)
        check_records(ctx, oracle_mod, True, "set_sdf, then the first fp32 use")
        # fp32 in use: both precisions in one pass (two rows per lane)
        ctx.set_sdf(rp.probe_field(grid, 1), grid, pr.origin, rp.RES, map_size=pr.map_size)
        check_records(ctx, oracle_mod, True, "set_sdf with fp32 in use")
        ctx.init_sdf_map(pr.map_size, pr.origin, rp.RES)
        ctx.update_sdf_map(_points(grid, pr.origin, 2))
        field = ctx.get_sdf()
        assert field.min() == 0.0 and field.max() <= 10000.0
        check_records(ctx, oracle_mod, True, "init_sdf_map + update_sdf_map")
        ctx.update_sdf_map_device(torch.tensor(_points(grid, pr.origin, 3), dtype=torch.float64, device="cuda:0"))
        torch.cuda.synchronize()
        assert not np.array_equal(ctx.get_sdf(), field)
        check_records(ctx, oracle_mod, True, "update_sdf_map_device")
    finally:
        ctx.close()


def test_lone_wavefront_body_reads_every_record(gtop, oracle_mod):
    """(e): six-segment rows, 1024 of them: the launch rule's lone-wavefront body (hand-issued loads, v_med3 index)."""
    grid = (9, 7, 5)
    pr6 = probe(grid, LONE_M, LONE_ROWS)
    ctx = gtop.GtopContext(device=0)
    try:
        for seed in (0, 1):
            ctx.set_sdf(rp.probe_field(grid, seed), grid, pr6.origin, rp.RES, map_size=pr6.map_size)
            check_records(ctx, oracle_mod, True, f"six segments, field seed {seed}", pr=pr6, geos=[(0, 0)])
    finally:
        ctx.close()


WALK = [(25, 24, 7), (3, 8, 2), (17, 16, 33), (9, 7, 5)]


@pytest.mark.parametrize("how", ["set_sdf", "borrowed-f64", "borrowed-f32"])
def test_grid_changes_reuse_the_buffers(gtop, oracle_mod, how):
    """One context walks large -> small -> larger -> small: the record buffers only grow, the records of a smaller grid
    live at the front of a buffer that still holds the previous grid's.  Two field seeds per grid."""
    import torch
    ctx = gtop.GtopContext(device=0)
    try:
        if how != "set_sdf":        # the same history in front of the borrowed walks: one context all along
            g0 = WALK[0]
            ctx.set_sdf(rp.probe_field(g0, 5), g0, probe(g0).origin, rp.RES, map_size=probe(g0).map_size)
            _run_fp32(ctx, probe(g0))
        for grid in WALK:
            pr = probe(grid)
            for seed in (0, 1):
                field = rp.probe_field(grid, 10 * len(how) + seed)
                if how == "set_sdf":
                    ctx.set_sdf(field, grid, pr.origin, rp.RES, map_size=pr.map_size)
                    check_records(ctx, oracle_mod, True, f"{how} seed {seed}")
                elif how == "borrowed-f64":
                    t = torch.tensor(field, dtype=torch.float64, device="cuda:0")
                    ctx.set_sdf_device(t, grid, pr.origin, rp.RES, map_size=pr.map_size)
                    assert np.array_equal(ctx.get_sdf(), field)
                    check_records(ctx, oracle_mod, True, f"{how} seed {seed}")
                else:
                    # gtop.h: a GTOP_F32 field serves fp32 evaluations only — no fp64 field is resident: gtop_get_sdf,
                    # gtop_edt_query and fp64 evaluations refuse (GTOP_ERR_STATE), (d) alone is left
                    t = torch.tensor(field, dtype=torch.float32, device="cuda:0")
                    ctx.set_sdf_device(t, grid, pr.origin, rp.RES, map_size=pr.map_size)
                    for refused in (ctx.get_sdf, lambda: ctx.edt_query(pr.qpos[:4], -1.0),
                                    lambda: ctx.eval_device(*pr.dev["f64"])):
                        with pytest.raises(gtop.GtopError):
                            refused()
                    check_records(ctx, oracle_mod, True, f"{how} seed {seed}", field=t.double().cpu().numpy(), only32=True)
    finally:
        ctx.close()


def _window_cases(grid):
    """(name, lo, hi, with_points) voxel boxes; None = the window that clips to nothing."""
    nx, ny, nz = grid
    hx, hy, hz = nx - 1, ny - 1, nz - 1
    cases = [
        ("sliver", (5, 3, 1), (9, hy - 2, min(hz, 4)), True),                   # < 12 wide: the plain window kernels
        ("compact", (2, 1, 1), (14, 13, min(hz, 5)), True),                     # >= 12 x 12 x 3: the compact path
        ("low-corner", (0, 0, 0), (3, 4, 1), True),
        ("high-corner", (hx - 4, hy - 3, hz - 2), (hx, hy, hz), True),
        ("face-x0", (0, 0, 0), (2, hy, hz), True),
        ("face-yhi", (0, hy - 1, 0), (hx, hy, hz), True),
        ("face-z0-compact", (0, 0, 0), (hx, hy, 2), True),
        ("lox-1", (1, 2, 1), (6, 8, 3), True),                                  # lo_x % 8 = 1, 7 (slabs start off XCD 0)
        ("lox-7", (7, 5, 0), (12, 9, 2), True),
        ("lox-9", (9, 2, 0), (hx, 14, 3), True),                                # (compact where the grid leaves 12 voxels)
    ]
    for parity in (0, 1):                                                       # lo_y even / odd, every tile-edge height
        for h in (1, 2, 7, 8, 9):
            lo_y = 4 + parity
            cases.append((f"loy-{'odd' if parity else 'even'}-h{h}", (3, lo_y, 1), (10, lo_y + h - 1, 3), True))
    cases += [
        ("no-new-points", (4, 2, 1), (11, 10, 3), False),                       # its voxels go back to 10000
        ("empty", None, None, True),                                            # clips to nothing: nothing changes
        ("whole-map", (0, 0, 0), (hx, hy, hz), True),
    ]
    return cases


WINDOW_GRIDS = [(25, 24, 7), (17, 16, 33)]
WINDOW_IDS = [(g, k) for g in WINDOW_GRIDS for k in range(len(_window_cases(g)))]


@pytest.fixture(scope="module")
def window_contexts(gtop):
    held = {}
    yield held
    for ctx in held.values():
        ctx.close()


@pytest.mark.parametrize("grid,k", WINDOW_IDS, ids=[f"{g}-{_window_cases(g)[k][0]}" for g, k in WINDOW_IDS])
def test_window_rebuilds(gtop, oracle_mod, window_contexts, grid, k):
    """One window per case on ONE context per grid, in sequence (a row left stale by an earlier window stays wrong:
    every later check reads every record), the host and the device entry alternating; fp32 in use, so both precisions
    are rebuilt for the window in one pass."""
    name, lo, hi, with_points = _window_cases(grid)[k]
    pr = probe(grid)
    if grid not in window_contexts:
        window_contexts[grid], _ = _map_context(gtop, grid, seed=4)
        _run_fp32(window_contexts[grid], pr)
    ctx = window_contexts[grid]
    before = ctx.get_sdf()
    if lo is None:
        import torch
        a, b = pr.origin + pr.map_size + 1.0, pr.origin + pr.map_size + 2.0
        pts = _points(grid, pr.origin, 50 + k, density=0.01)
        if k % 2:
            ctx.update_sdf_map_window_device(a, b, torch.tensor(pts, dtype=torch.float64, device="cuda:0"))
            torch.cuda.synchronize()
        else:
            ctx.update_sdf_map_window(a, b, pts)
        assert np.array_equal(ctx.get_sdf(), before)
    else:
        assert all(0 <= l <= h < n for l, h, n in zip(lo, hi, grid)), (name, lo, hi)
        _window(ctx, pr, oracle_mod, lo, hi, 50 + k, device=bool(k % 2), with_points=with_points)
        after = ctx.get_sdf()
        box = tuple(slice(l, h + 1) for l, h in zip(lo, hi))
        assert not np.array_equal(after[box], before[box]), name
        after[box] = before[box]
        assert np.array_equal(after, before), (name, "the field changed outside the window")
        if not with_points:
            assert (ctx.get_sdf()[box] == 10000.0).all()
    check_records(ctx, oracle_mod, True, f"window {name} {lo} .. {hi}, {'device' if k % 2 else 'host'} entry")


def test_fp32_bookkeeping(gtop, oracle_mod):
    """Which fp32 records a context holds — current, stale, none — after each order of calls."""
    import torch
    grid = (25, 24, 7)
    lo, hi = (7, 3, 1), (12, 11, 4)
    # never ran fp32, host window: the fp32 records stay stale; the first fp32 evaluation builds them whole
    ctx, pr = _map_context(gtop, grid, seed=6)
    try:
        check_records(ctx, oracle_mod, False, "never ran fp32")
        _window(ctx, pr, oracle_mod, lo, hi, 60, device=False)
        check_records(ctx, oracle_mod, False, "never ran fp32: host window")
        check_records(ctx, oracle_mod, True, "never ran fp32: host window, then the first fp32 evaluation")
    finally:
        ctx.close()
    # never ran fp32, device window: fp32 is rebuilt whole behind it
    ctx, pr = _map_context(gtop, grid, seed=7)
    try:
        _window(ctx, pr, oracle_mod, lo, hi, 61, device=True)
        check_records(ctx, oracle_mod, True, "never ran fp32: device window")
        _window(ctx, pr, oracle_mod, (1, 2, 0), (9, 9, 2), 62, device=True)
        check_records(ctx, oracle_mod, True, "device window on current fp32 records")
    finally:
        ctx.close()
    # fp32 switched off: window, whole-map update, an fp32 evaluation is refused; switched on again: rebuilt
    ctx, pr = _map_context(gtop, grid, seed=8)
    try:
        _run_fp32(ctx, pr)
        ctx.set_field_precisions(False)
        _window(ctx, pr, oracle_mod, lo, hi, 63, device=False)
        check_records(ctx, oracle_mod, False, "fp32 off: host window")
        _window(ctx, pr, oracle_mod, (1, 2, 0), (9, 9, 2), 64, device=True)
        check_records(ctx, oracle_mod, False, "fp32 off: device window")
        ctx.update_sdf_map(_points(grid, pr.origin, 65))
        check_records(ctx, oracle_mod, False, "fp32 off: update_sdf_map")
        with pytest.raises(gtop.GtopError):
            ctx.eval_device(*pr.dev["f32"])
        torch.cuda.synchronize()
        ctx.set_field_precisions(True)
        check_records(ctx, oracle_mod, True, "fp32 on again")
    finally:
        ctx.close()
    # fp32 current: off and on again with no field change in between
    ctx, pr = _map_context(gtop, grid, seed=9)
    try:
        check_records(ctx, oracle_mod, True, "fp32 current")
        ctx.set_field_precisions(False)
        ctx.set_field_precisions(True)
        check_records(ctx, oracle_mod, True, "fp32 off and on, no field change")
        # ... and a window behind the toggle, while the fp32 records are still stale: they follow whole
        ctx.set_field_precisions(False)
        ctx.set_field_precisions(True)
        _window(ctx, pr, oracle_mod, lo, hi, 66, device=False)
        check_records(ctx, oracle_mod, True, "fp32 off and on, then a host window on stale fp32 records")
    finally:
        ctx.close()


STEPS = ["set_sdf", "update_sdf_map", "update_sdf_map_device", "window", "window_device", "fp32_eval", "toggle"]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_histories(gtop, oracle_mod, seed):
    """25 random steps on one context.  The test keeps no model beyond "the records are a function of get_sdf()": two
    flags say whether fp32 is switched on and whether an fp32 evaluation has run (before one, checking fp32 would be
    the step "first fp32 evaluation" itself).  The fp32 check is left out right after a toggle, so that the next step
    meets the records as the toggle left them."""
    import torch
    rng = np.random.default_rng([seed, 20264])
    grid = rp.GRIDS[int(rng.integers(len(rp.GRIDS)))]
    ctx, pr = _map_context(gtop, grid, seed=100 + seed)
    on, used = True, False
    n = np.array(grid)
    history = []
    try:
        for it in range(25):
            step = STEPS[int(rng.integers(len(STEPS)))]
            history.append(step)
            s = 1000 * seed + it
            if step == "set_sdf":
                ctx.set_sdf(rp.probe_field(grid, s), grid, pr.origin, rp.RES, map_size=pr.map_size)
            elif step == "update_sdf_map":
                ctx.update_sdf_map(_points(grid, pr.origin, s))
            elif step == "update_sdf_map_device":
                ctx.update_sdf_map_device(torch.tensor(_points(grid, pr.origin, s), dtype=torch.float64, device="cuda:0"))
                torch.cuda.synchronize()
            elif step in ("window", "window_device"):
                lo = rng.integers(0, n)
                hi = np.minimum(lo + rng.integers(0, np.maximum(n * 3 // 4, 1)), n - 1)
                _window(ctx, pr, oracle_mod, lo.tolist(), hi.tolist(), s, device=step == "window_device",
                        with_points=bool(rng.random() < 0.8))
            elif step == "fp32_eval":
                if on:
                    _run_fp32(ctx, pr)
                    used = True
                else:
                    with pytest.raises(gtop.GtopError):
                        ctx.eval_device(*pr.dev["f32"])
            else:
                on = not on
                ctx.set_field_precisions(on)
            check_records(ctx, oracle_mod, on and used and step != "toggle", f"seed {seed}, history {history}")
    finally:
        ctx.close()
