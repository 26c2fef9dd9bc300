"""The signed distance field (include/gtop.h, gtop_set_field_sign) on the MI355X: the builds bit for bit against scipy's
exact transforms, its properties against the unsigned field, every consumer of the field on it, and what it is for —
trajectories optimised out of a pillar that the unsigned field leaves them stuck in."""
import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import scenes

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4


def signed_reference(occ, res, max_depth):
    """Free voxels: res * (distance to the nearest occupied voxel), 10000 without one; occupied voxels:
    max(-D, res - res * (distance to the nearest free voxel)), -D without one; D = max_depth, 0 meaning 10000."""
    from scipy import ndimage
    D = 10000.0 if max_depth == 0 else float(max_depth)
    occ = occ == 1
    out = np.empty(occ.shape)
    out[~occ] = res * ndimage.distance_transform_edt(~occ)[~occ] if occ.any() else 10000.0
    if occ.any():
        out[occ] = np.maximum(-D, res - res * ndimage.distance_transform_edt(occ)[occ]) if (~occ).any() else -D
    return out


def unsigned_reference(occ, res):
    from scipy import ndimage
    return res * ndimage.distance_transform_edt(occ == 0) if (occ == 1).any() else np.full(occ.shape, 10000.0)


def _ctx(gtop, grid, res, signed=True, max_depth=0.0):
    mp = problem.MapSpec(tuple(grid), res, np.array([-grid[0] * res / 2, -grid[1] * res / 2, 0.0]),
                         np.zeros(grid, dtype=np.uint8))
    ctx = gtop.GtopContext(device=0)
    ctx.set_field_sign(signed, max_depth)
    ctx.init_sdf_map(mp.map_size, mp.origin, res)
    assert tuple(ctx.grid) == tuple(grid)
    return ctx, mp


def _build(ctx, mp, occ):
    ctx.update_sdf_map(problem.MapSpec(mp.grid, mp.resolution, mp.origin, occ).obstacle_points())
    return ctx.get_sdf()


def _fixed_maps():
    maps = []
    g = (24, 20, 16)
    maps.append(("empty", np.zeros(g, np.uint8)))
    maps.append(("full", np.ones(g, np.uint8)))
    one = np.zeros(g, np.uint8); one[5, 7, 9] = 1
    maps.append(("single", one))
    hole = np.ones(g, np.uint8); hole[23, 0, 15] = 0
    maps.append(("single free voxel", hole))
    slab = np.zeros((40, 32, 24), np.uint8); slab[10:22] = 1; slab[:, :, 3:9] = 1
    maps.append(("slabs", slab))
    for shape in ((300, 4, 8), (8, 300, 8), (8, 8, 300), (520, 16, 8), (6, 5, 301), (7, 270, 6)):
        line = np.zeros(shape, np.uint8); line[(0,) * 3] = 1                    # past 255 voxels: saturated scans
        maps.append((f"line {shape}", line))
        deep = np.ones(shape, np.uint8); deep[(0,) * 3] = 0                     # ... and the interior transform's
        maps.append((f"deep {shape}", deep))
    cube = np.zeros((64, 48, 40), np.uint8); cube[8:56, 4:44, 2:38] = 1          # a thick box, nz % 8 == 0
    maps.append(("box", cube))
    odd = np.zeros((33, 29, 27), np.uint8); odd[3:30, 5:20, :] = 1              # nz odd: one voxel per lane
    maps.append(("odd box", odd))
    return maps


@pytest.mark.parametrize("max_depth", [0.0, 0.5])
def test_signed_build_fixed_shapes_are_scipys_exact_transforms(gtop, max_depth):
    res = 0.2
    for name, occ in _fixed_maps():
        ctx, mp = _ctx(gtop, occ.shape, res, True, max_depth)
        d = _build(ctx, mp, occ)
        ref = signed_reference(occ, res, max_depth)
        assert np.array_equal(d, ref), (name, max_depth, int((d != ref).sum()))
        assert ctx.field_sign() == (True, max_depth)
        ctx.close()


def _random_map(rng):
    shape = [int(rng.choice([3, 8, 16, 24, 40, 64, 72])) for _ in range(3)]
    shape[int(rng.integers(0, 3))] = int(rng.choice([130, 264, 300]))
    if rng.random() < 0.3:
        shape = [int(v) for v in rng.integers(2, 50, size=3)]
    while shape[0] * shape[1] * shape[2] > 2_000_000:
        shape[int(np.argsort(shape)[1])] //= 2
    grid = tuple(max(2, v) for v in shape)
    occ = np.zeros(grid, dtype=np.uint8)
    kind = rng.choice(["boxes", "dense", "sparse", "mostly full"])
    if kind == "boxes":
        for _ in range(int(rng.integers(1, 12))):
            lo = [int(rng.integers(0, g)) for g in grid]
            hi = [min(g, a + int(rng.integers(1, max(2, g // 2)))) for a, g in zip(lo, grid)]
            occ[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    elif kind == "dense":
        occ[rng.random(grid) < 0.5] = 1
    elif kind == "sparse":
        occ[rng.random(grid) < 0.02] = 1
    else:
        occ[rng.random(grid) < 0.97] = 1
    return grid, occ, kind


@pytest.mark.parametrize("seed", range(40))
def test_signed_build_random_maps_are_scipys_exact_transforms(gtop, seed):
    rng = np.random.default_rng(9100 + seed)
    if seed == 0:
        mp = problem.make_map(200, density=0.05, seed=3, box_vox=(6, 30))
        grid, occ, kind = mp.grid, mp.occupancy, "200^3"
    else:
        grid, occ, kind = _random_map(rng)
    res = float(rng.choice([0.1, 0.2, 0.25]))
    max_depth = float(rng.choice([0.0, 0.3, 1.0]))
    ctx, mp = _ctx(gtop, grid, res, True, max_depth)
    d = _build(ctx, mp, occ)
    ref = signed_reference(occ, res, max_depth)
    assert np.array_equal(d, ref), (grid, kind, max_depth, int((d != ref).sum()))
    # a second build on the same context: nothing of the first survives in the workspaces
    occ2 = np.zeros(grid, dtype=np.uint8)
    occ2[tuple(int(v) for v in rng.integers(0, grid))] = 1
    assert np.array_equal(_build(ctx, mp, occ2), signed_reference(occ2, res, max_depth)), (grid, kind, "rebuild")
    ctx.close()


def test_signed_build_400x400x40_slab(gtop):
    mp0 = problem.make_map((400, 400, 40), density=0.04, seed=5, box_vox=(4, 40))
    occ = mp0.occupancy.copy()
    occ[:, :, 4:14] = 1                                                      # a slab ten voxels thick
    for max_depth in (0.0, 0.4):
        ctx, mp = _ctx(gtop, occ.shape, 0.2, True, max_depth)
        d = _build(ctx, mp, occ)
        assert np.array_equal(d, signed_reference(occ, 0.2, max_depth)), max_depth
        ctx.close()


def _window_ref(prev, occ, lo, hi, res, max_depth):
    out = prev.copy()
    box = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
    out[box] = signed_reference(occ[box], res, max_depth)
    return out


@pytest.mark.parametrize("max_depth", [0.0, 0.6])
def test_signed_window_updates_are_box_local_transforms(gtop, max_depth):
    """The compact path (windows of at least 12 x 12 x 3 voxels) and the small-window kernels, windows touching the
    border, a sequence on one context: the box is the signed transform of the box taken alone, the rest unchanged."""
    rng = np.random.default_rng(77)
    grid, res = (48, 40, 36), 0.2
    occ = np.zeros(grid, np.uint8)
    occ[10:30, 8:30, 0:20] = 1
    ctx, mp = _ctx(gtop, grid, res, True, max_depth)
    field = _build(ctx, mp, occ)
    assert np.array_equal(field, signed_reference(occ, res, max_depth))
    windows = [((4, 4, 2), (30, 33, 25)), ((0, 0, 0), (20, 15, 10)), ((30, 25, 20), (47, 39, 35)),   # compact
               ((5, 3, 0), (9, 30, 35)), ((0, 10, 4), (47, 20, 5)), ((40, 0, 30), (47, 39, 35))]      # slivers
    for lo, hi in windows:
        box = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
        occ[box] = 0
        sub = occ[box]
        a0 = [int(rng.integers(0, s)) for s in sub.shape]
        a1 = [min(s, a + int(rng.integers(1, s + 1))) for a, s in zip(a0, sub.shape)]
        sub[a0[0]:a1[0], a0[1]:a1[1], a0[2]:a1[2]] = 1                             # a box, deep where it can be
        sub[rng.random(sub.shape) < 0.05] = 1
        pts = (np.argwhere(sub == 1) + np.array(lo) + 0.5) * res + mp.origin
        a = mp.origin + (np.array(lo) + 0.25) * res
        b = mp.origin + (np.array(hi) + 0.75) * res
        if lo == (5, 3, 0):
            import torch
            ctx.update_sdf_map_window_device(a, b, torch.tensor(pts, device="cuda:0"))
            torch.cuda.synchronize()
        else:
            ctx.update_sdf_map_window(a, b, pts)
        field = _window_ref(field, occ, lo, hi, res, max_depth)
        d = ctx.get_sdf()
        assert np.array_equal(d, field), (lo, hi, int((d != field).sum()))
    ctx.close()


def test_mode_mismatch_refuses_a_window_and_leaves_the_field(gtop):
    grid, res = (30, 30, 20), 0.2
    occ = np.zeros(grid, np.uint8)
    occ[5:25, 5:25, 2:18] = 1
    ctx, mp = _ctx(gtop, grid, res, True, 0.0)
    d0 = _build(ctx, mp, occ)
    a, b = mp.origin + 1.0, mp.origin + 4.0
    pts = np.array([[0.0, 0.0, 1.0]])
    for mode, depth in ((False, 0.0), (True, 0.7)):
        ctx.set_field_sign(mode, depth)
        with pytest.raises(gtop.GtopError) as ei:
            ctx.update_sdf_map_window(a, b, pts)
        assert ei.value.code == ERR_STATE and "whole-map update needed after changing the field sign" in str(ei.value)
        assert np.array_equal(ctx.get_sdf(), d0)
        assert ctx.field_sign() == (True, 0.0)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(gtop.GtopError) as ei:
            ctx.set_field_sign(True, bad)
        assert ei.value.code == ERR_INVALID
    lib = gtop.load_library()
    assert lib.gtop_set_field_sign(ctx._h, 2, 0.0) == ERR_INVALID
    # a whole-map build takes the new setting, and windows follow it again
    ctx.set_field_sign(False)
    assert np.array_equal(_build(ctx, mp, occ), unsigned_reference(occ, res))
    assert ctx.field_sign() == (False, 0.0)
    ctx.update_sdf_map_window(a, b, pts)
    # an upload names the field with the mode in force
    ctx.set_field_sign(True, 2.0)
    ctx.set_sdf(d0, grid, mp.origin, res, map_size=mp.map_size)
    assert ctx.field_sign() == (True, 2.0)
    ctx.close()


def test_signed_and_unsigned_fields_differ_exactly_at_enclosed_voxels(gtop):
    mp0 = problem.make_map((80, 72, 48), density=0.25, seed=21, box_vox=(4, 20))
    occ, res = mp0.occupancy, mp0.resolution
    ctx, mp = _ctx(gtop, occ.shape, res, False)
    unsigned = _build(ctx, mp, occ)
    assert np.array_equal(unsigned, unsigned_reference(occ, res))
    ctx.set_field_sign(True, 0.0)
    signed = _build(ctx, mp, occ)
    assert ctx.field_sign() == (True, 0.0)
    pad = np.pad(occ == 1, 1, constant_values=True)                            # outside the box is not free
    enclosed = (occ == 1)
    for ax in range(3):
        for s in (-1, 1):
            enclosed &= np.roll(pad, s, axis=ax)[1:-1, 1:-1, 1:-1]
    assert enclosed.sum() > 1000
    assert np.array_equal(signed[~enclosed], unsigned[~enclosed])
    assert np.all(signed[enclosed] < 0.0) and np.all(unsigned[enclosed] == 0.0)
    ctx.set_field_sign(False)
    assert np.array_equal(_build(ctx, mp, occ), unsigned)                      # off again: today's field, bit for bit
    ctx.close()


def _pillar_map(side):
    grid, res, origin = (60, 60, 30), 0.2, np.array([-6.0, -6.0, 0.0])
    c = (np.arange(60) + 0.5) * res - 6.0
    inside = np.abs(c) < side / 2
    occ = np.zeros(grid, np.uint8)
    occ[np.ix_(inside, inside, np.ones(30, bool))] = 1
    return problem.MapSpec(grid, res, origin, occ)


def _signed_scene(gtop, oracle_mod, max_depth, seed=5):
    mp = problem.make_map((64, 56, 40), density=0.12, seed=seed, box_vox=(5, 16))
    ctx = gtop.GtopContext(device=0)
    ctx.set_field_sign(True, max_depth)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    d = ctx.get_sdf()
    assert np.array_equal(d, signed_reference(mp.occupancy, mp.resolution, max_depth))
    assert (d < -mp.resolution).sum() > 100
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.dist[:] = d.reshape(-1)
    return mp, ctx, sdf


def test_fp64_evaluations_on_a_signed_field_match_the_oracle(gtop, oracle_mod):
    mp, ctx, sdf = _signed_scene(gtop, oracle_mod, 0.0)
    for m in (4, 6, 9):
        b = problem.make_trajectories(96, m, mp, seed=40 + m, step_len=(0.8, 1.6))
        ctx.set_problem(b.T, b.Df)
        c_ref, g_ref, _ = oracle_mod.eval_batch(b.T, b.Df, b.x, sdf, oracle_mod.make_params())
        for spl in (0, 3, 6, 10, 30):
            if (spl == 3 and m > 12) or (spl == 10 and m > 10):
                continue
            try:
                ctx.set_launch_geometry(0, spl)
                c, g = ctx.eval_batch(b.x)
            finally:
                ctx.set_launch_geometry(0, 0)
            rc, rg = scenes.rel_err(c, g, c_ref, g_ref)
            assert rc <= 1e-12 and rg <= 1e-12, (m, spl, rc, rg)
    ctx.close()


def test_fp32_evaluations_and_optimizer_on_a_signed_field(gtop, oracle_mod):
    """max_depth inside the header's bound for fp32 (80 r - d0 = 39.2 with the launch file's r, d0): finite, and
    within the fp32 tolerances against fp64."""
    import torch
    mp, ctx, sdf = _signed_scene(gtop, oracle_mod, 2.0)
    b = problem.make_trajectories(256, 6, mp, seed=61)
    dev = torch.device("cuda:0")
    c32, g32 = ctx.eval_device(*[torch.tensor(v, dtype=torch.float32, device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T)])
    torch.cuda.synchronize()
    c32, g32 = c32.double().cpu().numpy(), g32.double().cpu().numpy()
    c_ref, g_ref, _ = oracle_mod.eval_batch(b.T, b.Df, b.x, sdf, oracle_mod.make_params())
    assert np.isfinite(c32).all() and np.isfinite(g32).all()
    assert np.max(np.abs(c32 - c_ref) / np.abs(c_ref)) <= 2e-4
    rg_rows = np.max(np.abs(g32 - g_ref), axis=1) / np.maximum(np.max(np.abs(g_ref), axis=1), 1e-2)
    assert np.max(rg_rows) <= 2e-4
    # the fp32 records are (float) of the fp64 field: an fp32 upload of that field evaluates bit for bit the same
    up = gtop.GtopContext(device=0)
    f32 = torch.tensor(ctx.get_sdf().astype(np.float32).reshape(-1), device=dev)
    up.set_sdf_device(f32, mp.grid, mp.origin, mp.resolution, map_size=mp.map_size)
    cu, gu = up.eval_device(*[torch.tensor(v, dtype=torch.float32, device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T)])
    torch.cuda.synchronize()
    assert np.array_equal(cu.double().cpu().numpy(), c32) and np.array_equal(gu.double().cpu().numpy(), g32)
    up.close()
    # the optimizer's fp32 evaluations
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    ctx.set_problem(b.T, b.Df)
    x64, cc64, n64, code64 = ctx.optimize_batch_ex(b.x, lb, ub, 25)
    try:
        ctx.set_optimizer_precision("f32")
        x32, cc32, n32, code32 = ctx.optimize_batch_ex(b.x, lb, ub, 25)
    finally:
        ctx.set_optimizer_precision("f64")
    assert np.isfinite(cc32).all() and np.isfinite(x32).all()
    assert np.array_equal(n32, n64) and np.array_equal(code32, code64)
    c_at, _, _ = oracle_mod.eval_batch(b.T, b.Df, x32, sdf, oracle_mod.make_params())
    assert np.max(np.abs(cc32 - c_at) / np.abs(c_at)) <= 2e-4
    assert 0.8 <= np.median(cc32 / cc64) <= 1.25
    ctx.close()


def test_edt_queries_on_a_signed_field_match_the_oracle(gtop, oracle_mod):
    mp, ctx, sdf = _signed_scene(gtop, oracle_mod, 0.0, seed=8)
    rng = np.random.default_rng(3)
    for nbox in (0, 1, 9, 40):
        p0 = rng.uniform(mp.origin, mp.origin + mp.map_size, size=(nbox, 3))
        vel = rng.uniform(-1.0, 1.0, size=(nbox, 3))
        scale = rng.uniform(0.3, 1.5, size=(nbox, 3))
        pos = rng.uniform(mp.origin - 0.3, mp.origin + mp.map_size + 0.3, size=(500, 3))
        pos[:200] = mp.obstacle_points()[rng.choice(len(mp.obstacle_points()), 200)] + rng.uniform(-0.1, 0.1, (200, 3))
        time = rng.uniform(0.0, 3.0, size=500)
        time[::3] = -1.0
        ctx.set_moving_boxes(p0, vel, scale)
        d, g = ctx.edt_query(pos, time)
        d_ref, g_ref = sdf.edt_query(pos, time, p0, vel, scale)
        assert (d_ref < 0).sum() > 20
        assert np.allclose(d, d_ref, rtol=1e-12, atol=1e-12) and np.allclose(g, g_ref, rtol=1e-10, atol=1e-10)
        dc = ctx.edt_coarse_query(pos, time)
        assert np.allclose(dc, sdf.edt_coarse(pos, time, p0, vel, scale), rtol=1e-13, atol=1e-13)
    ctx.close()


@pytest.mark.parametrize("side,evals", [(3.2, 200), (4.8, 200), (2.0, 50)])
def test_signed_field_pushes_trajectories_out_of_a_pillar(gtop, oracle_mod, side, evals):
    """256 straight lines through a full-height square pillar (z = 2 m, along x, y offsets 0 .. 0.9 half-widths),
    optimised on the unsigned and on the signed field: on the signed one every row off the pillar's axis ends outside
    (the 4.8 m pillar: at most grazing its surface); on the unsigned one most rows that started inside keep samples
    inside (zero gradient deeper than a voxel)."""
    mp = _pillar_map(side)
    B, half = 256, side / 2
    ys = np.linspace(0.0, 0.9 * half, B)
    xs = np.linspace(-4.0, 4.0, 5)
    wp = np.zeros((B, 5, 3))
    wp[:, :, 0] = xs
    wp[:, :, 1] = ys[:, None]
    wp[:, :, 2] = 2.0
    lb, ub = gtop.GtopContext.default_bounds(wp, 3.0, 8.0, 10.0)
    probe = gtop.GtopContext(device=0)                                         # the UNSIGNED field's lookups
    probe.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    probe.update_sdf_map(mp.obstacle_points())
    probe.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    depth = gtop.GtopContext(device=0)                                         # the SIGNED field's lookups
    depth.set_field_sign(True)
    depth.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    depth.update_sdf_map(mp.obstacle_points())
    depth.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    deepest = {}

    def inside(ctx, x, key=None):
        stats, samples = ctx.trajectory_samples(x, dt_sample=0.01)
        n = stats[:, 8].astype(int)
        assert n.max() <= samples.shape[1]
        keep = np.arange(samples.shape[1])[None, :] < n[:, None]
        d, _ = probe.edt_query(samples[keep], -1.0)
        out = np.zeros(B, dtype=int)
        np.add.at(out, np.nonzero(keep)[0], d <= 0.0)
        if key is not None:
            ds, _ = depth.edt_query(samples[keep], -1.0)
            deepest[key] = np.full(B, np.inf)
            np.minimum.at(deepest[key], np.nonzero(keep)[0], ds)
        return out

    res = {}
    for signed in (False, True):
        ctx = gtop.GtopContext(device=0)
        ctx.set_field_sign(signed)
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        ctx.update_sdf_map(mp.obstacle_points())
        x0 = ctx.set_paths(wp, 1.8, 0.3)
        before = inside(ctx, x0)
        x, cost, nev, code = ctx.optimize_batch_ex(x0, lb, ub, evals)
        assert np.isfinite(cost).all()
        res[signed] = (before, inside(ctx, x, signed))
        ctx.close()
    probe.close()
    depth.close()
    before = res[False][0]
    assert np.array_equal(before, res[True][0]) and (before > 0).mean() > 0.75
    # Rows closer to the pillar's axis than half a voxel sit on a saddle of the discrete field: the pillar is an even
    # number of voxels wide, the voxel centres either side of the axis hold equal values, and the trilinear lookup
    # has an exactly zero y-gradient there in either field.  Every other row must leave the pillar on the signed field.
    off_axis = ys >= mp.resolution / 2
    stuck = res[False][1][(before > 0) & off_axis] > 0
    print(f"pillar {side} m: samples inside before {int(before.sum())}, after unsigned {int(res[False][1].sum())} "
          f"({stuck.mean():.2f} of the crossing rows), signed {int(res[True][1].sum())} in rows "
          f"{np.flatnonzero(res[True][1] * off_axis).tolist()}; deepest signed value of a signed row "
          f"{deepest[True][off_axis].min():.3f}, of an unsigned row {deepest[False][off_axis].min():.3f}")
    assert stuck.mean() > 0.5, stuck.mean()
    assert res[True][1][off_axis].sum() * 10 < res[False][1][off_axis].sum()
    if side != 4.8:
        assert np.all(res[True][1][off_axis] == 0), np.flatnonzero(res[True][1] * off_axis)
    else:
        # The widest pillar: the loop settles (100 and 200 evaluations end alike) with some rows grazing its surface —
        # none deeper than a voxel (measured: 0.06 m); the unsigned field leaves rows metres inside (2.2 m).
        assert deepest[True][off_axis].min() >= -mp.resolution
        assert deepest[False][off_axis].min() < -mp.resolution
