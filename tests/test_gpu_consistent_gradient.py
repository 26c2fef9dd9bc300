"""The consistent gradient mode on the device (include/gtop.h, gtop_set_gradient_mode) against the numpy restatement
with a mode argument (tests/consistent_twin.py), through the public Python wrapper: every body the launch rule serves
(the lists of tests/test_gpu_kino.py, its criterion and tolerances, plus three lanes / one lane per segment), both
precisions, the moving-obstacle lookup, a signed field, the optimizer's launch forms, and the other roads a context
setting has to reach.  In every body exercised the COST is bit-identical between the two modes."""
import ctypes
import threading

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from oracle import np_twin
from tests import consistent_twin as ct
from tests import moving_twin, scenes
from tests.test_consistent_gradient import analytic_case
from tests.test_gpu_kino import TOL32, TOL64, _kino
from tests.test_optimizer import mma_serial

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
DYN = dict(enable_dyn=1, alpha_v=2.0, r_v=4.0, alpha_a=1.5, r_a=15.0, step=2)   # tests/test_gpu_kino.py's block


@pytest.fixture(scope="module")
def scene(gtop, oracle_mod):
    mp = problem.make_map((60, 50, 30), density=0.03, seed=11)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    yield mp, ctx, sdf
    ctx.close()


def _params(oracle_mod, **kw):
    return dict(oracle_mod.OPTI_NODE_PARAMS, **kw)


def _subsample(B):
    return np.arange(B) if B <= 64 else np.r_[0:40, B - 40:B]   # tests/test_gpu_kino.py::_check


def _run(ctx, b, waves, spl, dtype, mode, **params):
    import torch
    td = torch.float64 if dtype == "f64" else torch.float32
    dev = torch.device("cuda:0")
    x = torch.tensor(b.x, dtype=td, device=dev)
    Df = torch.tensor(b.Df.reshape(-1, 18), dtype=td, device=dev)
    T = torch.tensor(b.T, dtype=td, device=dev)
    try:
        ctx.set_params(**params)
        ctx.set_launch_geometry(waves, spl)
        ctx.set_gradient_mode(bool(mode))
        assert ctx.gradient_mode == mode
        c, g = ctx.eval_device(x, Df, T)
        torch.cuda.synchronize()
    finally:
        ctx.set_gradient_mode(False)
        ctx.set_launch_geometry(0, 0)
        ctx.set_params()
    return c.double().cpu().numpy(), g.double().cpu().numpy()


def _both_modes(ctx, b, waves, spl, dtype, **params):
    """The body in both modes: the cost bit-identical, the gradient not the same function."""
    c0, g0 = _run(ctx, b, waves, spl, dtype, 0, **params)
    c1, g1 = _run(ctx, b, waves, spl, dtype, 1, **params)
    assert np.array_equal(c0, c1), "the cost differs between the gradient modes"
    assert np.isfinite(c1).all() and np.isfinite(g1).all()
    assert not np.array_equal(g0, g1)
    return c1, g1


_twin_cache = {}


def _twin_rows(oracle_mod, sdf, b, key, **params):
    """Mode 1 of the twin on the subsample of the batch (the same rows serve both precisions)."""
    if key not in _twin_cache:
        idx = _subsample(b.x.shape[0])
        c, g = ct.eval_batch(b.T[idx], b.Df[idx], b.x[idx], sdf, _params(oracle_mod, **params), ct.CONSISTENT)
        _twin_cache[key] = (idx, c, g)
    return _twin_cache[key]


def _check(tag, c, g, idx, c_ref, g_ref, tol):
    rc, rg = scenes.rel_err(c[idx], g[idx], c_ref, g_ref)
    print(f"PARITY {tag} cost {rc:.3e} grad {rg:.3e}")
    assert rc <= tol and rg <= tol, (rc, rg)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("spl,m", [(3, 2), (3, 3), (3, 5), (3, 6), (6, 5), (6, 6), (6, 7), (6, 9), (6, 11), (6, 12)])
@pytest.mark.parametrize("B", [23, 3101])
def test_parity_every_wave_instantiation(scene, oracle_mod, dtype, spl, m, B):
    """tests/test_gpu_kino.py::test_kino_rows_every_wave_instantiation's bodies in mode 1 against the twin."""
    mp, ctx, sdf = scene
    b = _kino(B, m, mp, 1600 + 13 * m + spl)
    c, g = _both_modes(ctx, b, 1, spl, dtype)
    idx, c_ref, g_ref = _twin_rows(oracle_mod, sdf, b, ("plain", spl, m, B))
    _check(f"plain {dtype} spl={spl} m={m} B={B}", c, g, idx, c_ref, g_ref, TOL64 if dtype == "f64" else TOL32)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("waves,spl,m,B", [(0, 6, 3, 23), (0, 6, 4, 200), (1, 6, 13, 23), (0, 0, 13, 300), (0, 0, 20, 5000),
                                           (0, 0, 30, 64), (0, 0, 6, 1), (0, 0, 9, 100), (0, 0, 12, 4100),
                                           # three lanes and one lane per segment (samples_per_lane 10, 30)
                                           (1, 10, 4, 300), (1, 10, 7, 90), (1, 30, 6, 700), (1, 30, 12, 300)])
def test_parity_other_geometries(scene, oracle_mod, dtype, waves, spl, m, B):
    """tests/test_gpu_kino.py::test_kino_rows_other_geometries's list — two short trajectories per wavefront, past 12
    segments, the auto rule's switch points — and the two geometries that list has no row for."""
    mp, ctx, sdf = scene
    b = _kino(B, m, mp, 1700 + 7 * m + spl)
    c, g = _both_modes(ctx, b, waves, spl, dtype)
    idx, c_ref, g_ref = _twin_rows(oracle_mod, sdf, b, ("other", waves, spl, m, B))
    _check(f"other {dtype} waves={waves} spl={spl} m={m} B={B}", c, g, idx, c_ref, g_ref, TOL64 if dtype == "f64" else TOL32)


@pytest.mark.parametrize("spl,m,B", [(0, 6, 37), (3, 6, 600), (3, 4, 3200), (6, 6, 600), (6, 12, 200), (0, 13, 64), (0, 27, 40),
                                     (0, 6, 9000)])
def test_parity_dyn_bodies(scene, oracle_mod, spl, m, B):
    """tests/test_gpu_kino.py::test_kino_rows_dyn_feasibility's bodies: sgn(v), sgn(a) and the sum of the axes'
    penalties in every DYN body, fp32 on that test's rows."""
    mp, ctx, sdf = scene
    b = _kino(B, m, mp, 1800 + m + spl)
    c, g = _both_modes(ctx, b, 0, spl, "f64", **DYN)
    idx, c_ref, g_ref = _twin_rows(oracle_mod, sdf, b, ("dyn", spl, m, B), **DYN)
    _check(f"dyn f64 spl={spl} m={m} B={B}", c, g, idx, c_ref, g_ref, TOL64)
    if m <= 12 and B <= 600:
        keep = np.flatnonzero(b.T.min(axis=1) >= 0.25)
        bb = problem.permute(b, keep)
        c, g = _both_modes(ctx, bb, 0, spl, "f32", **DYN)
        idx, c_ref, g_ref = _twin_rows(oracle_mod, sdf, bb, ("dyn32", spl, m, B), **DYN)
        _check(f"dyn f32 spl={spl} m={m} B={len(keep)}", c, g, idx, c_ref, g_ref, TOL32)


STEEP = dict(DYN, r_v=0.5, r_a=1.0)   # tests/test_consistent_gradient.py's scale lengths: gv, ga weigh as much as the rest


@pytest.mark.parametrize("spl,m,B", [(0, 6, 37), (3, 5, 70), (6, 9, 70), (0, 13, 40)])
def test_parity_dyn_bodies_with_a_steep_block(scene, oracle_mod, spl, m, B):
    """The DYN bodies with scale lengths of 0.5 m/s and 1 m/s^2: the penalties' own derivatives (gv sgn(v), ga sgn(a))
    are then a large part of the gradient, so a wrong sign factor or a wrong sum shows at the parity tolerance."""
    mp, ctx, sdf = scene
    b = _kino(B, m, mp, 2700 + m + spl)
    c, g = _both_modes(ctx, b, 0, spl, "f64", **STEEP)
    idx, c_ref, g_ref = _twin_rows(oracle_mod, sdf, b, ("steep", spl, m, B), **STEEP)
    _check(f"steep dyn f64 spl={spl} m={m} B={B}", c, g, idx, c_ref, g_ref, TOL64)


def test_without_a_collision_term_the_modes_are_one_function(scene):
    """|wc| < 1e-4 skips the sample loop (:346): there is nothing the mode could change."""
    mp, ctx, _ = scene
    b = _kino(37, 6, mp, 1900)
    c0, g0 = _run(ctx, b, 0, 0, "f64", 0, wc=0.0)
    c1, g1 = _run(ctx, b, 0, 0, "f64", 1, wc=0.0)
    assert np.array_equal(c0, c1) and np.array_equal(g0, g1)


def _aimed_boxes(b, t0, rng, nbox):
    """tests/test_gpu_moving_cost.py: box k is where a random waypoint of a random trajectory is when it gets there."""
    j = rng.integers(0, len(b.x), nbox)
    w = rng.integers(0, b.m + 1, nbox)
    vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * np.array([1.0, 1.0, 0.2])
    when = np.array([t0[jj] + b.T[jj][:ww].sum() for jj, ww in zip(j, w)])
    return b.waypoints[j, w] - vel * when[:, None], vel, rng.uniform(1.0, 2.0, (nbox, 3))


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("spl,m", [(0, 4), (6, 6), (0, 9), (0, 13)])
def test_parity_with_the_moving_cost_on(scene, oracle_mod, spl, m, dyn):
    """dist and grad from the time-aware lookup (tests/moving_twin.TimedLookup plugged into the twin), with boxes that
    lower corner values on at least half of the rows."""
    mp, ctx, sdf = scene
    B = 32
    b = problem.make_trajectories(B, m, mp, seed=300 + m, step_len=(0.5, 1.2) if m > 6 else (1.0, 2.0))
    rng = np.random.default_rng(310 + m)
    t0 = rng.uniform(0.0, 5.0, B)
    boxes = _aimed_boxes(b, t0, rng, 8)
    extra = DYN if dyn else {}
    p = _params(oracle_mod, **extra)
    c_ref, g_ref, lowered = np.empty(B), np.empty_like(b.x), 0
    for i in range(B):
        look = moving_twin.TimedLookup(sdf, moving_twin.sample_times(b.T[i], t0[i]), *boxes)
        c_ref[i], g_ref[i], _ = ct.cost_grad(b.T[i], b.Df[i], b.x[i], look, p, ct.CONSISTENT)
        lowered += bool(np.any(look.lowered))
    assert lowered >= B // 2, lowered
    try:
        ctx.set_params(**extra)
        ctx.set_launch_geometry(0, spl)
        ctx.set_moving_boxes(*boxes)
        ctx.set_moving_cost(True)
        ctx.set_start_times(t0)
        ctx.set_problem(b.T, b.Df)
        c0, g0 = ctx.eval_batch(b.x)
        ctx.set_gradient_mode(True)
        c1, g1 = ctx.eval_batch(b.x)
    finally:
        ctx.set_gradient_mode(False)
        ctx.set_moving_cost(False)
        ctx.set_start_times(None)
        ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
        ctx.set_launch_geometry(0, 0)
        ctx.set_params()
    assert np.array_equal(c0, c1) and not np.array_equal(g0, g1)
    _check(f"moving f64 spl={spl} m={m} dyn={int(dyn)}", c1, g1, np.arange(B), c_ref, g_ref, TOL64)


class _Recording:
    def __init__(self, sdf):
        self.sdf, self.min_dist = sdf, np.inf

    def query(self, pos):
        d, g = self.sdf.query(pos)
        self.min_dist = min(self.min_dist, d)
        return d, g


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_parity_on_a_signed_field(gtop, oracle_mod, dtype):
    """A signed field is taken as it is: rows that cross obstacles read negative distances in both the twin and the
    kernels (max_depth 1 m keeps the fp32 penalty far from its overflow)."""
    mp = problem.make_map((60, 50, 30), density=0.08, seed=12)
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.set_field_sign(True, 1.0)
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        ctx.update_sdf_map(mp.obstacle_points())
        assert ctx.field_sign() == (True, 1.0)
        field = ctx.get_sdf()
        assert field.min() < 0.0
        sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
        sdf.dist[:] = field.reshape(-1)
        b = _kino(48, 6, mp, 2300)
        rec = _Recording(sdf)
        c_ref, g_ref = ct.eval_batch(b.T, b.Df, b.x, rec, _params(oracle_mod), ct.CONSISTENT)
        assert rec.min_dist < -0.1, rec.min_dist          # samples inside obstacles
        for spl in (3, 6):
            c, g = _both_modes(ctx, b, 1, spl, dtype)
            _check(f"signed {dtype} spl={spl}", c, g, np.arange(48), c_ref, g_ref, TOL64 if dtype == "f64" else TOL32)
    finally:
        ctx.close()


def test_hand_derived_known_answer_on_the_device(gtop):
    """tests/golden/CONSISTENT_ANALYTIC.md, case D, through the fp64 DYN bodies at ten and five lanes per segment."""
    z, p = analytic_case()
    grid, res = z["grid"], float(z["resolution"])
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.set_sdf(np.full(tuple(grid), 1.3), grid, z["origin"], res)
        ctx.set_params(**p)
        ctx.set_problem(z["D_T"][None], z["D_Df"][None])
        ctx.set_gradient_mode(True)
        for spl in (3, 6):
            ctx.set_launch_geometry(0, spl)
            c, g = ctx.eval_batch(z["D_x"][None])
            err = scenes.rel_err(c, g, float(z["D_cost"]), z["D_grad"])
            print(f"PARITY analytic f64 spl={spl} cost {err[0]:.3e} grad {err[1]:.3e}")
            assert err <= (1e-7, 1e-7)
            # sgn(+-0) = 0 on the kernel: the two idle axes get nothing but the callback's +1e-5, exactly
            assert np.all(g[0, g.shape[1] // 3:] == ct.GRAD_EPS), g[0, g.shape[1] // 3:]
        ctx.set_gradient_mode(False)
        _, g0 = ctx.eval_batch(z["D_x"][None])
        assert scenes.rel_err(c, g0, float(z["D_cost"]), z["D_grad"])[1] > 1e-2
    finally:
        ctx.close()


def test_switching_back_and_the_getter(scene, gtop):
    """Mode 0 after mode 1 is the gradient of a context that never left mode 0, bit for bit; the getter round-trips;
    another value is refused and changes nothing."""
    mp, ctx, _ = scene
    lib = gtop.load_library()
    b = _kino(300, 6, mp, 2400)
    fresh = gtop.GtopContext(device=0)
    try:
        fresh.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        fresh.update_sdf_map(mp.obstacle_points())
        assert fresh.gradient_mode == gtop.GtopContext.GRADIENT_REFERENCE      # the default
        for prm in ({}, DYN):
            fresh.set_params(**prm)
            fresh.set_problem(b.T, b.Df)
            c_ref, g_ref = fresh.eval_batch(b.x)
            ctx.set_params(**prm)
            ctx.set_problem(b.T, b.Df)
            ctx.set_gradient_mode(True)
            assert ctx.gradient_mode == gtop.GtopContext.GRADIENT_CONSISTENT
            c1, g1 = ctx.eval_batch(b.x)
            for bad in (2, -1, 7):
                assert lib.gtop_set_gradient_mode(ctx._h, bad) == ERR_INVALID
                assert ctx.gradient_mode == 1
            mode = ctypes.c_int(-5)
            assert lib.gtop_get_gradient_mode(ctx._h, None) == ERR_INVALID
            assert lib.gtop_get_gradient_mode(ctx._h, ctypes.byref(mode)) == 0 and mode.value == 1
            ctx.set_gradient_mode(False)
            assert ctx.gradient_mode == 0
            c0, g0 = ctx.eval_batch(b.x)
            assert np.array_equal(c0, c_ref) and np.array_equal(g0, g_ref)
            assert np.array_equal(c1, c_ref) and not np.array_equal(g1, g_ref)
    finally:
        ctx.set_gradient_mode(False)
        ctx.set_params()
        fresh.close()


@pytest.mark.parametrize("m,evals", [(6, 25), (9, 20), (12, 15), (13, 12)])
def test_optimizer_launch_forms(scene, oracle_mod, gtop, m, evals):
    """As tests/test_gpu_kino.py::test_kino_rows_optimizer_launch_forms, in mode 1: the three fusion modes bit-identical
    at one pinned body; each row follows the serial CCSA-MMA twin driven by the restatement in mode 1; each row's cost
    ends below its start; fp32 evaluations run to completion."""
    mp, ctx, sdf = scene
    B = 12
    b = _kino(B, m, mp, 2000 + m)
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    ctx.set_params()
    ctx.set_problem(b.T, b.Df)
    res = {}
    try:
        ctx.set_gradient_mode(True)
        c_start, _ = ctx.eval_batch(b.x)
        ctx.set_launch_geometry(0, 3 if m <= 6 else 6)
        for mode in (2, 1, 0):
            ctx.set_optimizer_fusion(mode)
            res[mode] = ctx.optimize_batch(b.x, lb, ub, evals)
        ctx.set_optimizer_fusion(2)
        ctx.set_launch_geometry(0, 0)
        xs, costs = ctx.optimize_batch(b.x, lb, ub, evals)              # the auto rule's own choice
        ctx.set_optimizer_precision("f32")
        xs32, costs32, nev32, _ = ctx.optimize_batch_ex(b.x, lb, ub, evals)
        ctx.set_optimizer_precision("f64")
        ctx.set_gradient_mode(False)
        xs_ref_mode, costs_ref_mode = ctx.optimize_batch(b.x, lb, ub, evals)
    finally:
        ctx.set_gradient_mode(False)
        ctx.set_optimizer_precision("f64")
        ctx.set_optimizer_fusion(2)
        ctx.set_launch_geometry(0, 0)
    for mode in (1, 0):
        assert np.array_equal(res[mode][0], res[2][0]) and np.array_equal(res[mode][1], res[2][1])
    assert not np.array_equal(xs, xs_ref_mode)                          # the mode reached the loop
    assert np.isfinite(xs32).all() and np.isfinite(costs32).all() and np.all((nev32 >= 1) & (nev32 <= evals))
    p = _params(oracle_mod)
    for i in range(B):
        gen = np_twin.generator(b.T[i])

        def f(x, i=i, gen=gen):
            return ct.cost_grad(b.T[i], b.Df[i], x, sdf, p, ct.CONSISTENT, gen=gen)[:2]
        x_ref, f_ref, _ = mma_serial(f, b.x[i], lb[i], ub[i], evals)
        for xo, co in ((xs, costs), res[2]):
            assert abs(co[i] - f_ref) <= 1e-6 * abs(f_ref), (i, co[i], f_ref)
            assert np.max(np.abs(xo[i] - x_ref)) <= 1e-6 * max(1.0, np.max(np.abs(x_ref)))
        assert costs[i] < c_start[i]
    print(f"optimizer m={m}: median final cost, mode 1 {np.median(costs):.1f} mode 0 {np.median(costs_ref_mode):.1f} "
          f"(start {np.median(c_start):.1f})")


@pytest.mark.parametrize("case,m,spl", [("dyn", 6, 0), ("dyn", 4, 6), ("dyn", 9, 6), ("moving", 6, 0), ("moving+dyn", 6, 0)])
def test_optimizer_with_the_block_and_with_the_moving_cost(scene, oracle_mod, gtop, case, m, spl):
    """The optimizer's other mode-1 bodies — enable_dyn on (also where two short trajectories share a wavefront in the
    evaluations, samples_per_lane 6 at m = 4), the moving-obstacle cost on, and both — against the serial CCSA-MMA twin
    driven by the restatement in mode 1 (tests/moving_twin.TimedLookup plugged in where the moving cost is on), to the
    1e-6 of test_optimizer_launch_forms; the iterates differ from mode 0's and each row's cost ends below its start."""
    mp, ctx, sdf = scene
    dyn, moving = "dyn" in case, "moving" in case
    B, evals = (4, 10) if moving else (8, 12)                           # (the timed lookup of the twin is the slow part)
    b = problem.make_trajectories(B, m, mp, seed=2600 + m) if moving else _kino(B, m, mp, 2600 + m)
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    rng = np.random.default_rng(2610 + m)
    t0 = rng.uniform(0.0, 5.0, B)
    boxes = _aimed_boxes(b, t0, rng, 8)
    extra = DYN if dyn else {}
    p = _params(oracle_mod, **extra)
    try:
        ctx.set_params(**extra)
        ctx.set_launch_geometry(0, spl)
        if moving:
            ctx.set_moving_boxes(*boxes)
            ctx.set_moving_cost(True)
            ctx.set_start_times(t0)
        ctx.set_problem(b.T, b.Df)
        xs0, costs0 = ctx.optimize_batch(b.x, lb, ub, evals)
        ctx.set_gradient_mode(True)
        c_start, _ = ctx.eval_batch(b.x)
        xs, costs = ctx.optimize_batch(b.x, lb, ub, evals)
    finally:
        ctx.set_gradient_mode(False)
        ctx.set_moving_cost(False)
        ctx.set_start_times(None)
        ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
        ctx.set_launch_geometry(0, 0)
        ctx.set_params()
    assert not np.array_equal(xs, xs0)                                  # the mode reached these bodies
    worst_c = worst_x = 0.0
    for i in range(B):
        gen = np_twin.generator(b.T[i])
        taus = moving_twin.sample_times(b.T[i], t0[i])

        def f(x, i=i, gen=gen, taus=taus):
            look = moving_twin.TimedLookup(sdf, taus, *boxes) if moving else sdf
            return ct.cost_grad(b.T[i], b.Df[i], x, look, p, ct.CONSISTENT, gen=gen)[:2]
        x_ref, f_ref, _ = mma_serial(f, b.x[i], lb[i], ub[i], evals)
        worst_c = max(worst_c, abs(costs[i] - f_ref) / abs(f_ref))
        worst_x = max(worst_x, np.max(np.abs(xs[i] - x_ref)) / max(1.0, np.max(np.abs(x_ref))))
    print(f"PARITY optimizer {case} m={m} spl={spl}: cost {worst_c:.3e} point {worst_x:.3e}; median final cost, mode 1 "
          f"{np.median(costs):.1f} mode 0 {np.median(costs0):.1f} (start {np.median(c_start):.1f})")
    assert worst_c <= 1e-6 and worst_x <= 1e-6, (worst_c, worst_x)
    assert np.all(costs < c_start)


def test_rendezvous_and_nlopt_roads_return_the_batch_rows(scene, gtop):
    """gtop_cost_nlopt_shared and gtop_cost_nlopt in mode 1: the rows of the batch road, bit for bit."""
    mp, ctx, _ = scene
    n_callers, m = 8, 6
    b = _kino(n_callers, m, mp, 2100)
    ctx.set_params()
    ctx.set_problem(b.T, b.Df)
    c_mode0, g_mode0 = ctx.eval_batch(b.x)
    got, errors = {}, []
    try:
        ctx.set_gradient_mode(True)
        c_ref, g_ref = ctx.eval_batch(b.x)
        assert np.array_equal(c_ref, c_mode0) and not np.array_equal(g_ref, g_mode0)
        rdv = gtop.Rendezvous(ctx, n_callers, m)

        def worker(i):
            try:
                got[i] = rdv.cost(i, b.x[i])
            except Exception as e:      # noqa: BLE001 — reported below; the slot must leave either way
                errors.append(e)
            finally:
                rdv.leave(i)

        th = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(n_callers)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
            assert not t.is_alive()
        rdv.close()
        assert not errors, errors
        for i in range(n_callers):
            assert got[i][0] == c_ref[i] and np.array_equal(got[i][1], g_ref[i])
        c1, g1 = ctx.cost_nlopt(b.x[0])
        assert c1 == c_ref[0] and np.array_equal(g1, g_ref[0])
    finally:
        ctx.set_gradient_mode(False)


def test_group_forwards_the_mode(scene, gtop):
    """gtop_group_set_gradient_mode on a group that lists one device twice: the sharded evaluation (host buffers and
    resident) and the sharded optimizer are a single context's in mode 1."""
    mp, ctx, _ = scene
    B, m = 300, 6
    b = problem.make_trajectories(B, m, mp, seed=60)
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    ctx.set_params()
    ctx.set_problem(b.T, b.Df)
    g = gtop.GtopGroup([0, 0])
    try:
        g.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        g.update_sdf_map(mp.obstacle_points())
        g.set_problem(b.T, b.Df)
        c_mode0, g_mode0 = g.eval_batch(b.x)
        ctx.set_gradient_mode(True)
        c_ref, g_ref = ctx.eval_batch(b.x)
        ref = ctx.optimize_batch_ex(b.x, lb, ub, 15, ftol_rel=1e-3)
        g.set_gradient_mode(True)
        c, gr = g.eval_batch(b.x)
        assert np.array_equal(c, c_ref) and np.array_equal(gr, g_ref) and not np.array_equal(gr, g_mode0)
        for ci, gi in g.eval_resident(gather=2):
            assert np.array_equal(ci, c_ref) and np.array_equal(gi, g_ref)
        got = g.optimize_batch_ex(b.x, lb, ub, 15, ftol_rel=1e-3)
        for a, r in zip(got, ref):
            assert np.array_equal(a, r)
        g.set_gradient_mode(False)
        c, gr = g.eval_batch(b.x)
        assert np.array_equal(c, c_mode0) and np.array_equal(gr, g_mode0)
    finally:
        ctx.set_gradient_mode(False)
        g.close()


def test_a_captured_evaluation_keeps_the_mode_it_was_captured_with(scene):
    """The setting is read when the call is made: a torch.cuda.graph capture of gtop_eval_device in mode 1 replays in
    mode 1 after the context has gone back to mode 0, and the other way round."""
    import torch
    mp, ctx, _ = scene
    b = _kino(200, 6, mp, 2500)
    dev = torch.device("cuda:0")
    xt, Dft, Tt = (torch.tensor(a, device=dev) for a in (b.x, b.Df.reshape(-1, 18), b.T))
    ctx.set_params()
    want = {}
    try:
        for mode in (0, 1):
            ctx.set_gradient_mode(bool(mode))
            c, g = ctx.eval_device(xt, Dft, Tt)                     # (eager, and the warm-up: module load)
            torch.cuda.synchronize()
            want[mode] = (c.cpu().numpy(), g.cpu().numpy())
        assert not np.array_equal(want[0][1], want[1][1])
        for mode in (1, 0):
            cost = torch.empty(200, dtype=torch.float64, device=dev)
            grad = torch.empty_like(xt)
            ctx.set_gradient_mode(bool(mode))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ctx.eval_device(xt, Dft, Tt, cost=cost, grad=grad)
            ctx.set_gradient_mode(not mode)                         # the context moves on; the graph does not
            for _ in range(2):
                grad.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert np.array_equal(cost.cpu().numpy(), want[mode][0])
                assert np.array_equal(grad.cpu().numpy(), want[mode][1])
    finally:
        ctx.set_gradient_mode(False)
