"""Moving obstacles on polynomial predictions on the device (gtop_set_moving_box_polynomials) against the independent
restatement of tests/box_poly_twin.py — exact-arithmetic centres, then the C oracle's evaluateEDTWithGrad — through the
public Python wrapper: every fp64 road and body, the optimizer's three launch forms, identities that need no twin
(a degree-1 list is the constant-velocity list; a list frozen at one time is a list of parked boxes; the report's
clearance is the query's minimum), the report and the selection, the refusals, and the C++ shim.

World and parameters are tests/test_gpu_moving_cost.py's.  Boxes are aimed as its _aimed_boxes aims them, plus an
acceleration of up to 1 m/s^2 (0.2 in z): c(t) = w + v (t - when) + a (t - when)^2 / 2 in powers of t.  Before any
device result is looked at, every case asserts on the twin alone that a static lookup AND the list's constant-velocity
part {c0, c1} get enough of the trajectories wrong: a pass can come from neither the static kernels nor the
constant-velocity bodies."""
import functools

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from oracle import mma_twin
from tests import box_poly_twin as bpt
from tests import consistent_twin as ct
from tests import moving_twin, scenes
from tests import validate_twin as vt
from tests.test_gpu_moving_cost import PARAMS, TOL, _aimed_boxes, _share_changed, _static

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
ACC = np.array([1.0, 1.0, 0.2])       # m/s^2, the largest acceleration per axis
NONE = np.zeros((0, 3))


@pytest.fixture(scope="module")
def world(gtop, oracle_mod):
    mp = problem.make_map((64, 56, 40), density=0.05, seed=5)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    ctx.set_params(**PARAMS)
    yield mp, sdf, ctx
    ctx.close()


def _reset(ctx):
    ctx.set_moving_cost(False)
    ctx.set_start_times(None)
    ctx.set_moving_boxes(NONE, NONE, NONE)
    ctx.set_gradient_mode(False)
    ctx.set_launch_geometry(0, 0)
    ctx.set_optimizer_fusion(2)
    ctx.set_optimizer_precision("f64")
    ctx.set_params(**PARAMS)


def aimed_polynomials(b, t0, rng, nbox):
    """_aimed_boxes' boxes with an acceleration: (coef (nbox, 3, 6), scale, (w, v, a, when))."""
    j = rng.integers(0, len(b.x), nbox)
    w = rng.integers(0, b.m + 1, nbox)
    vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * np.array([1.0, 1.0, 0.2])
    when = np.array([t0[jj] + b.T[jj][:ww].sum() for jj, ww in zip(j, w)])
    scale = rng.uniform(1.0, 2.0, (nbox, 3))
    acc = rng.uniform(-1.0, 1.0, (nbox, 3)) * ACC
    return bpt.coefficients(b.waypoints[j, w], vel, acc, when), scale, (b.waypoints[j, w], vel, acc, when)


_cases = {}


def poly_case(oracle_mod, mp, sdf, m, nbox, B=48):
    """The (m, nbox) case and its twin results, computed once: dict(b, t0, coef, scale, c, g, infos, share_static,
    share_cv).  The two shares are asserted here, on the twin alone."""
    key = (m, nbox, B)
    if key not in _cases:
        b = problem.make_trajectories(B, m, mp, seed=40 + m)
        rng = np.random.default_rng(1000 * m + nbox)
        t0 = rng.uniform(0.0, 5.0, B)
        coef, scale, _ = aimed_polynomials(b, t0, rng, nbox)
        c, g, infos = bpt.eval_batch(b.T, b.Df, b.x, sdf, PARAMS, coef, scale, t0=t0)
        c_st, _ = _static(oracle_mod, b, sdf)
        share_static = _share_changed(infos, c, c_st)
        p0, vel = bpt.constant_velocity_part(coef)
        c_cv, _, _ = moving_twin.eval_batch(b.T, b.Df, b.x, sdf, PARAMS, p0, vel, scale, t0=t0)
        share_cv = float(np.mean(np.abs(c - c_cv) > 1e-6 * np.abs(c_cv)))
        print(f"m={m} nbox={nbox}: share of trajectories a static lookup gets wrong {share_static:.3f}, "
              f"the constant-velocity part {share_cv:.3f}")
        need = 1 / 8 if nbox == 1 else 1 / 2
        assert share_static >= need and share_cv >= need, (share_static, share_cv)
        _cases[key] = dict(b=b, t0=t0, coef=coef, scale=scale, c=c, g=g, infos=infos, share_static=share_static,
                           share_cv=share_cv)
    return _cases[key]


def _set_case(ctx, k):
    ctx.set_moving_box_polynomials(k["coef"], k["scale"])
    ctx.set_moving_cost(True)
    ctx.set_start_times(k["t0"])
    ctx.set_problem(k["b"].T, k["b"].Df)


@pytest.mark.parametrize("m,nbox", [(2, 1), (2, 32), (6, 8), (6, 32), (13, 8)])
def test_parity_with_the_twin(gtop, oracle_mod, world, m, nbox):
    """The ten-lane body (m = 2), the five-lane body (6) and the 12-segments-at-a-time body (13): eval_batch,
    eval_device and cost_nlopt (row 0 of the problem, and row 17 as a problem of its own)."""
    import torch
    mp, sdf, ctx = world
    _reset(ctx)
    k = poly_case(oracle_mod, mp, sdf, m, nbox)
    b, t0, c_ref, g_ref = k["b"], k["t0"], k["c"], k["g"]
    _set_case(ctx, k)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_POLYNOMIAL, nbox)
    c, g = ctx.eval_batch(b.x)
    err = scenes.rel_err(c, g, c_ref, g_ref)
    print("  eval_batch", err)
    assert err <= (TOL, TOL)
    dev = torch.device("cuda:0")
    xt, Dft, Tt = (torch.tensor(a, device=dev) for a in (b.x, b.Df.reshape(-1, 18), b.T))
    cd, gd = ctx.eval_device(xt, Dft, Tt)
    torch.cuda.synchronize()
    err = scenes.rel_err(cd.cpu().numpy(), gd.cpu().numpy(), c_ref, g_ref)
    print("  eval_device", err)
    assert err <= (TOL, TOL)
    c0, g0 = ctx.cost_nlopt(b.x[0])
    err = scenes.rel_err(c0, g0, c_ref[0], g_ref[0])
    print("  cost_nlopt row 0", err)
    assert err <= (TOL, TOL)
    ctx.set_problem(b.T[17:18], b.Df[17:18])
    ctx.set_start_times(t0[17])
    ci, gi = ctx.cost_nlopt(b.x[17])
    err = scenes.rel_err(ci, gi, c_ref[17], g_ref[17])
    print("  cost_nlopt row 17", err)
    assert err <= (TOL, TOL)
    _reset(ctx)


def test_with_the_velocity_acceleration_block_and_the_consistent_gradient(gtop, oracle_mod, world):
    """The (6, 8) case with enable_dyn at step 2 (the DYN + moving body) against the twin's callback, which has the
    block; and under GTOP_GRADIENT_CONSISTENT, with and without the block, against tests/consistent_twin.py around the
    same lookup.  The twins are pure-Python loops: rows 0 .. 15 of the 48 evaluated."""
    mp, sdf, ctx = world
    _reset(ctx)
    k = poly_case(oracle_mod, mp, sdf, 6, 8)
    b, t0 = k["b"], k["t0"]
    rows = np.arange(16)
    prm = dict(PARAMS, enable_dyn=1, alpha_v=2.0, alpha_a=1.5)
    sub = (b.T[rows], b.Df[rows], b.x[rows])
    c_dyn, g_dyn, _ = bpt.eval_batch(*sub, sdf, prm, k["coef"], k["scale"], t0=t0[rows])
    assert np.all(np.abs(c_dyn - k["c"][rows]) > 1e-6 * np.abs(c_dyn))          # the block contributes on every row
    cons = functools.partial(ct.cost_grad, mode=ct.CONSISTENT)
    c_con, g_con, _ = bpt.eval_batch(*sub, sdf, PARAMS, k["coef"], k["scale"], t0=t0[rows], callback=cons)
    c_cd, g_cd, _ = bpt.eval_batch(*sub, sdf, prm, k["coef"], k["scale"], t0=t0[rows], callback=cons)
    assert scenes.rel_err(k["c"][rows], g_con, k["c"][rows], k["g"][rows])[1] > 1e-3   # the modes differ in the gradient
    _set_case(ctx, k)
    for tag, params, mode, c_ref, g_ref in (("dyn", prm, False, c_dyn, g_dyn), ("consistent", PARAMS, True, c_con, g_con),
                                            ("dyn + consistent", prm, True, c_cd, g_cd)):
        ctx.set_params(**params)
        ctx.set_gradient_mode(mode)
        c, g = ctx.eval_batch(b.x)
        err = scenes.rel_err(c[rows], g[rows], c_ref, g_ref)
        print(f"(6, 8) {tag}: eval_batch", err)
        assert err <= (TOL, TOL), tag
        if mode:        # the cost does not depend on the gradient mode
            ctx.set_gradient_mode(False)
            c_r, g_r = ctx.eval_batch(b.x)
            assert np.array_equal(c, c_r) and not np.array_equal(g, g_r)
    _reset(ctx)


def test_optimizer_three_fusion_modes_against_the_serial_twin(gtop, oracle_mod, world):
    """m = 6, 8 boxes, 16 trajectories, 12 evaluations: the three launch forms bit-identical to each other, and against
    oracle/mma_twin.minimize around the twin's callback at the bar of
    test_gpu_moving_cost.py::test_optimizer_against_the_serial_twin (evaluation counts equal; cost and point 1e-6)."""
    mp, sdf, ctx = world
    _reset(ctx)
    B, m, evals = 16, 6, 12
    b = problem.make_trajectories(B, m, mp, seed=500)
    rng = np.random.default_rng(501)
    t0 = rng.uniform(0.0, 5.0, B)
    coef, scale, _ = aimed_polynomials(b, t0, rng, 8)
    p0, vel = bpt.constant_velocity_part(coef)
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    ref = []
    for i in range(B):
        gen = moving_twin.np_twin.generator(b.T[i])
        f = lambda x, i=i, gen=gen: bpt.cost_grad(b.T[i], b.Df[i], x, sdf, PARAMS, coef, scale, t0=t0[i], gen=gen)[:2]
        ref.append(mma_twin.minimize(f, b.x[i], lb[i], ub[i], evals))
    x_ref = np.array([r["x"] for r in ref])
    c_ref = np.array([r["minf"] for r in ref])
    n_ref = np.array([r["nevals"] for r in ref])
    ctx.set_problem(b.T, b.Df)
    ctx.set_moving_cost(True)
    ctx.set_start_times(t0)
    # what the constant-velocity bodies find on the list's constant-velocity part is not the twin's optimum
    ctx.set_moving_boxes(p0, vel, scale)
    _, c_cv, _, _ = ctx.optimize_batch_ex(b.x, lb, ub, evals)
    differs = float(np.mean(np.abs(c_ref - c_cv) > 1e-6 * np.abs(c_cv)))
    print(f"rows whose optimum the curvature moves: {differs:.2f}")
    assert differs >= 0.5
    ctx.set_moving_box_polynomials(coef, scale)
    runs = {}
    for fusion in (2, 1, 0):
        ctx.set_optimizer_fusion(fusion)
        runs[fusion] = ctx.optimize_batch_ex(b.x, lb, ub, evals)
    for fusion in (1, 0):
        assert all(np.array_equal(u, v) for u, v in zip(runs[2], runs[fusion])), fusion
    xs, costs, nev, _ = runs[2]
    dc = np.abs(costs - c_ref) / np.abs(c_ref)
    dx = np.max(np.abs(xs - x_ref), axis=1) / np.maximum(1.0, np.max(np.abs(x_ref), axis=1))
    print(f"worst cost diff {dc.max():.2e}, point diff {dx.max():.2e}")
    assert np.array_equal(nev, n_ref), (nev, n_ref)
    assert np.all(dc <= 1e-6) and np.all(dx <= 1e-6), (dc, dx)
    _reset(ctx)


def test_optimizer_with_the_block_and_the_consistent_gradient_five_lanes(gtop, oracle_mod, world):
    """Nine segments (five lanes per segment in the optimizer loop), enable_dyn and GTOP_GRADIENT_CONSISTENT with a
    polynomial list: the one combination whose one-launch body runs on the one-wavefront register budget
    (gtop_wave_budget).  8 trajectories, 8 evaluations: the three launch forms bit-identical to each other — the
    separate-update form evaluates through the plain bodies —, and against the serial loop around
    tests/consistent_twin.py with the polynomial lookup at the 1e-6 of the optimizer tests."""
    mp, sdf, ctx = world
    _reset(ctx)
    B, m, evals = 8, 9, 8
    prm = dict(PARAMS, enable_dyn=1, alpha_v=2.0, alpha_a=1.5)
    b = problem.make_trajectories(B, m, mp, seed=609)
    rng = np.random.default_rng(610)
    t0 = rng.uniform(0.0, 5.0, B)
    coef, scale, _ = aimed_polynomials(b, t0, rng, 8)
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    cons = functools.partial(ct.cost_grad, mode=ct.CONSISTENT)
    ref = []
    for i in range(B):
        gen = moving_twin.np_twin.generator(b.T[i])
        f = lambda x, i=i, gen=gen: bpt.cost_grad(b.T[i], b.Df[i], x, sdf, prm, coef, scale, t0=t0[i], gen=gen,
                                                  callback=cons)[:2]
        ref.append(mma_twin.minimize(f, b.x[i], lb[i], ub[i], evals))
    x_ref = np.array([r["x"] for r in ref])
    c_ref = np.array([r["minf"] for r in ref])
    n_ref = np.array([r["nevals"] for r in ref])
    ctx.set_params(**prm)
    ctx.set_gradient_mode(True)
    ctx.set_problem(b.T, b.Df)
    ctx.set_moving_box_polynomials(coef, scale)
    ctx.set_moving_cost(True)
    ctx.set_start_times(t0)
    runs = {}
    for fusion in (2, 1, 0):
        ctx.set_optimizer_fusion(fusion)
        runs[fusion] = ctx.optimize_batch_ex(b.x, lb, ub, evals)
    for fusion in (1, 0):
        assert all(np.array_equal(u, v) for u, v in zip(runs[2], runs[fusion])), fusion
    xs, costs, nev, _ = runs[2]
    ctx.set_moving_cost(False)
    _, c_off, _, _ = ctx.optimize_batch_ex(b.x, lb, ub, evals)
    assert np.mean(np.abs(costs - c_off) > 1e-6 * np.abs(c_off)) >= 0.5      # the boxes steer the road
    dc = np.abs(costs - c_ref) / np.abs(c_ref)
    dx = np.max(np.abs(xs - x_ref), axis=1) / np.maximum(1.0, np.max(np.abs(x_ref), axis=1))
    print(f"dyn + consistent, m = 9: worst cost diff {dc.max():.2e}, point diff {dx.max():.2e}")
    assert np.array_equal(nev, n_ref), (nev, n_ref)
    assert np.all(dc <= 1e-6) and np.all(dx <= 1e-6), (dc, dx)
    _reset(ctx)


def _samples(ctx, b, t0, dt=0.01):
    """Positions and tau of every report sample, reconstructed as tests/test_gpu_validate.py::composed does: the stored
    getTraj samples and the twin's accumulated sample times.  Returns (pos (N, 3), tau (N,), counts (B,), times)."""
    B = len(b.x)
    _, stats = ctx.trajectory_stats(b.x, dt)
    cap = int(stats[:, 8].max())
    _, samples = ctx.trajectory_samples(b.x, dt, cap)
    times = [vt.sample_times(b.T[i], dt)[0] for i in range(B)]
    counts = np.array([len(t) for t in times])
    assert np.array_equal(counts, stats[:, 8])
    pos = np.concatenate([samples[i, :counts[i]] for i in range(B)])
    tau = np.concatenate([t0[i] + times[i] for i in range(B)])
    return pos, tau, counts, times


def _everything(ctx, gtop, b, pos, tau):
    """One evaluation, the two queries and the report with the list in force."""
    c, g = ctx.eval_batch(b.x)
    d, dg = ctx.edt_query(pos, tau)
    dc = ctx.edt_coarse_query(pos, tau)
    rep, _, _ = ctx.validate_batch(b.x, gtop.GtopLimits(margin=0.3, use_boxes=1))
    return dict(cost=c, grad=g, dist=d, dist_grad=dg, coarse=dc, report=rep)


def test_a_degree_one_list_is_the_constant_velocity_list(gtop, oracle_mod, world):
    """The same boxes through gtop_set_moving_box_polynomials (c0 = p0, c1 = vel, no t_range) and through
    gtop_set_moving_boxes: evaluation, edt_query, edt_coarse_query and the report within 1e-12 — and, as printed,
    whether bit-identical (the design expects it: p0 + vel * t contracts to the Horner chain's last fma)."""
    mp, sdf, ctx = world
    _reset(ctx)
    k = poly_case(oracle_mod, mp, sdf, 6, 8)
    b, t0 = k["b"], k["t0"]
    p0, vel, scale = _aimed_boxes(b, t0, np.random.default_rng(61), 8)
    coef = np.zeros((8, 3, 6))
    coef[:, :, 0], coef[:, :, 1] = p0, vel
    ctx.set_problem(b.T, b.Df)
    ctx.set_start_times(t0)
    ctx.set_moving_cost(True)
    pos, tau, _, _ = _samples(ctx, b, t0)
    pos, tau = pos[::7], tau[::7]
    ctx.set_moving_boxes(p0, vel, scale)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_CONST_VEL, 8)
    cv = _everything(ctx, gtop, b, pos, tau)
    ctx.set_moving_cost(False)
    c_off, _ = ctx.eval_batch(b.x)
    ctx.set_moving_cost(True)
    assert np.mean(np.abs(cv["cost"] - c_off) > 1e-6 * np.abs(c_off)) >= 0.5      # the boxes matter
    ctx.set_moving_box_polynomials(coef, scale)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_POLYNOMIAL, 8)
    po = _everything(ctx, gtop, b, pos, tau)
    for name in cv:
        same = np.array_equal(cv[name], po[name])
        scale_ = np.maximum(1.0, np.abs(cv[name]))
        worst = float(np.max(np.abs(cv[name] - po[name]) / scale_))
        print(f"degree-1 list vs constant-velocity list, {name}: bit-identical {same}, worst difference {worst:.2e}")
        assert worst <= 1e-12, name
    assert scenes.rel_err(po["cost"], po["grad"], cv["cost"], cv["grad"]) <= (1e-12, 1e-12)
    _reset(ctx)


def test_a_list_frozen_at_one_time_is_a_list_of_parked_boxes(gtop, oracle_mod, world):
    """Every box with t1 = t2 = T*: it stands at the twin's c(T*) at every tau.  Against boxes parked there with zero
    velocity through gtop_set_moving_boxes: cost, gradient, query distances and report bit-identical."""
    mp, sdf, ctx = world
    _reset(ctx)
    k = poly_case(oracle_mod, mp, sdf, 6, 8)
    b, t0, coef, scale = k["b"], k["t0"], k["coef"], k["scale"]
    t_star = np.random.default_rng(62).uniform(1.0, 6.0, 8)
    parked = np.array([bpt.centres(coef[i:i + 1], t_star[i], fma_=bpt.fma_fraction)[0] for i in range(8)])
    ctx.set_problem(b.T, b.Df)
    ctx.set_start_times(t0)
    ctx.set_moving_cost(True)
    pos, tau, _, _ = _samples(ctx, b, t0)
    pos, tau = pos[::7], tau[::7]
    ctx.set_moving_boxes(parked, np.zeros((8, 3)), scale)
    want = _everything(ctx, gtop, b, pos, tau)
    ctx.set_moving_box_polynomials(coef, scale, np.stack([t_star, t_star], axis=1))
    got = _everything(ctx, gtop, b, pos, tau)
    ctx.set_moving_box_polynomials(coef, scale)
    free = _everything(ctx, gtop, b, pos, tau)
    assert not np.array_equal(free["cost"], got["cost"]) and not np.array_equal(free["dist"], got["dist"])   # the clamp acts
    for name in want:
        assert np.array_equal(want[name], got[name]), name
    _reset(ctx)


@pytest.mark.parametrize("nbox", [33, 49])
def test_a_frozen_list_longer_than_one_stage_is_the_parked_list(gtop, oracle_mod, world, nbox):
    """A POLYNOMIAL list of more boxes than one LDS stage holds — 33: the whole-trajectory report takes 32 a stage and
    restages inside its sample loop; 49: the query takes 48 — under the frozen-list law: every box with t1 = t2 = T*,
    against the same boxes parked at the twin's c(T*) with zero velocity through gtop_set_moving_boxes, a list that is
    one stage in both kernels.  The report, the segment report, the query's distance and gradient and the coarse query
    are bit-identical between the two kinds; the report's clearance is the query's minimum over the report's own
    samples; and the LAST box, put on the middle waypoint of the row with the most clearance, decides that row's
    clearance, so the boxes behind the first stage are read.  The (6, 8) case's 48 rows of 6 segments."""
    mp, sdf, ctx = world
    _reset(ctx)
    k = poly_case(oracle_mod, mp, sdf, 6, 8)
    b, t0 = k["b"], k["t0"]
    B, margin = len(b.x), 0.3
    lim = gtop.GtopLimits(margin=margin, use_boxes=1)
    rng = np.random.default_rng(7000 + nbox)
    coef, scale, _ = aimed_polynomials(b, t0, rng, nbox)
    scale *= 0.4                                     # many boxes: smaller ones, so that rows keep some clearance
    t_star = rng.uniform(1.0, 6.0, nbox)
    frozen = np.stack([t_star, t_star], axis=1)
    ctx.set_problem(b.T, b.Df)
    ctx.set_start_times(t0)
    # the list without its last box is one stage in the kernel the case is about; the last box goes where it matters
    ctx.set_moving_box_polynomials(coef[:-1], scale[:-1], frozen[:-1])
    rep_less, _, _ = ctx.validate_batch(b.x, lim)
    row = int(np.argmax(rep_less[:, 1]))
    assert rep_less[row, 1] > 0.0
    coef[-1] = 0.0
    coef[-1, :, 0], scale[-1] = b.waypoints[row, (b.m + 1) // 2], 0.8
    parked = np.array([bpt.centres(coef[i:i + 1], t_star[i], fma_=bpt.fma_fraction)[0] for i in range(nbox)])
    pos, tau, counts, times = _samples(ctx, b, t0)
    dist_less, _ = ctx.edt_query(pos, tau)

    def everything():
        rep, _, _ = ctx.validate_batch(b.x, lim)
        d, dg = ctx.edt_query(pos, tau)
        return dict(report=rep, segments=ctx.validate_segments(b.x, lim), dist=d, dist_grad=dg,
                    coarse=ctx.edt_coarse_query(pos, tau))

    ctx.set_moving_boxes(parked, np.zeros((nbox, 3)), scale)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_CONST_VEL, nbox)
    want = everything()
    ctx.set_moving_box_polynomials(coef, scale, frozen)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_POLYNOMIAL, nbox)
    got = everything()
    for name in want:
        assert np.array_equal(want[name], got[name]), name
    # the report's clearance is the minimum of the query at the report's own samples
    rep, dist = got["report"], got["dist"]
    o = 0
    for i in range(B):
        d = dist[o:o + counts[i]]
        j = int(np.argmin(d))
        assert (rep[i, 0], rep[i, 1], rep[i, 2], rep[i, 3]) == (counts[i], d[j], times[i][j], j), i
        below = np.flatnonzero(d <= margin)
        assert rep[i, 4] == len(below) and rep[i, 5] == (times[i][below[0]] if len(below) else -1.0), i
        o += counts[i]
    # the last box of the list is read: it lowers its row's clearance, and nothing rises
    print(f"{nbox} boxes: row {row}, clearance {rep_less[row, 1]:.3f} without the last box, {rep[row, 1]:.3f} with it")
    assert np.all(rep[:, 1] <= rep_less[:, 1]) and rep[row, 1] < rep_less[row, 1]
    assert np.all(dist <= dist_less) and np.any(dist < dist_less)
    seg_row = got["segments"][row]
    assert seg_row[:, 2].min() == rep[row, 1]
    # the clamp acts: the same list running free gives another report
    ctx.set_moving_box_polynomials(coef, scale)
    free, _, _ = ctx.validate_batch(b.x, lim)
    assert not np.array_equal(free, rep)
    _reset(ctx)


def test_report_clearance_is_the_minimum_of_the_query_and_matches_the_twin(gtop, oracle_mod, world):
    """The (6, 8) case.  (c) edt_query at the report's own samples: its minimum per trajectory IS report[:, 1], bit for
    bit, with the first index and time.  (4) validate_batch with use_boxes against tests/validate_twin.py fed the twin's
    distances, every row, at that file's bars — entries 0 .. 6 and 11 equal
    where the two distances are (1e-12 on the clearance otherwise), 7 .. 10 within vel_acc_bounds(1e-12) — and the
    selection by the twin's rule.  At least one row fails the margin on a curved box its constant-velocity part
    passes: asserted on the twin first."""
    mp, sdf, ctx = world
    _reset(ctx)
    k = poly_case(oracle_mod, mp, sdf, 6, 8)
    b, t0, coef, scale = k["b"], k["t0"], k["coef"], k["scale"]
    B, margin = len(b.x), 0.3
    rows = np.arange(B)
    _set_case(ctx, k)
    coeff, _ = ctx.trajectory_stats(b.x, 0.01)
    p0, vel = bpt.constant_velocity_part(coef)
    twin, twin_cv = [], []
    for i in rows:
        twin.append(bpt.report(oracle_mod, coeff[i], b.T[i], sdf, margin, coef, scale, t0=t0[i]))
        twin_cv.append(vt.report(oracle_mod, coeff[i], b.T[i], sdf, margin, p0, vel, scale, t0=t0[i], use_boxes=True))
    r_twin = np.array([t[0] for t in twin])
    r_cv = np.array([t[0] for t in twin_cv])
    curved_only = np.flatnonzero((r_twin[:, 4] > 0) & (r_cv[:, 4] == 0))
    print(f"rows that fail margin {margin} only on the curved boxes (twin): {curved_only}")
    assert curved_only.size >= 1
    lim = gtop.GtopLimits(margin=margin, use_boxes=1)
    cost = k["c"]
    rep, ok, best = ctx.validate_batch(b.x, lim, cost=cost)
    # (c) the query at the report's samples
    pos, tau, counts, times = _samples(ctx, b, t0)
    dist, _ = ctx.edt_query(pos, tau)
    o = 0
    for i in range(B):
        d = dist[o:o + counts[i]]
        j = int(np.argmin(d))
        assert (rep[i, 0], rep[i, 1], rep[i, 2], rep[i, 3]) == (counts[i], d[j], times[i][j], j), i
        below = np.flatnonzero(d <= margin)
        assert rep[i, 4] == len(below) and rep[i, 5] == (times[i][below[0]] if len(below) else -1.0), i
        if i in rows:       # the same samples against the twin's distances
            dt = twin[i][1]["dist"]
            assert np.max(np.abs(d - dt) / np.maximum(1.0, np.abs(dt))) <= 1e-12, i
        o += counts[i]
    # (4) the report against the twin's
    for n, i in enumerate(rows):
        want, data = twin[n]
        assert rep[i, 0] == want[0] and rep[i, 6] == want[6] and rep[i, 11] == want[11], i
        assert abs(rep[i, 1] - want[1]) <= 1e-12 * max(1.0, abs(want[1])), i
        tie = np.abs(data["dist"] - data["dist"].min()) <= 1e-12          # (a different sample may win a tie)
        assert rep[i, 3] == want[3] or tie[int(rep[i, 3])], i
        near = np.abs(data["dist"] - margin) <= 1e-12                     # ... and a sample on the margin may go either way
        if not near.any():
            assert rep[i, 4] == want[4] and rep[i, 5] == want[5], i
        assert np.all(np.abs(rep[i, 7:11] - want[7:11]) <= vt.vel_acc_bounds(data, 1e-12)), i
    assert np.all(rep[curved_only, 4] > 0)
    # the constant-velocity part through the device passes those rows
    ctx.set_moving_boxes(p0, vel, scale)
    rep_cv, _, _ = ctx.validate_batch(b.x, lim, cost=cost)
    assert np.all(rep_cv[curved_only, 4] == 0)
    ctx.set_moving_box_polynomials(coef, scale)
    ok_twin, best_twin = vt.select(rep, cost)
    assert np.array_equal(ok.astype(bool), ok_twin) and np.array_equal(best, best_twin)
    assert 0 < best[1] < B
    _reset(ctx)


def test_refusals_and_state(gtop, oracle_mod, world):
    import torch
    mp, sdf, ctx = world
    _reset(ctx)
    k = poly_case(oracle_mod, mp, sdf, 6, 8)
    b, t0, coef, scale = k["b"], k["t0"], k["coef"], k["scale"]
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    pos, tau = b.waypoints[:, 3], t0 + 2.0
    # the parent's sequence: a constant-velocity list, then everything
    boxes = _aimed_boxes(b, t0, np.random.default_rng(63), 8)
    ctx.set_problem(b.T, b.Df)
    ctx.set_start_times(t0)
    ctx.set_moving_cost(True)
    ctx.set_moving_boxes(*boxes)
    cv = _everything(ctx, gtop, b, pos, tau)
    cv_opt = ctx.optimize_batch_ex(b.x, lb, ub, 5)
    _set_case(ctx, k)

    def still_fine():
        assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_POLYNOMIAL, 8)
        c, g = ctx.eval_batch(b.x)
        assert scenes.rel_err(c, g, k["c"], k["g"]) <= (TOL, TOL)
        d, _ = ctx.edt_query(pos, tau)
        assert np.array_equal(d, d_before)

    d_before, _ = ctx.edt_query(pos, tau)
    d_twin, _ = bpt.edt_query(sdf, pos, tau, coef, scale)
    assert np.max(np.abs(d_before - d_twin)) <= 1e-12 * max(1.0, np.max(np.abs(d_twin)))
    tr = np.stack([np.zeros(8), np.full(8, 9.0)], axis=1)
    bad_lists = []
    t = tr.copy(); t[3] = (2.0, 1.0); bad_lists.append((coef, scale, t))                 # t1 > t2
    t = tr.copy(); t[5, 0] = np.nan; bad_lists.append((coef, scale, t))                  # a NaN bound
    t = tr.copy(); t[0, 1] = np.nan; bad_lists.append((coef, scale, t))
    c_ = coef.copy(); c_[2, 1, 4] = np.inf; bad_lists.append((c_, scale, tr))            # a non-finite coefficient
    c_ = coef.copy(); c_[7, 0, 0] = np.nan; bad_lists.append((c_, scale, None))
    s_ = scale.copy(); s_[1, 2] = -0.5; bad_lists.append((coef, s_, tr))                 # a negative extent
    s_ = scale.copy(); s_[6, 0] = np.inf; bad_lists.append((coef, s_, None))             # a non-finite extent
    for n, (c_, s_, t_) in enumerate(bad_lists):
        with pytest.raises(gtop.GtopError) as e:
            ctx.set_moving_box_polynomials(c_, s_, t_)
        assert e.value.code == ERR_INVALID, n
        still_fine()
    # infinite bounds are fine and clamp nothing: the list without t_range
    ctx.set_moving_box_polynomials(coef, scale, np.stack([np.full(8, -np.inf), np.full(8, np.inf)], axis=1))
    still_fine()
    # fp32 with the mode on
    dev = torch.device("cuda:0")
    x32, Df32, T32 = (torch.tensor(a, device=dev, dtype=torch.float32) for a in (b.x, b.Df.reshape(-1, 18), b.T))
    with pytest.raises(gtop.GtopError) as e:
        ctx.eval_device(x32, Df32, T32)
    assert e.value.code == ERR_STATE
    ctx.set_optimizer_precision("f32")
    with pytest.raises(gtop.GtopError) as e:
        ctx.optimize_batch_ex(b.x, lb, ub, 5)
    assert e.value.code == ERR_STATE
    ctx.set_optimizer_precision("f64")
    still_fine()
    # 33 polynomial boxes: the queries and the report take them, an evaluation in moving mode does not
    nmax = gtop.GtopContext.MOVING_COST_MAX_BOXES
    many_coef, many_scale, _ = aimed_polynomials(b, t0, np.random.default_rng(64), nmax + 1)
    ctx.set_moving_box_polynomials(many_coef, many_scale)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_POLYNOMIAL, nmax + 1)
    d, _ = ctx.edt_query(pos, tau)
    d_twin, _ = bpt.edt_query(sdf, pos, tau, many_coef, many_scale)
    assert np.max(np.abs(d - d_twin)) <= 1e-12 * max(1.0, np.max(np.abs(d_twin)))
    ctx.set_moving_box_polynomials(many_coef[:nmax], many_scale[:nmax])
    d32, _ = ctx.edt_query(pos, tau)
    rep32, _, _ = ctx.validate_batch(b.x, gtop.GtopLimits(margin=0.3, use_boxes=1))
    ctx.set_moving_box_polynomials(many_coef, many_scale)
    rep33, _, _ = ctx.validate_batch(b.x, gtop.GtopLimits(margin=0.3, use_boxes=1))   # (the report restages past 32)
    assert np.all(d <= d32) and np.all(rep33[:, 1] <= rep32[:, 1])
    with pytest.raises(gtop.GtopError) as e:
        ctx.eval_batch(b.x)
    assert e.value.code == ERR_INVALID
    with pytest.raises(gtop.GtopError) as e:
        ctx.optimize_batch_ex(b.x, lb, ub, 5)
    assert e.value.code == ERR_INVALID
    # nbox = 0 clears the list under either call
    ctx.set_moving_box_polynomials(np.zeros((0, 3, 6)), NONE)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_CONST_VEL, 0)
    ctx.set_moving_box_polynomials(coef, scale)
    ctx.set_moving_boxes(NONE, NONE, NONE)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_CONST_VEL, 0)
    # a constant-velocity list after a polynomial one: the kind and every result as if the polynomial list had never been
    ctx.set_moving_box_polynomials(coef, scale)
    ctx.set_moving_boxes(*boxes)
    assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_CONST_VEL, 8)
    again = _everything(ctx, gtop, b, pos, tau)
    for name in cv:
        assert np.array_equal(cv[name], again[name]), name
    again_opt = ctx.optimize_batch_ex(b.x, lb, ub, 5)
    assert all(np.array_equal(u, v) for u, v in zip(cv_opt, again_opt))
    _reset(ctx)


def test_cpp_shim_sets_predictions(gtop, tmp_path):
    """GradTrajOptimizer::setMovingObstaclePredictions (tests/cpp/prediction_shim.cpp) on the reference's own scene with
    two curved boxes over the path: its costFunc at the start (step 1) and after a 40-evaluation optimisation
    (step 2) against the Python binding's cost_nlopt on the same inputs, bit for bit."""
    f = scenes.write_scene(tmp_path / "scene.txt", scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES,
                           scenes.opti_node_obstacles(), scenes.OPTI_NODE_PATH)
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)
    t_start = 1.5
    T = problem.segment_times(wp[None])[0]            # each box is over its waypoint when the trajectory is
    when = t_start + np.array([T[:3].sum(), T[:7].sum()])
    coef = bpt.coefficients(wp[[3, 7]] + (0.0, 0.0, 0.2), [(0.6, -0.4, 0.0), (-0.5, 0.3, 0.05)],
                            [(0.8, 0.5, 0.0), (-0.6, 0.9, 0.1)], when)
    scale = np.array([(1.2, 1.0, 1.5), (1.0, 1.4, 1.1)])
    t_range = np.array([(0.0, when[0] + 1.0), (when[1] - 1.5, when[1] + 0.25)])
    with open(f, "a") as out:
        out.write("start_time %.17g\npredictions 2\n" % t_start)
        for i in range(2):
            out.write(" ".join("%.17g" % v for v in (*coef[i].reshape(-1), *t_range[i], *scale[i])) + "\n")
    res = scenes.run_scene(f, 40, exe_name="gtop_prediction_shim")
    assert res["refused"] == 1                       # the backwards interval was reported, the next call went through
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES)
        ctx.update_sdf_map(scenes.opti_node_obstacles())
        Df, _ = problem.initial_derivatives(wp[None])
        ctx.set_problem(np.array(res["segment_times"])[None], Df)
        ctx.set_start_times(t_start)
        costs = {}
        for state, step in (("start", 1), ("optimised", 2)):
            s = res[state]
            assert s["ok"] == 1
            ctx.set_params(**dict(gtop.OPTI_NODE_PARAMS, step=step))
            ctx.set_moving_cost(False)
            c_off, _ = ctx.cost_nlopt(np.array(s["x"]))
            ctx.set_moving_box_polynomials(coef, scale, t_range)
            ctx.set_moving_cost(True)
            c, g = ctx.cost_nlopt(np.array(s["x"]))
            assert c == s["cost"] and np.array_equal(g, np.array(s["grad"])), state
            assert c != c_off, state                  # the boxes are in the shim's cost
            p0, vel = bpt.constant_velocity_part(coef)
            ctx.set_moving_boxes(p0, vel, scale)
            c_cv, _ = ctx.cost_nlopt(np.array(s["x"]))
            assert c != c_cv, state                   # ... as curved boxes
            costs[state] = c
            print(state, "cost", c, "static", c_off, "constant-velocity part", c_cv)
        assert not np.array_equal(res["start"]["x"], res["optimised"]["x"])
    finally:
        ctx.close()
