"""The trajectory report and the selection on the device (gtop_validate_trajectories_device, gtop_select_best_device,
gtop_validate_batch) through the public Python wrapper.  Entries 0 .. 6 and 11 against the composition of the entry
points that existed before (trajectory_samples + edt_query + numpy min / argmin / count, trajectory_stats): the kernel
is specified as the same expressions, so array_equal, no tolerance.  Entries 7 .. 10 against the numpy twin
(tests/validate_twin.py) at 1e-12 of the sum of the absolute values of the polynomial's terms.  The selection against
the twin's rule; the entry points' behaviour (host = device, graph replay, refusals); and validation after an
optimisation."""
import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import validate_twin as vt
from tests.test_validate import known_answer_quintic

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
PARAMS = dict(ws=1.0, wc=5.0, alpha=10.0, r=0.5, d0=0.8, alpha_v=0.0, r_v=1.5, v0=2.5, alpha_a=0.0, r_a=1.5, a0=3.5,
              step=2, enable_dyn=0)
MARGIN = 0.3
# (grid, density, B, m, seed): the scenes of tests/test_moving_cost.py's _scene helper at other sizes
SCENES = {"dense": ((48, 40, 24), 0.04, 64, 6, 7), "wide": ((100, 100, 30), 0.03, 128, 6, 11),
          "long": ((48, 40, 24), 0.04, 32, 13, 21)}


def _scene(grid, density, B, m, seed):
    mp = problem.make_map(grid, density=density, seed=seed)
    b = problem.make_trajectories(B, m, mp, seed=seed + 1)
    return mp, b


def _boxes(b, rng, nbox, moving=True):
    """Boxes near the batch's own waypoints (so that they matter), 1 .. 2 m wide."""
    j = rng.integers(0, len(b.x), nbox)
    w = rng.integers(0, b.m + 1, nbox)
    p0 = b.waypoints[j, w] + rng.uniform(-0.3, 0.3, (nbox, 3))
    vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * (1.0, 1.0, 0.2) if moving else np.zeros((nbox, 3))
    scale = rng.uniform(1.0, 2.0, (nbox, 3))
    return p0, vel, scale


def with_out_of_map_row(b, mp):
    """The batch plus one constructed row: row 0's waypoints with the middle one 1 m beyond max_range in x."""
    wp = b.waypoints[:1].copy()
    wp[0, (b.m + 1) // 2, 0] = mp.origin[0] + mp.map_size[0] + 1.0
    T = problem.segment_times(wp)
    Df, Dp = problem.initial_derivatives(wp)
    return problem.Batch(np.concatenate([b.waypoints, wp]), np.concatenate([b.T, T]), np.concatenate([b.Df, Df]),
                         np.concatenate([b.x, Dp.reshape(1, -1)]), b.m)


def make_ctx(gtop, mp, signed=None):
    ctx = gtop.GtopContext(device=0)
    if signed is not None:
        ctx.set_field_sign(True, signed)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    ctx.set_params(**PARAMS)
    return ctx


def set_boxes(ctx, boxes):
    none = np.zeros((0, 3))
    ctx.set_moving_boxes(*(boxes if boxes is not None else (none, none, none)))


def composed(ctx, mp, b, x, dt, margin, use_boxes, t0, signed=False):
    """Entries 0 .. 6 and 11 from the entry points the library had before the report: the stored samples, one
    edt_query over all of them at tau = t0[b] + eval_t (numpy's fp64 addition) or -1, and numpy reductions.
    t0: None, a scalar or (B,).  Returns (expected (B, 12) with NaN in 7 .. 10, rows compared)."""
    B = len(x)
    _, stats = ctx.trajectory_stats(x, dt)
    cap = int(stats[:, 8].max())
    stats2, samples = ctx.trajectory_samples(x, dt, cap)
    assert np.array_equal(stats, stats2)
    t0 = np.broadcast_to(np.float64(0.0) if t0 is None else np.asarray(t0, dtype=np.float64), (B,))
    times = [vt.sample_times(b.T[i], dt)[0] for i in range(B)]
    counts = np.array([len(t) for t in times])
    assert np.array_equal(counts, stats[:, 8])                       # the twin's accumulated times are the kernel's count
    pos = np.concatenate([samples[i, :counts[i]] for i in range(B)])
    tau = np.concatenate([(t0[i] + times[i]) if use_boxes else np.full(counts[i], -1.0) for i in range(B)])
    dist, _ = ctx.edt_query(pos, tau)
    oom = vt.out_of_map(pos, mp.origin, mp.origin + mp.map_size)
    if signed:          # a signed field may hold -1 inside the map too
        assert np.all(dist[oom] == -1.0)
    else:
        assert np.array_equal(dist == -1.0, oom)
    exp = np.full((B, 12), np.nan)
    o = 0
    for i in range(B):
        d, t = dist[o:o + counts[i]], times[i]
        k = int(np.argmin(d))
        below = np.flatnonzero(d <= margin)
        exp[i, :7] = (counts[i], d[k], t[k], k, len(below), t[below[0]] if len(below) else -1.0,
                      np.count_nonzero(oom[o:o + counts[i]]))
        exp[i, 11] = stats[i, 0]
        o += counts[i]
    return exp, B


def check_exact(rep, exp):
    cols = [0, 1, 2, 3, 4, 5, 6, 11]
    bad = np.flatnonzero((rep[:, cols] != exp[:, cols]).any(axis=1))
    assert bad.size == 0, (bad[:5], rep[bad[:3]], exp[bad[:3]])


def check_vel_acc(ctx, b, x, rep, dt):
    """Entries 7 .. 10 against the twin, every row."""
    coeff, _ = ctx.trajectory_stats(x, dt)
    worst = 0.0
    for i in range(len(x)):
        kin = vt.kinematics(coeff[i], b.T[i], dt)
        want = vt.reduce_report(kin["t"], np.ones(len(kin["t"])), np.zeros(len(kin["t"]), dtype=bool), kin, 0.0)[7:11]
        tol = vt.vel_acc_bounds(kin, 1e-12)
        err = np.abs(rep[i, 7:11] - want)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (i, rep[i, 7:11], want, tol)
        # and the sharper bound the two evaluation orders themselves allow (vt.VEL_ACC_EPS has the count)
        assert np.all(err <= vt.vel_acc_bounds(kin, vt.VEL_ACC_EPS * np.finfo(np.float64).eps)), (i, err, tol)
    print(f"entries 7..10: worst error / bound = {worst:.3g} over {len(x)} rows")
    return len(x)


@pytest.fixture(scope="module", params=list(SCENES))
def world(request, gtop):
    mp, b = _scene(*SCENES[request.param])
    ctx = make_ctx(gtop, mp)
    boxes = _boxes(b, np.random.default_rng(3), 8)
    be = with_out_of_map_row(b, mp)
    yield request.param, mp, b, be, ctx, boxes
    ctx.close()


def test_scene_is_not_vacuous_and_report_matches_the_composition(world, gtop):
    name, mp, b, be, ctx, boxes = world
    B = len(b.x)
    ctx.set_problem(be.T, be.Df)
    ctx.set_start_times(None)
    reps = {}
    for use_boxes in (0, 1):
        set_boxes(ctx, boxes)
        lim = gtop.GtopLimits(margin=MARGIN, use_boxes=use_boxes)
        rep, _, _ = ctx.validate_batch(be.x, lim)
        exp, compared = composed(ctx, mp, be, be.x, 0.01, MARGIN, use_boxes, None)
        assert compared == B + 1 == len(rep)                       # no row is left out
        check_exact(rep, exp)
        assert check_vel_acc(ctx, be, be.x, rep, 0.01) == B + 1
        reps[use_boxes] = rep
        # the scene's own rows: no out-of-map sample, some pass and some fail the margin
        assert np.all(rep[:B, 6] == 0)
        fails = np.count_nonzero(rep[:B, 4] > 0)
        print(f"{name}: use_boxes={use_boxes}: {fails}/{B} rows fail margin {MARGIN}, samples "
              f"{int(rep[:B, 0].min())}..{int(rep[:B, 0].max())}")
        assert 0 < fails < B
        # the constructed row
        assert rep[B, 6] > 0 and rep[B, 1] == -1.0 and rep[B, 4] >= rep[B, 6]
    lowered = np.count_nonzero(reps[1][:B, 1] < reps[0][:B, 1])
    print(f"{name}: the boxes lower the clearance of {lowered}/{B} rows")
    assert lowered >= B // 4
    assert np.array_equal(reps[0][:, [0, 7, 8, 9, 10, 11]], reps[1][:, [0, 7, 8, 9, 10, 11]])
    # static reports ignore boxes and start times altogether
    ctx.set_start_times(3.0)
    rep, _, _ = ctx.validate_batch(be.x, gtop.GtopLimits(margin=MARGIN, use_boxes=0))
    assert np.array_equal(rep, reps[0])
    set_boxes(ctx, None)
    rep, _, _ = ctx.validate_batch(be.x, gtop.GtopLimits(margin=MARGIN, use_boxes=1))
    assert np.array_equal(rep, reps[0])
    ctx.set_start_times(None)


def test_report_does_not_depend_on_the_wavefronts_per_trajectory(world, gtop):
    """The launcher gives a trajectory 4, 2 or 1 wavefronts by the batch size (on 256 compute units: up to 1 024 / up
    to 2 048 / more rows):
    the scene's rows tiled to 1 300 and to 2 600 rows give, row for row, the report of the scene alone (which the
    tests above hold to the composition)."""
    name, mp, b, be, ctx, boxes = world
    n = len(be.x)
    t0 = np.random.default_rng(6).uniform(0.0, 4.0, n)
    set_boxes(ctx, boxes)
    lim = gtop.GtopLimits(margin=MARGIN, use_boxes=1)
    ctx.set_problem(be.T, be.Df)
    ctx.set_start_times(t0)
    try:
        rep, _, _ = ctx.validate_batch(be.x, lim)
        exp, _ = composed(ctx, mp, be, be.x, 0.01, MARGIN, 1, t0)
        check_exact(rep, exp)
        for rows in (1300, 2600):
            k = -(-rows // n)
            ctx.set_problem(np.tile(be.T, (k, 1))[:rows], np.tile(be.Df, (k, 1, 1))[:rows])
            ctx.set_start_times(np.tile(t0, k)[:rows])
            big, _, _ = ctx.validate_batch(np.tile(be.x, (k, 1))[:rows], lim)
            assert np.array_equal(big, np.tile(rep, (k, 1))[:rows]), rows
    finally:
        ctx.set_start_times(None)


def _aimed_at(b, t0, rows, rng):
    """One slow 0.8 m box per listed row, at the row's middle waypoint at the moment the trajectory is there (slow, so
    that it does not sweep the other rows of a small map as well)."""
    w = (b.m + 1) // 2
    vel = rng.uniform(-0.3, 0.3, (len(rows), 3))
    when = np.array([t0[j] + b.T[j][:w].sum() for j in rows])
    return b.waypoints[rows, w] - vel * when[:, None], vel, np.full((len(rows), 3), 0.8)


@pytest.mark.parametrize("nbox,m", [(65, 6), (100, 6), (130, 6), (130, 13)])
def test_box_lists_longer_than_one_stage(gtop, nbox, m):
    """The report kernel keeps 64 boxes in LDS; a longer list is restaged, 64 at a time, inside the sample loop (the
    query kernel it is compared with stages 128: 65 and 100 boxes are one stage there, 130 two).  The first 64 boxes
    lie near the batch's own waypoints; those of each later stage are aimed at the quarter of the rows the stages before
    leave the most clearance (an input built from a report of the shorter list, so that every stage is known to matter).  Per-row
    start times, the exact comparison with the composition — and the guards: dropping the boxes behind the first 64,
    the first 64, or the last stage raises at least one row's clearance.  (A 20 x 20 x 6 m map: in the smaller scenes
    128 boxes leave no row any clearance for a third stage to take.)"""
    name = f"m={m}"
    mp, b = _scene((100, 100, 30), 0.03, 96, m, 50 + m)
    be = with_out_of_map_row(b, mp)
    ctx = make_ctx(gtop, mp)
    n, B = len(be.x), len(b.x)
    rng = np.random.default_rng(40 + nbox)
    t0 = np.random.default_rng(nbox).uniform(0.0, 4.0, n)
    lim = gtop.GtopLimits(margin=MARGIN, use_boxes=1)
    ctx.set_problem(be.T, be.Df)
    ctx.set_start_times(t0)
    try:
        p0, vel, scale = _boxes(b, rng, 64)
        boxes = (p0, vel, 0.4 * scale)          # 0.4 .. 0.8 m: 64 of them leave most rows some clearance
        for upto in (min(nbox, 128), nbox):
            extra = upto - len(boxes[0])
            if extra <= 0:
                continue
            set_boxes(ctx, boxes)
            shorter, _, _ = ctx.validate_batch(be.x, lim)
            rows = np.argsort(-shorter[:B, 1], kind="stable")[np.arange(extra) % (B // 4)]   # a quarter of the scene's rows, clearest first
            assert np.all(shorter[rows, 1] > 0)         # an aimed box (all 8 corners inside it: distance 0) will lower them
            boxes = tuple(np.concatenate([old, new]) for old, new in zip(boxes, _aimed_at(b, t0, rows, rng)))
        p0, vel, scale = boxes
        assert len(p0) == nbox
        set_boxes(ctx, boxes)
        rep, _, _ = ctx.validate_batch(be.x, lim)
        exp, compared = composed(ctx, mp, be, be.x, 0.01, MARGIN, 1, t0)
        assert compared == n
        check_exact(rep, exp)
        parts = {"first stage only": slice(0, 64), "without the first stage": slice(64, None)}
        if nbox > 128:
            parts["without the last stage"] = slice(0, 128)
        for what, sl in parts.items():
            set_boxes(ctx, (p0[sl], vel[sl], scale[sl]))
            part, _, _ = ctx.validate_batch(be.x, lim)
            assert np.all(rep[:, 1] <= part[:, 1])
            raised = np.count_nonzero(rep[:, 1] < part[:, 1])
            print(f"{name}, {nbox} boxes, {what}: the dropped boxes decided the clearance of {raised}/{n} rows")
            assert raised >= 1, what
    finally:
        ctx.close()


@pytest.mark.parametrize("t0_form", ["default", "shared", "per_row"])
def test_start_time_forms(world, gtop, t0_form):
    name, mp, b, be, ctx, boxes = world
    ctx.set_problem(be.T, be.Df)
    set_boxes(ctx, boxes)
    n = len(be.x)
    t0 = {"default": None, "shared": 1.375, "per_row": np.random.default_rng(5).uniform(0.0, 4.0, n)}[t0_form]
    ctx.set_start_times(t0)
    try:
        rep, _, _ = ctx.validate_batch(be.x, gtop.GtopLimits(margin=MARGIN, use_boxes=1))
        exp, compared = composed(ctx, mp, be, be.x, 0.01, MARGIN, 1, t0)
        assert compared == n
        check_exact(rep, exp)
        if t0_form == "per_row":    # a prefix of the problem's rows is served by the problem-sized list
            k = n // 2
            rep_k, _, _ = ctx.validate_batch(be.x[:k], gtop.GtopLimits(margin=MARGIN, use_boxes=1))
            assert np.array_equal(rep_k, rep[:k])
    finally:
        ctx.set_start_times(None)


@pytest.mark.parametrize("m", [2, 6, 13, 40])
@pytest.mark.parametrize("dt", [0.01, 0.05])
def test_lengths_and_sampling_steps(gtop, m, dt):
    mp = problem.make_map((48, 40, 24), density=0.04, seed=7)
    b = with_out_of_map_row(problem.make_trajectories(12, m, mp, seed=30 + m), mp)
    ctx = make_ctx(gtop, mp)
    try:
        ctx.set_problem(b.T, b.Df)
        boxes = _boxes(b, np.random.default_rng(m), 8)
        set_boxes(ctx, boxes)
        t0 = np.random.default_rng(m + 1).uniform(0.0, 3.0, len(b.x))
        ctx.set_start_times(t0)
        for use_boxes in (0, 1):
            rep, _, _ = ctx.validate_batch(b.x, gtop.GtopLimits(margin=MARGIN, use_boxes=use_boxes), dt_sample=dt)
            exp, compared = composed(ctx, mp, b, b.x, dt, MARGIN, use_boxes, t0)
            assert compared == len(b.x)
            check_exact(rep, exp)
            check_vel_acc(ctx, b, b.x, rep, dt)
    finally:
        ctx.close()


def test_signed_field(gtop):
    mp, b = _scene(*SCENES["dense"])
    be = with_out_of_map_row(b, mp)
    ctx = make_ctx(gtop, mp, signed=1.0)
    try:
        assert ctx.field_sign()[0]
        ctx.set_problem(be.T, be.Df)
        boxes = _boxes(b, np.random.default_rng(3), 8)
        set_boxes(ctx, boxes)
        for use_boxes in (0, 1):
            rep, _, _ = ctx.validate_batch(be.x, gtop.GtopLimits(margin=-0.05, use_boxes=use_boxes))
            exp, _ = composed(ctx, mp, be, be.x, 0.01, -0.05, use_boxes, None, signed=True)
            check_exact(rep, exp)
        inside = np.count_nonzero(rep[:-1, 1] < 0)
        print(f"signed field: {inside}/{len(b.x)} rows go inside an obstacle")
        assert inside > 0        # the negative distances are exercised
    finally:
        ctx.close()


def test_known_answer_quintic_and_more_boxes_than_one_stage(gtop):
    """tests/golden/VALIDATE_ANALYTIC.md through the device form (one segment: coefficients given directly), in a free
    map, with 70 far-away boxes (more than the kernel stages at once)."""
    import torch
    mp = problem.make_map((48, 48, 24), density=0.0, seed=1)      # 9.6 x 9.6 x 4.8 m: the whole curve is inside
    ctx = make_ctx(gtop, mp)
    try:
        c = np.array([[0, 0, 0, 0, 0, 0.1, 1, 2, 0, 0, 0, 0, 0.5, 0, 0.5, 0, 0, 0]], dtype=np.float64)
        c[0, [0, 6, 12]] += mp.origin + 1.0          # inside the map
        dev = torch.device("cuda:0")
        coeff = torch.tensor(c.reshape(1, 1, 18), device=dev)
        T = torch.tensor([[1.5]], dtype=torch.float64, device=dev)
        far = np.tile(mp.origin + mp.map_size + 50.0, (70, 1))
        ctx.set_moving_boxes(far, np.zeros((70, 3)), np.ones((70, 3)))
        rep = ctx.validate_device(coeff, T, gtop.GtopLimits(margin=MARGIN, use_boxes=1))
        torch.cuda.synchronize()
        r = rep.cpu().numpy()[0]
        t = vt.sample_times([1.5], 0.01)[0]
        want = known_answer_quintic(t[-1])
        assert r[0] == len(t) and np.all(np.abs(r[7:12] - want) <= 1e-12 * np.abs(want)), (r, want)
        assert r[6] == 0 and r[4] == 0 and r[5] == -1.0
    finally:
        ctx.close()


def _device_problem(b, n=None):
    import torch
    dev = torch.device("cuda:0")
    n = len(b.x) if n is None else n
    return (torch.tensor(b.x[:n], device=dev), torch.tensor(b.Df[:n].reshape(-1, 18), device=dev),
            torch.tensor(b.T[:n], device=dev))


def test_selection_on_the_batchs_own_costs_and_host_equals_device(world, gtop):
    import torch
    name, mp, b, be, ctx, boxes = world
    ctx.set_problem(be.T, be.Df)
    set_boxes(ctx, boxes)
    ctx.set_start_times(None)
    cost, _ = ctx.eval_batch(be.x)
    x, Df, T = _device_problem(be)
    coeff = ctx.coefficients_device(x, Df, T)
    kin = ctx.trajectory_stats(be.x)[0]
    assert np.array_equal(coeff.cpu().numpy(), kin)
    # limits that bite on part of the batch: medians of the static report's own figures (inputs, not tolerances)
    rep0, _, _ = ctx.validate_batch(be.x, gtop.GtopLimits(margin=MARGIN))
    med = np.median(rep0[:, 7:11], axis=0)
    cases = (dict(), dict(max_vel=med[0]), dict(max_acc=med[3], per_axis=True),
             dict(max_vel=1.2 * med[0], max_acc=1.2 * med[1], use_boxes=True), dict(allow_out_of_map=True, use_boxes=True))
    for lim_kw in cases:
        lim = gtop.GtopLimits(margin=MARGIN, **lim_kw)
        rep_h, pass_h, best_h = ctx.validate_batch(be.x, lim, cost=cost)
        rep_d = ctx.validate_device(coeff, T, lim)
        pass_d, best_d = ctx.select_best_device(rep_d, torch.tensor(cost, device=x.device), lim)
        torch.cuda.synchronize()
        assert np.array_equal(rep_h, rep_d.cpu().numpy())                       # bit for bit
        assert np.array_equal(pass_h, pass_d.cpu().numpy().astype(bool)) and np.array_equal(best_h, best_d.cpu().numpy())
        sel = {k: v for k, v in lim_kw.items() if k != "use_boxes"}
        ok, best = vt.select(rep_h, cost, **sel)
        assert np.array_equal(pass_h, ok) and np.array_equal(best_h, best), (name, lim_kw, best_h, best)
        print(f"{name} {lim_kw}: {best_h[1]}/{len(cost)} pass, best row {best_h[0]}")
        assert 0 < best_h[1] < len(cost)        # every case has passing and failing rows
        _, best_np = ctx.select_best_device(rep_d, torch.tensor(cost, device=x.device), lim, want_pass=False)
        torch.cuda.synchronize()
        assert np.array_equal(best_np.cpu().numpy(), best)
    assert not pass_h[-1] and rep_h[-1, 6] > 0       # out-of-map samples are -1 <= margin: allowed or not, the row fails


def test_selection_constructed_cases(gtop):
    import torch
    mp = problem.make_map((24, 24, 24), density=0.0, seed=1)
    ctx = make_ctx(gtop, mp)
    dev = torch.device("cuda:0")
    try:
        for name, rep, cost, lim_kw in vt.selection_cases():
            lim = gtop.GtopLimits(margin=MARGIN, **lim_kw)
            ok_d, best_d = ctx.select_best_device(torch.tensor(rep, device=dev), torch.tensor(cost, device=dev), lim)
            torch.cuda.synchronize()
            ok, best = vt.select_loop(rep, cost, **lim_kw)
            assert np.array_equal(ok_d.cpu().numpy().astype(bool), ok) and np.array_equal(best_d.cpu().numpy(), best), name
        # no rows: nobody passes
        empty = torch.empty(0, 12, dtype=torch.float64, device=dev)
        _, best_d = ctx.select_best_device(empty, torch.empty(0, dtype=torch.float64, device=dev), gtop.GtopLimits(),
                                           best=torch.full((2,), 9, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        assert best_d.tolist() == [-1, 0]
    finally:
        ctx.close()


def test_selection_large_batch_returns_the_earlier_of_two_equal_minima(world, gtop):
    import torch
    name, mp, b, be, ctx, boxes = world
    ctx.set_problem(b.T, b.Df)
    set_boxes(ctx, None)
    lim = gtop.GtopLimits(margin=MARGIN)
    rep, _, _ = ctx.validate_batch(b.x, lim)
    cost, _ = ctx.eval_batch(b.x)
    B = 131072
    reps = -(-B // len(rep))
    big = np.tile(rep, (reps, 1))[:B].copy()
    bigc = np.tile(cost, reps)[:B].copy()
    first, second = 70001, 120007
    for r in (first, second):
        big[r, 4] = 0
        big[r, 6] = 0
        bigc[r] = 0.5 * cost.min()
    dev = torch.device("cuda:0")
    ok_d, best_d = ctx.select_best_device(torch.tensor(big, device=dev), torch.tensor(bigc, device=dev), lim)
    torch.cuda.synchronize()
    ok, best = vt.select(big, bigc)
    assert best[0] == first and ok[second]
    assert np.array_equal(best_d.cpu().numpy(), best) and np.array_equal(ok_d.cpu().numpy().astype(bool), ok)
    # without the planted rows every tile holds the same minimum: the first tile's wins
    big2 = np.tile(rep, (reps, 1))[:B]
    bigc2 = np.tile(cost, reps)[:B]
    _, best_d = ctx.select_best_device(torch.tensor(big2, device=dev), torch.tensor(bigc2, device=dev), lim, want_pass=False)
    torch.cuda.synchronize()
    assert np.array_equal(best_d.cpu().numpy(), vt.select(big2, bigc2)[1]) and 0 <= best_d[0].item() < len(rep)


def test_graph_replay_follows_start_times_and_boxes(world, gtop):
    """The device forms captured in a torch.cuda.graph; replayed after t0 (a borrowed device buffer) and the boxes
    changed, they give the new answer."""
    import torch
    name, mp, b, be, ctx, boxes = world
    n = len(b.x)
    ctx.set_problem(b.T, b.Df)
    set_boxes(ctx, boxes)
    x, Df, T = _device_problem(b)
    t0 = torch.zeros(n, dtype=torch.float64, device=x.device)
    ctx.set_start_times_device(t0)
    lim = gtop.GtopLimits(margin=MARGIN, use_boxes=1)
    cost = torch.tensor(ctx.eval_batch(b.x)[0], device=x.device)
    coeff = torch.empty(n, b.m, 18, dtype=torch.float64, device=x.device)
    rep = torch.zeros(n, 12, dtype=torch.float64, device=x.device)
    best = torch.zeros(2, dtype=torch.int32, device=x.device)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # warm-up outside the capture
            ctx.coefficients_device(x, Df, T, coeff=coeff)
            ctx.validate_device(coeff, T, lim, report=rep)
            ctx.select_best_device(rep, cost, lim, want_pass=False, best=best)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx.coefficients_device(x, Df, T, coeff=coeff)
            ctx.validate_device(coeff, T, lim, report=rep)
            ctx.select_best_device(rep, cost, lim, want_pass=False, best=best)
        graph.replay()
        torch.cuda.synchronize()
        first = rep.cpu().numpy().copy()
        exp, _ = composed(ctx, mp, b, b.x, 0.01, MARGIN, 1, None)
        check_exact(first, exp)
        # new start times in the borrowed buffer, new boxes in the context's (same address, same count)
        t0_new = np.random.default_rng(8).uniform(0.5, 3.0, n)
        t0.copy_(torch.tensor(t0_new, device=x.device))
        boxes2 = _boxes(b, np.random.default_rng(4), 8)
        set_boxes(ctx, boxes2)
        graph.replay()
        torch.cuda.synchronize()
        second = rep.cpu().numpy().copy()
        exp2, _ = composed(ctx, mp, b, b.x, 0.01, MARGIN, 1, t0_new)
        check_exact(second, exp2)
        assert not np.array_equal(first[:, 1], second[:, 1])
        assert np.array_equal(best.cpu().numpy(), vt.select(second, cost.cpu().numpy())[1])
    finally:
        ctx.set_start_times_device(None)
        ctx.set_start_times(None)


def test_refusals_launch_nothing(world, gtop):
    import torch
    name, mp, b, be, ctx, boxes = world
    ctx.set_problem(b.T, b.Df)
    set_boxes(ctx, boxes)
    x, Df, T = _device_problem(b)
    coeff = ctx.coefficients_device(x, Df, T)
    sentinel = -12345.0
    rep = torch.full((len(b.x), 12), sentinel, dtype=torch.float64, device=x.device)
    best = torch.full((2,), -7, dtype=torch.int32, device=x.device)
    cost = torch.ones(len(b.x), dtype=torch.float64, device=x.device)
    good = gtop.GtopLimits(margin=MARGIN)

    def refused(code, fn):
        with pytest.raises(gtop.GtopError) as ei:
            fn()
        assert ei.value.code == code, ei.value

    refused(ERR_INVALID, lambda: ctx.validate_device(coeff, T, good, dt_sample=0.0, report=rep))
    refused(ERR_INVALID, lambda: ctx.validate_device(coeff, T, good, dt_sample=-0.01, report=rep))
    for bad in (dict(margin=np.nan), dict(margin=np.inf), dict(max_vel=np.inf), dict(max_acc=np.nan)):
        lim = gtop.GtopLimits(**bad)
        refused(ERR_INVALID, lambda: ctx.validate_device(coeff, T, lim, report=rep))
        refused(ERR_INVALID, lambda: ctx.select_best_device(rep, cost, lim, best=best))
        refused(ERR_INVALID, lambda: ctx.validate_batch(b.x, lim))
    refused(ERR_INVALID, lambda: ctx.validate_batch(b.x, good, dt_sample=0.0))
    ctx.set_start_times(np.linspace(0.0, 1.0, len(b.x) + 3))            # neither 0, 1 nor B
    try:
        lim = gtop.GtopLimits(margin=MARGIN, use_boxes=1)
        refused(ERR_INVALID, lambda: ctx.validate_device(coeff, T, lim, report=rep))
        refused(ERR_INVALID, lambda: ctx.validate_batch(b.x, lim))
        refused(ERR_INVALID, lambda: ctx.validate_device(coeff, T, good, report=rep))   # a static report too
        refused(ERR_INVALID, lambda: ctx.validate_batch(b.x, good))
    finally:
        ctx.set_start_times(None)
    fresh = gtop.GtopContext(device=0)                                  # no field resident
    try:
        refused(ERR_STATE, lambda: fresh.validate_device(coeff, T, good, report=rep))
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert torch.all(rep == sentinel).item() and torch.all(best == -7).item()


def test_validation_after_optimisation(gtop):
    """The dense scene: optimise, validate before and after under the static field."""
    mp, b = _scene(*SCENES["dense"])
    ctx = make_ctx(gtop, mp)
    try:
        ctx.set_problem(b.T, b.Df)
        lim = gtop.GtopLimits(margin=MARGIN)
        cost0, _ = ctx.eval_batch(b.x)
        rep0, pass0, best0 = ctx.validate_batch(b.x, lim, cost=cost0)
        lb, ub = ctx.default_bounds(b.waypoints)
        x1, cost1, _, _ = ctx.optimize_batch_ex(b.x, lb, ub, 40)
        rep1, pass1, best1 = ctx.validate_batch(x1, lim, cost=cost1)
        print(f"passing rows before optimisation {best0[1]}, after {best1[1]} of {len(b.x)}")
        assert np.array_equal(best1, vt.select(rep1, cost1)[1]) and np.array_equal(best0, vt.select(rep0, cost0)[1])
        assert best1[1] > best0[1]
    finally:
        ctx.close()
