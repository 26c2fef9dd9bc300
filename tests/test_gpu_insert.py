"""Waypoint insertion on the device (gtop_insert_waypoints[_device]; csrc/gtop_insert.hip) through the public Python
wrapper (grad_traj_optimization_amd/insert.py).

(1) All five outputs against the numpy twin (tests/insert_twin.py), bit for bit: segment counts that put 9m and m + 1
    either side of multiples of 64 and of the arg-max's 64-lane passes, batches that do and do not fill a workgroup,
    shared and per-row times, cuts in the first, a middle and the last segment, beyond time_sum, on a junction, the
    fallbacks, ties of LONGEST, a min_fraction that clamps and one that does not; guard words around every output,
    inputs bitwise unchanged, the optional buffers left out.
(2) `when` read in place from real report and certificate buffers (strides 12 and 8); the new position is the report's
    sample, bit for bit.
(3) Row independence.  (4) The push against the composition with gtop_edt_query_device.  (5) The known answer.
(6) Host form = device form.  (7) One captured graph.  (8) Refusals.  (9) The optimizer on the new problem."""
import numpy as np
import pytest

from grad_traj_optimization_amd import certify, insert, problem
from tests import insert_twin as it
from tests.test_gpu_validate import _device_problem, _scene, make_ctx
from tests.test_insert_twin import check_constant_velocity, constant_velocity_row

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
GRID = (48, 40, 24)
GUARD, SENTINEL = 16, -12345.0
SEGMENTS = (2, 3, 6, 7, 8, 22, 64, 65, 226)
BATCHES = (1, 3, 65, 130)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def world(gtop):
    mp = problem.make_map(GRID, density=0.03, seed=3)
    ctx = make_ctx(gtop, mp)
    yield mp, ctx
    ctx.close()


class Guarded:
    """An output tensor of `shape` with GUARD sentinel words on either side, all in one allocation."""

    def __init__(self, shape, device):
        import torch
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=device)
        self.t = self.whole[GUARD:GUARD + n].view(shape)

    def guards_intact(self):
        w = self.whole
        return bool((w[:GUARD] == SENTINEL).all().item() and (w[-GUARD:] == SENTINEL).all().item())

    def untouched(self):
        return bool((self.whole == SENTINEL).all().item())


def run_device(ctx, opts, x, coeff, T, when=None, when_column=0, lb=None, ub=None, want_info=True):
    """One call with guarded outputs -> dict of numpy arrays (None for what was left out); guards and inputs checked."""
    import torch
    B, m = coeff.shape[:2]
    dev = x.device
    inputs = [a for a in (x, coeff, T, when, lb, ub) if a is not None]
    before = [a.clone() for a in inputs]
    out = dict(x_out=Guarded((B, 9 * m), dev), T_out=Guarded((B, m + 1), dev))
    if lb is not None:
        out.update(lb_out=Guarded((B, 9 * m), dev), ub_out=Guarded((B, 9 * m), dev))
    if want_info:
        out["info"] = Guarded((B, 6), dev)
    res = insert.insert_waypoints_device(ctx, opts, x, coeff, T, when=when, when_column=when_column, lb=lb, ub=ub,
                                         want_info=want_info, **{k: g.t for k, g in out.items()})
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in out.values()), [k for k, g in out.items() if not g.guards_intact()]
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(inputs, before))
    assert res[2] is None or lb is not None
    return {k: (out[k].t.cpu().numpy() if k in out else None) for k in ("x_out", "T_out", "lb_out", "ub_out", "info")}


def check_against_twin(got, want, what):
    for k in ("x_out", "T_out", "lb_out", "ub_out", "info"):
        if got[k] is None:
            continue
        if not same_bits(got[k], want[k]):
            rows = np.flatnonzero((_bits(got[k]) != _bits(want[k])).reshape(len(got[k]), -1).any(axis=1))
            raise AssertionError((what, k, rows[:5], got["info"][rows[0]] if got["info"] is not None else None,
                                  want["info"][rows[0]]))


def times_of_interest(T, rng):
    """One cut time per row, the kinds in turn: inside the first, a middle and the last segment, beyond time_sum,
    exactly on a junction, -1, NaN, +inf."""
    B, m = T.shape
    starts = np.concatenate([np.zeros((B, 1)), np.cumsum(T, axis=1)], axis=1)
    when = np.empty(B)
    for i in range(B):
        kind = i % 8
        f = rng.uniform(0.2, 0.8)
        if kind == 0:
            when[i] = f * T[i, 0]
        elif kind == 1:
            s = m // 2
            when[i] = starts[i, s] + f * T[i, s]
        elif kind == 2:
            when[i] = starts[i, m - 1] + f * T[i, m - 1]
        elif kind == 3:
            when[i] = starts[i, m] + 1.0 + f
        elif kind == 4:          # on a junction as the walk's own subtractions see it: the serial sum of the first times
            j = 1 + i % (m - 1)
            acc = np.float64(0.0)
            for s in range(j):
                acc = acc + T[i, s]
            when[i] = acc
        else:
            when[i] = (-1.0, np.nan, np.inf)[kind - 5]
    return when


def tied_times(T, rng):
    """Rows whose largest time occurs two or three times (every other row), elsewhere as they are."""
    T = T.copy()
    B, m = T.shape
    for i in range(0, B, 2):
        top = T[i].max() + 0.25
        T[i, rng.choice(m, size=min(m, 2 + i % 2), replace=False)] = top
    return T


@pytest.mark.parametrize("m", SEGMENTS)
def test_all_outputs_are_the_twins_bit_for_bit(world, gtop, m):
    import torch
    mp, ctx = world
    rng = np.random.default_rng(100 + m)
    b = problem.make_trajectories(max(BATCHES), m, mp, seed=200 + m)
    lbh, ubh = ctx.default_bounds(b.waypoints)
    forms = [(B, shared) for B in BATCHES for shared in (False, True)]
    if m > 8:                # the large rows: every batch once, the time forms alternating
        forms = [(B, bool(i % 2)) for i, B in enumerate(BATCHES)]
    seen_clamp, seen_cut, seen_fallback, seen_tie = set(), set(), 0, 0
    for B, shared in forms:
        Th = tied_times(b.T[:B], rng)
        if shared:
            Th = np.tile(Th[0], (B, 1))
        xh = b.x[:B]
        dev = torch.device("cuda:0")
        x, Df = torch.tensor(xh, device=dev), torch.tensor(b.Df[:B].reshape(-1, 18), device=dev)
        T = torch.tensor(Th[0] if shared else Th, device=dev)
        coeff = ctx.coefficients_device(x, Df, T)
        torch.cuda.synchronize()
        ch = coeff.cpu().numpy()
        bounds = B in (3, 130)
        lb = torch.tensor(lbh[:B], device=dev) if bounds else None
        ub = torch.tensor(ubh[:B], device=dev) if bounds else None
        wh = times_of_interest(Th, rng)
        when = torch.tensor(wh, device=dev)
        for mode, frac in ((it.AT_TIME, 0.1), (it.AT_TIME, 0.45), (it.LONGEST, 0.25)):
            kw = dict(mode=mode, min_fraction=frac, bos=2.5, vos=7.0, aos=9.0)
            got = run_device(ctx, gtop.GtopInsert(**kw), x, coeff, T, when=when if mode == it.AT_TIME else None,
                             lb=lb, ub=ub, want_info=B != 65)
            want = it.insert_batch(m, xh, ch, Th[0] if shared else Th, when=wh, lb=lbh[:B] if bounds else None,
                                   ub=ubh[:B] if bounds else None, **kw)
            check_against_twin(got, want, (m, B, shared, mode, frac))
            info = want["info"]
            if mode == it.AT_TIME:
                seen_clamp |= set(info[:, 3])
                seen_fallback += int(info[:, 2].sum())
                seen_cut |= {"first" if s == 0 else "last" if s == m - 1 else "middle" for s in info[info[:, 2] == 0, 0]}
            else:
                first = np.array([int(np.argmax(row)) for row in Th])
                assert np.array_equal(info[:, 0], first) and np.all(info[:, 1] == 0.5 * Th[np.arange(B), first])
                seen_tie += int(np.count_nonzero((Th == Th.max(axis=1, keepdims=True)).sum(axis=1) > 1))
    assert seen_clamp == {0.0, 1.0} and seen_fallback >= 3 and seen_tie >= 1
    assert seen_cut == ({"first", "last"} if m == 2 else {"first", "middle", "last"})


def test_when_is_read_in_place_from_report_and_certificate_and_the_position_is_the_reports_sample(world, gtop):
    import torch
    mp, ctx = world
    B, m, dt = 65, 6, 0.01
    _, b = _scene(GRID, 0.03, B, m, 3)
    x, Df, T = _device_problem(b)
    coeff = ctx.coefficients_device(x, Df, T)
    report = ctx.validate_device(coeff, T, gtop.GtopLimits(margin=0.3), dt_sample=dt)
    cert = certify.certify_device(ctx, coeff, T, certify.GtopCertifyOpts(0.3, 1, 16))
    stats, samples = ctx.sample_trajectories_device(coeff, T, dt_sample=dt, max_samples=2048)
    torch.cuda.synchronize()
    rep, cer, ch = report.cpu().numpy(), cert.cpu().numpy(), coeff.cpu().numpy()
    assert rep.shape == (B, 12) and cer.shape == (B, 8) and rep[:, 0].max() <= 2048
    assert np.any(cer[:, 4] == -1.0) and np.any(cer[:, 4] >= 0.0)        # rows without and with a violation
    kw = dict(mode=it.AT_TIME, min_fraction=2.0 ** -30)
    opts = gtop.GtopInsert(**kw)
    for buf, host, col in ((report, rep, 2), (cert, cer, 3), (cert, cer, 4)):
        got = run_device(ctx, opts, x, coeff, T, when=buf, when_column=col)
        want = it.insert_batch(m, b.x, ch, b.T, when=host[:, col], **kw)
        check_against_twin(got, want, ("column", col))
        if col == 4:
            assert np.array_equal(got["info"][:, 2], (cer[:, 4] < 0).astype(float)) and got["info"][:, 2].any()
        if col == 2:     # the new waypoint IS sample report[3] of the sampled trajectory
            idle = got["info"][:, 3] == 0
            assert np.count_nonzero(idle) >= B // 2, np.count_nonzero(idle)   # (a clearance at t = 0 is clamped)
            smp = samples.cpu().numpy()[np.arange(B), rep[:, 3].astype(int)]
            s = got["info"][:, 0].astype(int)
            p_new = got["x_out"].reshape(B, 3, 3 * m)[np.arange(B), :, 3 * s]
            assert same_bits(p_new[idle], smp[idle])


def test_a_rows_bits_depend_on_that_row_alone(world, gtop):
    import torch
    mp, ctx = world
    B, m = 130, 7
    b = problem.make_trajectories(B, m, mp, seed=77)
    Th = np.tile(b.T[5], (B, 1))                      # the same times in every row: shared and per-row forms agree
    dev = torch.device("cuda:0")
    x, Df = torch.tensor(b.x, device=dev), torch.tensor(b.Df.reshape(-1, 18), device=dev)
    T_rows, T_shared = torch.tensor(Th, device=dev), torch.tensor(Th[0], device=dev)
    coeff = ctx.coefficients_device(x, Df, T_rows)
    wh = times_of_interest(Th, np.random.default_rng(4))
    when = torch.tensor(wh, device=dev)
    lbh, ubh = ctx.default_bounds(b.waypoints)
    lb, ub = torch.tensor(lbh, device=dev), torch.tensor(ubh, device=dev)
    for mode in (it.AT_TIME, it.LONGEST):
        opts = gtop.GtopInsert(mode=mode, min_fraction=0.2)
        whole = run_device(ctx, opts, x, coeff, T_rows, when=when, lb=lb, ub=ub)
        shared = run_device(ctx, opts, x, coeff, T_shared, when=when, lb=lb, ub=ub)
        perm = torch.tensor(np.random.default_rng(5).permutation(B), device=dev)
        moved = run_device(ctx, opts, x[perm].contiguous(), coeff[perm].contiguous(), T_rows, when=when[perm].contiguous(),
                           lb=lb[perm].contiguous(), ub=ub[perm].contiguous())
        ph = perm.cpu().numpy()
        for k in whole:
            assert same_bits(whole[k], shared[k]), (mode, k)
            assert same_bits(whole[k][ph], moved[k]), (mode, k)
        for i in (0, 64, 129):
            one = run_device(ctx, opts, x[i:i + 1], coeff[i:i + 1], T_rows[i:i + 1], when=when[i:i + 1], lb=lb[i:i + 1],
                             ub=ub[i:i + 1])
            for k in whole:
                assert same_bits(whole[k][i:i + 1], one[k]), (mode, k, i)


# ---- (4) the push --------------------------------------------------------------------------------------------------
def _wall_world(gtop):
    """A 16^3 map at 0.2 m with one wall across x, and rows of two segments along x at several distances from it."""
    occ = np.zeros((16, 16, 16), dtype=np.uint8)
    occ[8, :, :] = 1
    mp = problem.MapSpec((16, 16, 16), 0.2, np.array([-1.6, -1.6, 0.0]), occ)
    ctx = make_ctx(gtop, mp)
    mid = np.array([[-1.0, 0.13, 1.5], [-0.31, -0.4, 1.1], [0.02, 0.3, 1.7], [0.35, 0.1, 0.9], [0.9, -0.7, 2.1],
                    [1.3, 0.5, 1.3], [2.5, 0.2, 1.4], [0.11, 0.2, 3.9]])        # the last two: out of the map
    wp = np.stack([mid + (-0.4, 0.05, -0.03), mid, mid + (0.3, -0.02, 0.06)], axis=1)
    T = problem.segment_times(wp)
    Df, Dp = problem.initial_derivatives(wp)
    x = Dp.reshape(len(mid), -1) + np.random.default_rng(2).normal(0.0, 0.05, (len(mid), 9))
    return mp, ctx, problem.Batch(wp, T, Df, x, 2)


def test_push_is_the_composition_with_the_distance_query(gtop):
    import torch
    mp, ctx, b = _wall_world(gtop)
    try:
        B, m = len(b.x), 2
        x, Df, T = _device_problem(b)
        coeff = ctx.coefficients_device(x, Df, T)
        when = torch.tensor(b.T[:, 0] + 2.0 ** -12, device=x.device)          # just behind the middle waypoint
        lbh, ubh = ctx.default_bounds(b.waypoints)
        lb, ub = torch.tensor(lbh, device=x.device), torch.tensor(ubh, device=x.device)
        base = dict(mode=it.AT_TIME, min_fraction=2.0 ** -20, bos=1.5)
        push, below = 0.15, 0.45
        off = run_device(ctx, gtop.GtopInsert(**base), x, coeff, T, when=when, lb=lb, ub=ub)
        on = run_device(ctx, gtop.GtopInsert(push=push, push_below=below, **base), x, coeff, T, when=when, lb=lb, ub=ub)
        assert np.all(off["info"][:, 4:] == 0) and np.all(off["info"][:, 0] == 1)
        p0 = off["x_out"].reshape(B, 3, 6)[:, :, 3]
        d, g = ctx.edt_query_device(torch.tensor(p0, device=x.device), torch.full((B,), -1.0, dtype=torch.float64,
                                                                                  device=x.device))
        torch.cuda.synchronize()
        d, g = d.cpu().numpy(), g.cpu().numpy()
        out = np.any((p0 < mp.origin + 1e-4) | (p0 > mp.origin + mp.map_size - 1e-4), axis=1)
        assert np.array_equal(d == -1.0, out) and out.sum() == 2
        n = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        moved = ~out & ~(d >= below) & ~(n == 0.0)
        assert 2 <= moved.sum() <= B - 4 and np.any(~out & (d >= below))     # near rows, far rows, out-of-map rows
        with np.errstate(invalid="ignore", divide="ignore"):
            p_want = np.where(moved[:, None], p0 + (push * g) / n[:, None], p0)
        assert same_bits(on["info"][:, 4], d) and np.array_equal(on["info"][:, 5], moved.astype(float))
        assert same_bits(on["info"][:, :4], off["info"][:, :4]) and same_bits(on["T_out"], off["T_out"])
        want_x = off["x_out"].reshape(B, 3, 6).copy()
        want_x[:, :, 3] = p_want
        assert same_bits(on["x_out"], want_x.reshape(B, 18))
        want_lb, want_ub = off["lb_out"].reshape(B, 3, 6).copy(), off["ub_out"].reshape(B, 3, 6).copy()
        want_lb[:, :, 3], want_ub[:, :, 3] = p_want - 1.5, p_want + 1.5
        assert same_bits(on["lb_out"], want_lb.reshape(B, 18)) and same_bits(on["ub_out"], want_ub.reshape(B, 18))
        assert np.all(np.abs(np.linalg.norm(p_want[moved] - p0[moved], axis=1) - push) < 1e-12)
        # and the twin with the device's own lookup
        table = {p0[i].tobytes(): (d[i], g[i], bool(out[i])) for i in range(B)}
        want = it.insert_batch(m, b.x, coeff.cpu().numpy(), b.T, when=when.cpu().numpy(), lb=lbh, ub=ubh, push=push,
                               push_below=below, lookup=lambda p: table[p.tobytes()], **base)
        check_against_twin(on, want, "push")
        # a field without a gradient: nothing moves
        flat = gtop.GtopContext(device=0)
        try:
            flat.set_sdf(np.full((16, 16, 16), 0.25), (16, 16, 16), mp.origin, 0.2)
            still = run_device(flat, gtop.GtopInsert(push=push, push_below=below, **base), x, coeff, T, when=when)
            inside = ~out
            assert np.all(np.abs(still["info"][inside, 4] - 0.25) < 1e-15) and np.all(still["info"][:, 5] == 0)
            assert same_bits(still["x_out"], off["x_out"])
        finally:
            flat.close()
        # push > 0 without a field
        bare = gtop.GtopContext(device=0)
        try:
            guard = Guarded((B, 18), x.device)
            with pytest.raises(gtop.GtopError) as ei:
                insert.insert_waypoints_device(bare, gtop.GtopInsert(push=push, **base), x, coeff, T, when=when,
                                               x_out=guard.t)
            assert ei.value.code == ERR_STATE
            torch.cuda.synchronize()
            assert guard.untouched()
            insert.insert_waypoints_device(bare, gtop.GtopInsert(**base), x, coeff, T, when=when, x_out=guard.t)  # no push: no field needed
            torch.cuda.synchronize()
            assert same_bits(guard.t.cpu().numpy(), off["x_out"])
        finally:
            bare.close()
    finally:
        ctx.close()


def test_constant_velocity_known_answer_on_the_device(world, gtop):
    import torch
    mp, ctx = world
    xh, Dfh, Th, ch, when, _, _, _ = constant_velocity_row()
    dev = torch.device("cuda:0")
    got = run_device(ctx, gtop.GtopInsert(mode=it.AT_TIME, min_fraction=0.125), torch.tensor(xh[None], device=dev),
                     torch.tensor(ch.reshape(1, 5, 18), device=dev), torch.tensor(Th[None], device=dev),
                     when=torch.tensor([when], dtype=torch.float64, device=dev))
    check_constant_velocity(got["x_out"][0], got["T_out"][0], got["info"][0])


def test_host_form_equals_device_form_and_leaves_the_problem(world, gtop):
    import torch
    mp, ctx = world
    B, m = 33, 5
    b = problem.make_trajectories(B, m, mp, seed=9)
    ctx.set_problem(b.T, b.Df)
    lbh, ubh = ctx.default_bounds(b.waypoints)
    x, Df, T = _device_problem(b)
    coeff = ctx.coefficients_device(x, Df, T)
    wh = times_of_interest(b.T, np.random.default_rng(6))
    for opts, w in ((gtop.GtopInsert(mode=0, min_fraction=0.2), wh), (gtop.GtopInsert(mode=1), None)):
        dev_out = run_device(ctx, opts, x, coeff, T, when=None if w is None else torch.tensor(w, device=x.device),
                             lb=torch.tensor(lbh, device=x.device), ub=torch.tensor(ubh, device=x.device))
        host = dict(zip(("x_out", "T_out", "lb_out", "ub_out", "info"), insert.insert_waypoints(ctx, b.x, opts, when=w,
                                                                                                lb=lbh, ub=ubh)))
        for k in host:
            assert same_bits(host[k], dev_out[k]), k
        bare = insert.insert_waypoints(ctx, b.x[:7], opts, when=None if w is None else w[:7])     # a prefix, no bounds
        assert bare[2] is None and same_bits(bare[0], dev_out["x_out"][:7]) and same_bits(bare[4], dev_out["info"][:7])
        T_now, Df_now = ctx.get_problem()
        assert same_bits(T_now, b.T) and same_bits(Df_now, b.Df) and ctx.m == m
    ctx.set_problem(host["T_out"], b.Df)
    cost, grad = ctx.eval_batch(host["x_out"])
    assert cost.shape == (B,) and grad.shape == (B, 9 * m) and np.all(np.isfinite(cost)) and np.all(cost > 0)


def test_one_captured_graph_of_the_loop(world, gtop):
    """coefficients -> report -> insert (when = report + 2) -> coefficients (m + 1) -> report, captured once and
    replayed after the start point was changed in place: the eager run on the changed point, bit for bit."""
    import torch
    mp, ctx = world
    B, m, dt = 40, 6, 0.02
    b = problem.make_trajectories(B, m, mp, seed=12)
    x, Df, T = _device_problem(b)
    dev = x.device
    lim = gtop.GtopLimits(margin=0.3)
    opts = gtop.GtopInsert(mode=0, min_fraction=0.15)
    f64 = dict(dtype=torch.float64, device=dev)
    coeff, report = torch.empty(B, m, 18, **f64), torch.empty(B, 12, **f64)
    x2, T2, info = torch.empty(B, 9 * m, **f64), torch.empty(B, m + 1, **f64), torch.empty(B, 6, **f64)
    coeff2, report2 = torch.empty(B, m + 1, 18, **f64), torch.empty(B, 12, **f64)

    def loop():
        ctx.coefficients_device(x, Df, T, coeff=coeff)
        ctx.validate_device(coeff, T, lim, dt_sample=dt, report=report)
        insert.insert_waypoints_device(ctx, opts, x, coeff, T, when=report, when_column=2, x_out=x2, T_out=T2, info=info)
        ctx.coefficients_device(x2, Df, T2, coeff=coeff2)
        ctx.validate_device(coeff2, T2, lim, dt_sample=dt, report=report2)

    outputs = (coeff, report, x2, T2, info, coeff2, report2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        loop()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = [o.clone() for o in outputs]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop()
    x_new = torch.tensor(b.x + np.random.default_rng(13).normal(0.0, 0.2, b.x.shape), device=dev)
    x.copy_(x_new)
    for o in outputs:
        o.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outputs]
    loop()
    torch.cuda.synchronize()
    for r, e, f in zip(replayed, outputs, first):
        assert torch.equal(r.view(torch.int64), e.view(torch.int64))
    assert not torch.equal(replayed[2], first[2])
    # the same curve wherever it was cut: the report of the longer problem sees the old clearance (the coefficients of
    # the two new segments carry a few roundings of the waypoints' magnitude, far below 1e-9 m)
    r1, r2 = report.cpu().numpy(), report2.cpu().numpy()
    assert np.allclose(r2[:, 1], r1[:, 1], rtol=0, atol=1e-9) and np.allclose(r2[:, 11], r1[:, 11], rtol=1e-14, atol=0)
    assert set(info[:, 3].cpu().numpy()) == {0.0, 1.0}


def test_refusals_launch_nothing_and_an_empty_batch_is_accepted(world, gtop):
    import torch
    mp, ctx = world
    B, m = 5, 4
    b = problem.make_trajectories(B, m, mp, seed=21)
    x, Df, T = _device_problem(b)
    dev = x.device
    coeff = ctx.coefficients_device(x, Df, T)
    when = torch.tensor(0.5 * b.T.sum(axis=1), device=dev)
    lbh, ubh = ctx.default_bounds(b.waypoints)
    lb, ub = torch.tensor(lbh, device=dev), torch.tensor(ubh, device=dev)
    outs = {k: Guarded(shape, dev) for k, shape in (("x_out", (B, 9 * m)), ("T_out", (B, m + 1)), ("lb_out", (B, 9 * m)),
                                                    ("ub_out", (B, 9 * m)), ("info", (B, 6)))}
    L, h = ctx._L, ctx._h
    G = gtop.GtopInsert
    vp = lambda t: None if t is None else t.data_ptr()
    good = dict(o=G(mode=0), B_=B, m_=m, px=vp(x), pc=vp(coeff), pt=vp(T), stride=m, pw=vp(when), ws=1, plb=vp(lb),
                pub=vp(ub), pxo=vp(outs["x_out"].t), pto=vp(outs["T_out"].t), plo=vp(outs["lb_out"].t),
                puo=vp(outs["ub_out"].t), pi=vp(outs["info"].t))

    def call(**kw):
        a = dict(good, **kw)
        return L.gtop_insert_waypoints_device(h, a["o"], a["B_"], a["m_"], a["px"], a["pc"], a["pt"], a["stride"], a["pw"],
                                              a["ws"], a["plb"], a["pub"], a["pxo"], a["pto"], a["plo"], a["puo"], a["pi"],
                                              None)

    refused = [dict(o=None), dict(o=G(mode=2)), dict(o=G(mode=-1)), dict(o=G(mode=0, reserved=1)),
               dict(o=G(mode=0, min_fraction=0.0)), dict(o=G(mode=0, min_fraction=0.5000001)),
               dict(o=G(mode=0, min_fraction=-0.1)), dict(o=G(mode=0, min_fraction=np.nan)),
               dict(o=G(mode=0, push=np.inf)), dict(o=G(mode=0, push=np.nan)), dict(o=G(mode=0, push_below=-np.inf)),
               dict(o=G(mode=0, push_below=np.nan)),
               dict(o=G(mode=0, bos=-1.0)), dict(o=G(mode=0, vos=np.inf)), dict(o=G(mode=0, aos=np.nan)),
               dict(pub=None), dict(plb=None), dict(plo=None), dict(puo=None), dict(plo=None, puo=None),
               dict(plb=None, pub=None),                                    # outputs for bounds that are not given
               dict(B_=-1), dict(m_=1), dict(m_=227), dict(stride=m - 1), dict(stride=1), dict(ws=0), dict(ws=-8),
               dict(px=None), dict(pc=None), dict(pt=None), dict(pw=None), dict(pxo=None), dict(pto=None)]
    for kw in refused:
        assert call(**kw) == ERR_INVALID, kw
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs.values())
    # negative or non-finite bos / vos / aos are not read without bounds; when and when_stride not under LONGEST
    assert call(o=G(mode=0, bos=-1.0, vos=np.nan), plb=None, pub=None, plo=None, puo=None) == 0
    assert call(o=G(mode=1), pw=None, ws=0) == 0 and call(pi=None) == 0
    # B = 0: accepted, nothing launched, no buffer needed
    fresh = {k: Guarded(g.t.shape, dev) for k, g in outs.items()}
    f = {k: vp(g.t) for k, g in fresh.items()}
    empty = dict(B_=0, pxo=f["x_out"], pto=f["T_out"], plo=f["lb_out"], puo=f["ub_out"], pi=f["info"])
    assert call(**empty) == 0
    assert call(B_=0, px=None, pc=None, pt=None, pw=None, plb=None, pub=None, pxo=None, pto=None, plo=None, puo=None,
                pi=None) == 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in fresh.values())
    # the host form: no problem set is a state error, its own refusals are invalid arguments
    none = gtop.GtopContext(device=0)
    try:
        none.B, none.m = B, m
        with pytest.raises(gtop.GtopError) as ei:
            insert.insert_waypoints(none, b.x, G(mode=1))
        assert ei.value.code == ERR_STATE
    finally:
        none.close()
    ctx.set_problem(b.T, b.Df)
    for bad in (lambda: insert.insert_waypoints(ctx, b.x, G(mode=0)),                       # AT_TIME without when
                lambda: insert.insert_waypoints(ctx, b.x[:0], G(mode=1)),
                lambda: insert.insert_waypoints(ctx, np.tile(b.x, (2, 1)), G(mode=1)),       # more rows than the problem
                lambda: insert.insert_waypoints(ctx, b.x, G(mode=1, min_fraction=0.6))):
        with pytest.raises(gtop.GtopError) as ei:
            bad()
        assert ei.value.code == ERR_INVALID


def test_the_optimizer_runs_on_the_new_problem_inside_its_bounds(world, gtop):
    import torch
    mp, ctx = world
    B, m = 16, 5
    b = problem.make_trajectories(B, m, mp, seed=31)
    x, Df, T = _device_problem(b)
    dev = x.device
    lbh, ubh = ctx.default_bounds(b.waypoints)
    x0, _, _, _ = ctx.optimize_device_ex(x.clone(), Df, T, torch.tensor(lbh, device=dev), torch.tensor(ubh, device=dev), 10)
    coeff = ctx.coefficients_device(x0, Df, T)
    report = ctx.validate_device(coeff, T, gtop.GtopLimits(margin=0.3))
    x2, T2, lb2, ub2, info = insert.insert_waypoints_device(ctx, gtop.GtopInsert(mode=0, min_fraction=0.2), x0, coeff, T,
                                                            when=report, when_column=2, lb=torch.tensor(lbh, device=dev),
                                                            ub=torch.tensor(ubh, device=dev))
    start = torch.minimum(torch.maximum(x2, lb2), ub2)
    cost_start, _ = ctx.eval_device(start, Df, T2)
    torch.cuda.synchronize()
    assert torch.all(lb2 <= ub2).item() and torch.all(torch.isfinite(cost_start)).item()
    x_opt, cost, nev, code = ctx.optimize_device_ex(x2.clone(), Df, T2, lb2, ub2, 10)
    torch.cuda.synchronize()
    assert x_opt.shape == (B, 9 * m) and torch.all((x_opt >= lb2) & (x_opt <= ub2)).item()
    assert torch.all(cost <= cost_start).item(), (cost - cost_start).max().item()
    assert torch.all(nev >= 1).item()
