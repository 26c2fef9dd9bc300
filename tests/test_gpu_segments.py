"""The per-segment report and the segment-time reallocation on the device (gtop_validate_segments[_device],
gtop_reallocate_times[_device]; csrc/gtop_segments.hip, csrc/gtop_retime.hip) through the public Python wrapper.

(1) The laws include/gtop.h states between the segment report S and the whole-trajectory report R of the same inputs,
    bit for bit, every row, static and with boxes.
(2) Entries 0 .. 5 against the composition trajectory_samples + edt_query + the twin's segment of each sample
    (array_equal); entries 6 .. 9 against the twin's kinematics per segment at the project's derived bound
    (validate_twin.VEL_ACC_EPS eps of the sum of the absolute values of the derivative's terms).
(3) Both kinds of box list, a list longer than one LDS stage, the three start-time forms.
(4) The reallocation against the numpy twin (tests/segments_twin.py), array_equal; LENGTH against the path set-up and
    against exact arithmetic.
(5) What it is for: a rest-to-rest row stretched uniformly is the old curve flown slower.
(6) The entry points: host = device, one captured graph of the whole loop, refusals, B = 0."""
import decimal

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import segments_twin as st
from tests import validate_twin as vt
from tests.test_gpu_validate import MARGIN, _boxes, _device_problem, _scene, make_ctx, set_boxes, with_out_of_map_row

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
GRID = (48, 40, 24)
EPS = np.finfo(np.float64).eps
# name: (B, m, dt_sample, seed)
CASES = {"m2": (32, 2, 0.01, 41), "m6": (64, 6, 0.01, 7), "m13": (32, 13, 0.01, 21), "m40": (32, 40, 0.05, 33),
         "short": (32, 6, 0.01, 55)}


def _short_times(b):
    """Segment times below dt_sample in the rows of a six-segment batch.  The first segment lasts 1.003 s, so the
    samples at 1.00 and 1.01 s straddle whatever lies in [1.003, 1.0095]: single empty segments, a run of two, nearly
    everything short (every fourth row from row 3), and an empty last-but-one segment [2.803, 2.805]."""
    T = b.T.copy()
    T[:, 0] = 1.003
    T[0::4, 1] = 0.004
    T[1::4, 1:3] = (0.003, 0.0035)
    T[2::4, 1:5] = (0.5, 0.6, 0.7, 0.002)
    T[3::4, 1:5] = (0.002, 0.001, 0.002, 0.0015)
    return problem.Batch(b.waypoints, T, b.Df, b.x, b.m)


def _case(name):
    B, m, dt, seed = CASES[name]
    mp, b = _scene(GRID, 0.04, B, m, seed)
    if name == "short":
        b = _short_times(b)
    return mp, b, with_out_of_map_row(b, mp), dt


def composed_segments(ctx, mp, b, x, dt, margin, use_boxes, t0):
    """Entries 0 .. 5 of every row from the entry points the library had before: the stored samples, one edt_query over
    all of them at tau = t0[b] + eval_t (numpy's fp64 addition) or -1, the twin's segment of each sample, and numpy
    reductions; entries 6 .. 9 from the twin's kinematics, with their tolerances.  -> (exp (B, m, 10), tol (B, m, 4))"""
    B, m = len(x), b.m
    coeff, stats = ctx.trajectory_stats(x, dt)
    cap = int(stats[:, 8].max())
    _, samples = ctx.trajectory_samples(x, dt, cap)
    t0 = np.broadcast_to(np.float64(0.0) if t0 is None else np.asarray(t0, dtype=np.float64), (B,))
    kins = [vt.kinematics(coeff[i], b.T[i], dt) for i in range(B)]
    counts = np.array([len(k["t"]) for k in kins])
    assert np.array_equal(counts, stats[:, 8])
    pos = np.concatenate([samples[i, :counts[i]] for i in range(B)])
    tau = np.concatenate([(t0[i] + kins[i]["t"]) if use_boxes else np.full(counts[i], -1.0) for i in range(B)])
    dist, _ = ctx.edt_query(pos, tau)
    oom = vt.out_of_map(pos, mp.origin, mp.origin + mp.map_size)
    assert np.array_equal(dist == -1.0, oom)
    exp, tol = np.empty((B, m, st.N_SEG)), np.zeros((B, m, 4))
    o = 0
    for i in range(B):
        k, n = kins[i], counts[i]
        exp[i] = st.reduce_segments(m, k["t"], k["seg"], dist[o:o + n], oom[o:o + n], k["v"], k["a"], margin)
        for s in range(m):
            rows = k["seg"] == s
            if rows.any():
                tol[i, s] = vt.vel_acc_bounds(dict(sv=k["sv"][rows], sa=k["sa"][rows]), vt.VEL_ACC_EPS * EPS)
        o += n
    return exp, tol


def check_against_composition(S, exp, tol):
    bad = np.argwhere((S[:, :, :6] != exp[:, :, :6]).any(axis=2))
    assert bad.size == 0, (bad[:5], S[tuple(bad[0])], exp[tuple(bad[0])])
    err = np.abs(S[:, :, 6:] - exp[:, :, 6:])
    assert np.all(err <= tol), (np.argwhere(err > tol)[:5], err.max())
    print(f"entries 6..9: worst error / bound = {np.max(err[tol > 0] / tol[tol > 0]):.3g}")


def check_laws(S, R):
    for i in range(len(R)):
        assert st.check_laws(S[i], R[i]) == [], (i, S[i], R[i])


@pytest.fixture(scope="module", params=list(CASES))
def world(request, gtop):
    mp, b, be, dt = _case(request.param)
    ctx = make_ctx(gtop, mp)
    boxes = _boxes(b, np.random.default_rng(3), 8)
    yield request.param, mp, b, be, dt, ctx, boxes
    ctx.close()


def test_laws_and_composition_static_and_with_boxes(world, gtop):
    name, mp, b, be, dt, ctx, boxes = world
    B, m = len(b.x), b.m
    ctx.set_problem(be.T, be.Df)
    ctx.set_start_times(None)
    set_boxes(ctx, boxes)
    seen = {}
    for use_boxes in (0, 1):
        lim = gtop.GtopLimits(margin=MARGIN, use_boxes=use_boxes)
        R, _, _ = ctx.validate_batch(be.x, lim, dt_sample=dt)
        S = ctx.validate_segments(be.x, lim, dt_sample=dt)
        assert S.shape == (B + 1, m, 10)
        check_laws(S, R)
        exp, tol = composed_segments(ctx, mp, be, be.x, dt, MARGIN, use_boxes, None)
        check_against_composition(S, exp, tol)
        seen[use_boxes] = S
        full = S[:B, :, 0] > 0
        fails, passes = np.count_nonzero(S[:B, :, 4] > 0), np.count_nonzero(full & (S[:B, :, 4] == 0))
        print(f"{name} use_boxes={use_boxes}: {fails} segments fail the margin, {passes} pass, "
              f"{np.count_nonzero(~full)} without samples, longest {int(S[:, :, 0].max())} samples")
        assert fails > 0 and passes > 0                               # not vacuous
        assert S[B, :, 5].sum() > 0 and S[B, :, 2].min() == -1.0        # the constructed out-of-map row
    assert np.count_nonzero(seen[1][:B, :, 2] < seen[0][:B, :, 2]) > 0         # boxes lower some segment's clearance
    assert np.array_equal(seen[0][:, :, [0, 1, 6, 7, 8, 9]], seen[1][:, :, [0, 1, 6, 7, 8, 9]])
    S = seen[0]
    if name == "short":        # empty segments, a run of them, an empty last-but-one segment
        empty = S[:B, :, 0] == 0
        assert empty[0::4, 1].all() and empty[1::4, 1:3].all() and empty[2::4, 4].all() and empty[3::4, 1:5].all()
        assert np.array_equal(S[:B][empty], np.tile(st.EMPTY_ROW, (np.count_nonzero(empty), 1)))
    if name in ("m2", "m6"):
        assert S[:, :, 0].max() > 64           # a segment longer than one chunk of samples
    if name == "m40":
        assert np.median(S[:B, :, 0]) < 24     # several segments in every chunk of 64 samples


@pytest.mark.parametrize("kind", ["constant_velocity", "polynomial", "65_boxes", "polynomial_40_boxes"])
@pytest.mark.parametrize("t0_form", ["default", "shared", "per_row"])
def test_box_lists_and_start_time_forms(gtop, kind, t0_form):
    mp, b, be, dt = _case("m6")
    ctx = make_ctx(gtop, mp)
    n = len(be.x)
    rng = np.random.default_rng(12)
    try:
        ctx.set_problem(be.T, be.Df)
        nbox = {"constant_velocity": 8, "polynomial": 8, "65_boxes": 65, "polynomial_40_boxes": 40}[kind]
        p0, vel, scale = _boxes(b, rng, nbox)
        if nbox > 8:
            scale = 0.4 * scale                  # many boxes: smaller ones, so that rows keep some clearance
        if nbox == 65:                           # the last box stands on row 0's middle waypoint
            p0[64], vel[64], scale[64] = be.waypoints[0, (b.m + 1) // 2], 0.0, 0.8
        if kind.startswith("polynomial"):        # a quadratic prediction with a validity interval
            coef = np.zeros((nbox, 3, 6))
            coef[:, :, 0], coef[:, :, 1], coef[:, :, 2] = p0, vel, rng.uniform(-0.3, 0.3, (nbox, 3))
            ctx.set_moving_box_polynomials(coef, scale, np.tile([0.5, 3.5], (nbox, 1)))
        else:
            ctx.set_moving_boxes(p0, vel, scale)
        t0 = {"default": None, "shared": 1.375, "per_row": np.random.default_rng(5).uniform(0.0, 4.0, n)}[t0_form]
        ctx.set_start_times(t0)
        lim = gtop.GtopLimits(margin=MARGIN, use_boxes=1)
        R, _, _ = ctx.validate_batch(be.x, lim)
        S = ctx.validate_segments(be.x, lim)
        check_laws(S, R)
        exp, tol = composed_segments(ctx, mp, be, be.x, dt, MARGIN, 1, t0)
        check_against_composition(S, exp, tol)
        S0 = ctx.validate_segments(be.x, gtop.GtopLimits(margin=MARGIN, use_boxes=0))
        assert np.count_nonzero(S[:, :, 2] < S0[:, :, 2]) > 0
        if t0_form == "per_row":                 # a prefix of the problem's rows is served by the problem-sized list
            assert np.array_equal(ctx.validate_segments(be.x[:n // 2], lim), S[:n // 2])
        if nbox == 65:                           # the box behind the first stage decides a clearance
            ctx.set_moving_boxes(p0[:64], vel[:64], scale[:64])
            S64 = ctx.validate_segments(be.x, lim)
            assert np.all(S[:, :, 2] <= S64[:, :, 2]) and np.any(S[:, :, 2] < S64[:, :, 2])
    finally:
        ctx.close()


def test_signed_field_is_taken_as_it_is(gtop):
    mp, b, be, dt = _case("m6")
    ctx = make_ctx(gtop, mp, signed=1.0)
    try:
        ctx.set_problem(be.T, be.Df)
        lim = gtop.GtopLimits(margin=-0.05)
        R, _, _ = ctx.validate_batch(be.x, lim)
        S = ctx.validate_segments(be.x, lim)
        check_laws(S, R)
        assert np.count_nonzero(S[:-1, :, 2] < 0) > 0
    finally:
        ctx.close()


# ---- (4) the reallocation, exact ----
def _twin_limits(b, x, T, S, **kw):
    out = [st.retime_limits(b.m, x[i], T[i] if T.ndim == 2 else T, S[i], **kw) for i in range(len(x))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def test_limits_mode_is_the_twin_bit_for_bit(world, gtop):
    import torch
    name, mp, b, be, dt, ctx, boxes = world
    B, m = len(be.x), be.m
    ctx.set_problem(be.T, be.Df)
    ctx.set_start_times(None)
    set_boxes(ctx, None)
    x, Df, T = _device_problem(be)
    coeff = ctx.coefficients_device(x, Df, T)
    Sd = ctx.validate_segments_device(coeff, T, gtop.GtopLimits(margin=MARGIN), dt_sample=dt)
    torch.cuda.synchronize()
    S = Sd.cpu().numpy()
    # limits that bite on about half of the rows: medians of the rows' own largest figures (inputs, not tolerances)
    med = {pa: (np.median(S[:, :, 8 if pa else 6].max(axis=1)), np.median(S[:, :, 9 if pa else 7].max(axis=1)))
           for pa in (0, 1)}
    combos = 0
    for per_axis in (0, 1):
        for uniform in (0, 1):
            for scale_x in (0, 1):
                for vel_on, acc_on in ((1, 1), (1, 0), (0, 1), (0, 0)):
                    kw = dict(max_vel=med[per_axis][0] if vel_on else 0.0, max_acc=med[per_axis][1] if acc_on else -1.0,
                              per_axis=per_axis, uniform=uniform, scale_x=scale_x, max_ratio=1.02)
                    opt = gtop.GtopRetime(mode=gtop.GtopRetime.LIMITS, **kw)
                    xd = x.clone()
                    Td = ctx.reallocate_times_device(opt, x=xd, T=T, seg_report=Sd)
                    torch.cuda.synchronize()
                    T_want, x_want = _twin_limits(be, be.x, be.T, S, **kw)
                    assert np.array_equal(Td.cpu().numpy(), T_want), kw
                    assert np.array_equal(xd.cpu().numpy(), x_want), kw
                    kept = np.all(T_want == be.T, axis=1)
                    if vel_on or acc_on:
                        assert 0 < np.count_nonzero(kept) < B, kw            # rows within their limits, and rows beyond
                        assert np.any(T_want == 1.02 * be.T) or uniform        # max_ratio bites somewhere
                    else:
                        assert kept.all()
                    assert np.array_equal(xd.cpu().numpy()[kept], be.x[kept]) and np.all(T_want >= be.T)
                    combos += 1
    assert combos == 32
    # in place: T_out is T itself
    kw = dict(max_vel=med[0][0], max_acc=med[0][1], scale_x=1, max_ratio=2.0)
    opt = gtop.GtopRetime(mode=1, **kw)
    T_alias, xd = T.clone(), x.clone()
    out = ctx.reallocate_times_device(opt, x=xd, T=T_alias, seg_report=Sd, T_out=T_alias)
    torch.cuda.synchronize()
    T_want, x_want = _twin_limits(be, be.x, be.T, S, **kw)
    assert out.data_ptr() == T_alias.data_ptr() and np.array_equal(T_alias.cpu().numpy(), T_want)
    assert np.array_equal(xd.cpu().numpy(), x_want)
    # a shared time vector in, per-row times out
    T_sh = T[0].contiguous()
    coeff_sh = ctx.coefficients_device(x, Df, T_sh)
    S_sh = ctx.validate_segments_device(coeff_sh, T_sh, gtop.GtopLimits(margin=MARGIN), dt_sample=dt)
    out = ctx.reallocate_times_device(opt, x=x.clone(), T=T_sh, seg_report=S_sh)
    torch.cuda.synchronize()
    T_want, _ = _twin_limits(be, be.x, be.T[0], S_sh.cpu().numpy(), **kw)
    assert out.shape == (B, m) and np.array_equal(out.cpu().numpy(), T_want)
    assert len(np.unique(T_want, axis=0)) > 1 and torch.equal(T_sh, T[0])


def _exact_length_times(m, x, Df, mean_v, init_time):
    """LENGTH in exact arithmetic from the differences dx, dy, dz AS ROUNDED (one IEEE subtraction each, the same
    operation on the device and here): (T (m,), len / mean_v (m,)) as Decimals of 60 digits."""
    decimal.getcontext().prec = 60
    D = decimal.Decimal
    p = st.positions(m, x, Df)
    T, q = [], []
    for i in range(m):
        d = [D(float(np.float64(p[i, k] - p[i + 1, k]))) for k in range(3)]
        ln = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]).sqrt()
        q.append(ln / D(mean_v))
        T.append(q[-1] + (D(init_time) if i in (0, m - 1) else 0))
    return T, q


def test_length_mode(world, gtop):
    import torch
    name, mp, b, be, dt, ctx, boxes = world
    B, m = len(b.x), b.m
    dev = torch.device("cuda:0")
    mean_v, init_time = 1.8, 0.3
    opt = gtop.GtopRetime(mode=gtop.GtopRetime.LENGTH, mean_v=mean_v, init_time=init_time)
    # on the straight-line start of the path set-up: its T, but for init_time on the last segment as well
    T0, Df, x0 = ctx.setup_paths_device(torch.tensor(b.waypoints, device=dev), mean_v, init_time)
    Tl = ctx.reallocate_times_device(opt, x=x0, Df=Df)
    torch.cuda.synchronize()
    T0, Tl = T0.cpu().numpy(), Tl.cpu().numpy()
    assert np.array_equal(Tl[:, :m - 1], T0[:, :m - 1]) and np.array_equal(Tl[:, m - 1], T0[:, m - 1] + init_time)
    # the twin, bit for bit, on the batch's own (perturbed) x and on optimised x
    ctx.set_problem(b.T, b.Df)
    ctx.set_start_times(None)
    set_boxes(ctx, None)
    if name in ("m2", "m6"):
        lb, ub = ctx.default_bounds(b.waypoints)
        x_opt = ctx.optimize_batch_ex(b.x, lb, ub, 10)[0]
    else:           # (the other cases: moved waypoints without a solve)
        x_opt = b.x + np.random.default_rng(1).normal(0.0, 0.3, b.x.shape)
    assert np.abs(x_opt - b.x).max() > 1e-3 and np.all(np.isfinite(x_opt))
    u = EPS / 2
    worst = 0.0
    for x in (b.x, x_opt):
        xd, Dfd, _ = _device_problem(problem.Batch(b.waypoints, b.T, b.Df, x, m))
        Tl = ctx.reallocate_times_device(opt, x=xd, Df=Dfd).cpu().numpy()
        want = np.array([st.retime_length(m, x[i], b.Df[i], mean_v, init_time) for i in range(B)])
        assert np.array_equal(Tl, want)
        # Against exact arithmetic.  With s = dx^2 + dy^2 + dz^2 of the rounded differences: each square is rounded
        # once (relative u of its own term, so u of s in all: the terms are non-negative) and each of the two additions
        # once, at most 3u of s; the root halves that, 1.5u, and adds its own u; the quotient adds u: under 4u of
        # len / mean_v.  The addition of init_time rounds once more: u |T_out|.  (Second-order terms: u^2, far below.)
        for i in range(0, B, 5):
            exact, q = _exact_length_times(m, x[i], b.Df[i], mean_v, init_time)
            for s in range(m):
                err = abs(decimal.Decimal(float(Tl[i, s])) - exact[s])
                bound = decimal.Decimal(4 * u) * q[s] + decimal.Decimal(u) * decimal.Decimal(float(abs(Tl[i, s])))
                worst = max(worst, float(err / bound))
                assert err <= bound, (i, s, err, bound)
    print(f"{name}: LENGTH against exact arithmetic, worst error / bound = {worst:.3g}")


# ---- (5) what it is for ----
def test_uniform_stretch_of_rest_to_rest_rows_is_the_old_curve_flown_slower(gtop):
    """Rows with zero boundary velocity and acceleration, at the minimum-jerk start.  max_vel = 0.6 of the row's own
    largest per-axis speed, uniform = scale_x = 1: T' = lambda T, v' = v / lambda, a' = a / lambda^2, which is exactly
    p'(t) = p(t / lambda).  Sampling is the only gap between the two curves: the new samples see the old curve at
    other parameters, and a per-axis speed between two old samples exceeds the sampled maximum R[9] by at most
    A-bar dt_sample (A-bar: the bound of |a_k| over the old curve from its coefficients), so
        R'[9] <= (R[9] + A-bar dt) / lambda = max_vel + A-bar dt / lambda,
    plus rounding: the new coefficients are formed in fp64 from the scaled boundary values, with the cancellation of
    the waypoints' magnitude (up to 10 m) against segment lengths of a metre or two — a relative 1e-13 at the very
    most of the curve's own velocity scale V-bar; 1e-10 V-bar is taken."""
    import torch
    mp, b = _scene(GRID, 0.02, 32, 6, 77)
    dt = 0.01
    ctx = make_ctx(gtop, mp)
    try:
        assert not b.Df[:, :, [1, 2, 4, 5]].any()
        ctx.set_problem(b.T, b.Df)
        x_mj = ctx.min_jerk_start(b.x)
        lim = gtop.GtopLimits(margin=MARGIN)
        R, _, _ = ctx.validate_batch(x_mj, lim, dt_sample=dt)
        coeff_old, _ = ctx.trajectory_stats(x_mj, dt)
        xd, Df, T = _device_problem(problem.Batch(b.waypoints, b.T, b.Df, x_mj, b.m))
        Sd = ctx.validate_segments_device(ctx.coefficients_device(xd, Df, T), T, lim, dt_sample=dt)
        T_new = torch.empty_like(T)
        max_vel = 0.6 * R[:, 9]
        for i in range(len(b.x)):          # every row has its own limit: one launch per row
            opt = gtop.GtopRetime(mode=1, max_vel=max_vel[i], per_axis=1, uniform=1, scale_x=1, max_ratio=4.0)
            ctx.reallocate_times_device(opt, x=xd[i:i + 1], T=T[i:i + 1], seg_report=Sd[i:i + 1], T_out=T_new[i:i + 1])
        torch.cuda.synchronize()
        T_new, x_new = T_new.cpu().numpy(), xd.cpu().numpy()
        lam = T_new[:, 0] / b.T[:, 0]
        assert np.all(np.abs(lam - 1 / 0.6) < 1e-12) and np.allclose(T_new, lam[:, None] * b.T, rtol=1e-14, atol=0)
        ctx.set_problem(T_new, b.Df)
        R2, _, _ = ctx.validate_batch(x_new, lim, dt_sample=dt)
        checked = 0
        for i in range(len(b.x)):
            a_bar, v_bar = st.acc_bound(coeff_old[i], b.T[i]), st.vel_bound(coeff_old[i], b.T[i])
            assert R2[i, 9] <= max_vel[i] + a_bar * dt / lam[i] + 1e-10 * v_bar, (i, R2[i, 9], max_vel[i], a_bar)
            assert R2[i, 9] >= 0.9 * max_vel[i]             # and it is the same curve, not a slower one
            # clearance: a new sample sees the old curve within V dt of an old sample, V the bound of ||v||_2 over the
            # old curve (the norm over the axes of the per-axis bounds, at most sqrt(3) V-bar)
            if R[i, 1] > MARGIN + np.sqrt(3.0) * v_bar * dt:
                assert R2[i, 4] == 0, i
                checked += 1
        print(f"no new margin violation in {checked} rows with room to spare")
        assert checked >= 1, checked
    finally:
        ctx.close()


# ---- (6) the entry points ----
def test_host_forms_equal_device_forms(world, gtop):
    import torch
    name, mp, b, be, dt, ctx, boxes = world
    ctx.set_problem(be.T, be.Df)
    set_boxes(ctx, boxes)
    t0 = np.random.default_rng(9).uniform(0.0, 3.0, len(be.x))
    ctx.set_start_times(t0)
    try:
        lim = gtop.GtopLimits(margin=MARGIN, use_boxes=1)
        x, Df, T = _device_problem(be)
        Sd = ctx.validate_segments_device(ctx.coefficients_device(x, Df, T), T, lim, dt_sample=dt)
        torch.cuda.synchronize()
        S = ctx.validate_segments(be.x, lim, dt_sample=dt)
        assert np.array_equal(S, Sd.cpu().numpy())
        kw = dict(max_vel=np.median(S[:, :, 6].max(axis=1)), max_acc=np.median(S[:, :, 7].max(axis=1)), scale_x=1)
        opt = gtop.GtopRetime(mode=1, **kw)
        T_h, x_h = ctx.reallocate_times(be.x, opt, lim, dt_sample=dt)
        xd = x.clone()
        T_d = ctx.reallocate_times_device(opt, x=xd, T=T, seg_report=Sd)
        torch.cuda.synchronize()
        assert np.array_equal(T_h, T_d.cpu().numpy()) and np.array_equal(x_h, xd.cpu().numpy())
        assert np.any(T_h != be.T) and np.any(x_h != be.x)
        opt = gtop.GtopRetime(mode=0, mean_v=1.5, init_time=0.2)
        T_h, x_h = ctx.reallocate_times(be.x, opt)           # LENGTH needs neither limits nor dt_sample
        T_d = ctx.reallocate_times_device(opt, x=x, Df=Df)
        torch.cuda.synchronize()
        assert np.array_equal(T_h, T_d.cpu().numpy()) and np.array_equal(x_h, be.x)
        assert np.array_equal(ctx.get_problem()[0], be.T)     # the context's problem is not changed
        k = len(be.x) // 2                                    # a prefix of the problem's rows
        assert np.array_equal(ctx.reallocate_times(be.x[:k], opt)[0], T_h[:k])
    finally:
        ctx.set_start_times(None)


def test_one_graph_of_the_whole_loop_follows_start_times_and_boxes(gtop):
    """coefficients -> segment report -> reallocate -> optimise on the new times, captured once; replayed after the
    start times (a borrowed device buffer) and the box values changed, the report follows them."""
    import torch
    mp, b, be, dt = _case("m6")
    ctx = make_ctx(gtop, mp)
    try:
        n, m = len(b.x), b.m
        ctx.set_problem(b.T, b.Df)
        boxes = _boxes(b, np.random.default_rng(3), 8)
        set_boxes(ctx, boxes)
        x0, Df, T = _device_problem(b)
        t0 = torch.zeros(n, dtype=torch.float64, device=x0.device)
        ctx.set_start_times_device(t0)
        lim = gtop.GtopLimits(margin=MARGIN, use_boxes=1)
        lb, ub = (torch.tensor(a, device=x0.device) for a in ctx.default_bounds(b.waypoints))
        S0 = ctx.validate_segments(b.x, gtop.GtopLimits(margin=MARGIN))
        opt = gtop.GtopRetime(mode=1, max_vel=np.median(S0[:, :, 6].max(axis=1)), scale_x=1, max_ratio=2.0)
        x = x0.clone()
        coeff = torch.empty(n, m, 18, dtype=torch.float64, device=x.device)
        S = torch.zeros(n, m, 10, dtype=torch.float64, device=x.device)
        T_new = torch.zeros(n, m, dtype=torch.float64, device=x.device)

        def loop():
            ctx.coefficients_device(x, Df, T, coeff=coeff)
            ctx.validate_segments_device(coeff, T, lim, dt_sample=dt, seg_report=S)
            ctx.reallocate_times_device(opt, x=x, T=T, seg_report=S, T_out=T_new)
            return ctx.optimize_device_ex(x, Df, T_new, lb, ub, 5)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # an eager pass sizes the optimizer's workspace
            x_e, c_e, _, _ = loop()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        x_eager, c_eager, S_eager, T_eager = x_e.clone(), c_e.clone(), S.clone(), T_new.clone()
        graph = torch.cuda.CUDAGraph()
        x.copy_(x0)
        with torch.cuda.graph(graph):
            x_g, c_g, _, _ = loop()
        x.copy_(x0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(S, S_eager) and torch.equal(T_new, T_eager)
        assert torch.equal(x_g, x_eager) and torch.equal(c_g, c_eager)
        exp, tol = composed_segments(ctx, mp, b, b.x, dt, MARGIN, 1, None)
        first = S.cpu().numpy().copy()
        check_against_composition(first, exp, tol)
        T_want, x_want = _twin_limits(b, b.x, b.T, first, max_vel=opt.max_vel, scale_x=1, max_ratio=2.0)
        assert np.array_equal(T_new.cpu().numpy(), T_want)
        # new start times in the borrowed buffer, new boxes in the context's (same address, same count)
        t0_new = np.random.default_rng(8).uniform(0.5, 3.0, n)
        t0.copy_(torch.tensor(t0_new, device=x.device))
        set_boxes(ctx, _boxes(b, np.random.default_rng(4), 8))
        x.copy_(x0)
        graph.replay()
        torch.cuda.synchronize()
        second = S.cpu().numpy().copy()
        exp2, tol2 = composed_segments(ctx, mp, b, b.x, dt, MARGIN, 1, t0_new)
        check_against_composition(second, exp2, tol2)
        assert not np.array_equal(first[:, :, 2], second[:, :, 2])
    finally:
        ctx.set_start_times_device(None)
        ctx.close()


def test_refusals_launch_nothing_and_an_empty_batch_is_accepted(gtop):
    import torch
    mp, b, be, dt = _case("m6")
    ctx = make_ctx(gtop, mp)
    try:
        n, m = len(b.x), b.m
        ctx.set_problem(b.T, b.Df)
        x, Df, T = _device_problem(b)
        keep_x = x.clone()
        coeff = ctx.coefficients_device(x, Df, T)
        sentinel = -12345.0
        S = torch.full((n, m, 10), sentinel, dtype=torch.float64, device=x.device)
        T_out = torch.full((n, m), sentinel, dtype=torch.float64, device=x.device)
        good = gtop.GtopLimits(margin=MARGIN)
        S_ok = ctx.validate_segments_device(coeff, T, good)
        L, h = ctx._L, ctx._h

        def refused(code, fn):
            with pytest.raises(gtop.GtopError) as ei:
                fn()
            assert ei.value.code == code, ei.value

        # the segment report: the report's own refusals
        refused(ERR_INVALID, lambda: ctx.validate_segments_device(coeff, T, good, dt_sample=0.0, seg_report=S))
        refused(ERR_INVALID, lambda: ctx.validate_segments(b.x, good, dt_sample=-0.01))
        for bad in (dict(margin=np.nan), dict(margin=np.inf), dict(max_vel=np.inf), dict(max_acc=np.nan)):
            refused(ERR_INVALID, lambda: ctx.validate_segments_device(coeff, T, gtop.GtopLimits(**bad), seg_report=S))
            refused(ERR_INVALID, lambda: ctx.validate_segments(b.x, gtop.GtopLimits(**bad)))
        ctx.set_start_times(np.linspace(0.0, 1.0, n + 3))            # neither 0, 1 nor B
        refused(ERR_INVALID, lambda: ctx.validate_segments_device(coeff, T, good, seg_report=S))
        refused(ERR_INVALID, lambda: ctx.validate_segments(b.x, good))
        lim_opt = gtop.GtopRetime(mode=1, max_vel=1.0)
        refused(ERR_INVALID, lambda: ctx.reallocate_times(b.x, lim_opt, good))
        ctx.set_start_times(None)
        vp = lambda t: None if t is None else t.data_ptr()
        assert L.gtop_validate_segments_device(h, n, m, None, vp(T), m, 0.01, good, vp(S), None) == ERR_INVALID
        assert L.gtop_validate_segments_device(h, n, m, vp(coeff), vp(T), m, 0.01, good, None, None) == ERR_INVALID
        assert L.gtop_validate_segments_device(h, -1, m, vp(coeff), vp(T), m, 0.01, good, vp(S), None) == ERR_INVALID
        assert L.gtop_validate_segments_device(h, n, m, vp(coeff), vp(T), m - 1, 0.01, good, vp(S), None) == ERR_INVALID
        refused(ERR_INVALID, lambda: ctx.validate_segments(b.x[:0], good))
        # the reallocation
        R = gtop.GtopRetime
        call = lambda o, B_=n, m_=m, px=vp(x), pd=vp(Df), pt=vp(T), stride=m, ps=vp(S_ok), po=vp(T_out): \
            L.gtop_reallocate_times_device(h, o, B_, m_, px, pd, pt, stride, ps, po, None)
        assert call(None) == ERR_INVALID
        for o in (R(mode=2), R(mode=-1), R(mode=0, mean_v=0.0), R(mode=0, mean_v=np.inf), R(mode=0, mean_v=np.nan),
                  R(mode=0, init_time=-0.1), R(mode=0, init_time=np.inf), R(mode=1, max_ratio=0.99),
                  R(mode=1, max_ratio=np.inf), R(mode=1, max_ratio=np.nan)):
            assert call(o) == ERR_INVALID, (o.mode, o.mean_v, o.init_time, o.max_ratio)
            refused(ERR_INVALID, lambda: ctx.reallocate_times(b.x, o, good))
        length, limits = R(mode=0), R(mode=1, max_vel=1.0, scale_x=1)
        for o in (length, limits):
            assert call(o, B_=-1) == ERR_INVALID and call(o, m_=1) == ERR_INVALID and call(o, m_=228) == ERR_INVALID
            assert call(o, stride=m - 1) == ERR_INVALID and call(o, po=None) == ERR_INVALID
        assert call(length, px=None) == ERR_INVALID and call(length, pd=None) == ERR_INVALID
        assert call(limits, pt=None) == ERR_INVALID and call(limits, ps=None) == ERR_INVALID
        assert call(limits, px=None) == ERR_INVALID                    # scale_x needs x
        assert call(limits, pt=vp(T_out), stride=0) == ERR_INVALID     # a shared vector cannot be its own output
        refused(ERR_INVALID, lambda: ctx.reallocate_times(b.x[:0], length))
        fresh = gtop.GtopContext(device=0)                            # no field, no problem
        try:
            refused(ERR_STATE, lambda: fresh.validate_segments_device(coeff, T, good, seg_report=S))
            fresh.B, fresh.m = n, m
            refused(ERR_STATE, lambda: fresh.validate_segments(b.x, good))
            refused(ERR_STATE, lambda: fresh.reallocate_times(b.x, length))
        finally:
            fresh.close()
        # B = 0: accepted, nothing launched
        empty = torch.empty(0, m, 18, dtype=torch.float64, device=x.device)
        ctx.validate_segments_device(empty, T[:0], good, seg_report=S[:0])
        assert call(length, B_=0) == 0 and call(limits, B_=0) == 0
        assert call(length, B_=0, px=None, pd=None, po=None) == 0
        torch.cuda.synchronize()
        assert torch.all(S == sentinel).item() and torch.all(T_out == sentinel).item() and torch.equal(x, keep_x)
        # what is allowed: LENGTH without T and seg_report, LIMITS without Df, and without x when scale_x is off
        assert call(length, pt=None, ps=None) == 0
        assert call(R(mode=1, max_vel=1.0), px=None, pd=None) == 0
        torch.cuda.synchronize()
        assert not torch.any(T_out == sentinel).item() and torch.equal(x, keep_x)
    finally:
        ctx.close()
