"""include/gtop_time_moving.h on the GPU: the segment-time gradient under the moving-obstacle cost against the
evaluation's cost and against the numpy twin (tests/time_moving_twin.py) on the library's own field, gt0 against central
differences of the library's own cost in the start time, the bit-level laws, the special rows, the optimizer against its
laws and the twin's run, one captured graph of the whole cycle, the refusals and the host forms.

Criterion and tolerance of the comparisons: tests/test_gpu_time.py's — scenes.rel_err at 1e-5, the project's fp64
parity bound, which covers a sample whose float rounding falls differently.

That criterion is normwise and, in a batch of more than six rows, looks at six of them (the twins are pure-Python loops).  Every row and every entry — the cost, each gT_s, each parts column, gt0, q_s and R_s — is held at rounding-error level by
tests/test_gpu_time_entrywise.py against tests/time_entry_ref.py (whose magnitudes tests/test_time_entrywise_bound.py holds
against 40-digit arithmetic)."""
import ctypes as C

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import scenes
from tests import time_moving_twin as tm
from tests.test_gpu_time import DYN, ERR_INVALID, ERR_STATE, GUARD, OPT, _batch, _dev, _field
from tests.test_time_moving_twin import (ANALYTIC, GT0_H, _waypoint, aimed, analytic_case, analytic_parts, gt0_case,
                                         lookup_of)

pytestmark = pytest.mark.gpu
TOL = 1e-5
NONE3 = np.zeros((0, 3))


@pytest.fixture(scope="module")
def scene(gtop, oracle_mod):
    mp = problem.make_map((60, 50, 30), density=0.03, seed=11)
    ctx, sdf = _field(gtop, oracle_mod, mp)
    yield mp, ctx, sdf
    ctx.close()


def _clear(ctx):
    ctx.set_moving_cost(False)
    ctx.set_moving_boxes(NONE3, NONE3, NONE3)
    ctx.set_start_times(None)


def set_boxes(ctx, bx):
    if bx["poly"]:
        ctx.set_moving_box_polynomials(bx["coef"], bx["scale"], bx["t_range"])
    else:
        ctx.set_moving_boxes(bx["p0"], bx["vel"], bx["scale"])


def _gradient(gtop, ctx, b, T, **kw):
    import torch
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    out = gtop.time_gradient_moving_device(ctx, x, Df, Tt, **kw)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in out]


def _laws(c, g, g0, p):
    """gT == ([2] + [3]) + [5]; [5] and gt0 are the stated sums of [4]; the parts sum to the cost."""
    assert np.array_equal(g, (p[:, :, 2] + p[:, :, 3]) + p[:, :, 5])
    R = np.zeros(p.shape[0])
    for s in range(p.shape[1] - 1, -1, -1):
        assert np.array_equal(p[:, s, 5], R)
        R = R + p[:, s, 4]
    assert np.array_equal(g0, R)
    assert np.max(np.abs((p[:, :, 0].sum(1) + p[:, :, 1].sum(1) + 1e-3) - c) / np.abs(c)) <= 1e-12


@pytest.mark.parametrize("B,m,poly,nbox,per_row,mode", [
    (3, 2, False, 1, False, "plain"), (65, 7, True, 32, True, "plain"), (5, 13, False, 32, True, "dyn"),
    (2, 227, True, 1, False, "plain"), (5, 13, True, 1, True, "step1"), (5, 13, False, 1, False, "signed"),
    (65, 7, False, 32, False, "dyn"), (3, 2, True, 32, True, "plain"), (5, 13, True, 32, False, "signed")])
def test_gradient_against_the_evaluation_and_the_twin(gtop, oracle_mod, scene, B, m, poly, nbox, per_row, mode):
    """A partial last workgroup, an odd m, the LDS limit; lists of 1 and 32 boxes of both kinds; shared and per-row
    start times; plain, dyn, step 1 and the signed field."""
    import torch
    mp, ctx, sdf = scene
    if mode == "signed":
        ctx, sdf = _field(gtop, oracle_mod, mp, signed=True)
        assert ctx.field_sign()[0] and sdf.dist.min() < 0.0
    extra = {"plain": {}, "signed": dict(ws=0.0), "dyn": DYN, "step1": dict(DYN, step=1)}[mode]
    params = dict(gtop.OPTI_NODE_PARAMS, **extra)
    b, T = _batch(B, m, mp, 7100 + 17 * m + B + nbox)
    rows = np.arange(B) if B <= 6 else np.r_[0:3, B - 3:B]
    t0 = np.linspace(0.2, 1.4, B) if per_row else 0.6
    b, bx = aimed(b, T, t0, rows, nbox, poly, 7200 + m + nbox)
    try:
        ctx.set_params(**extra)
        set_boxes(ctx, bx)
        ctx.set_moving_cost(True)
        ctx.set_start_times(t0)
        c, g, g0, p = _gradient(gtop, ctx, b, T, want_parts=True)
        ce, _ = ctx.eval_device(*_dev(b.x, b.Df.reshape(-1, 18), T))
        torch.cuda.synchronize()
    finally:
        ctx.set_params()
        _clear(ctx)
    ce = ce.cpu().numpy()
    r_eval = float(np.max(np.abs(c - ce) / np.abs(ce)))
    t0b = np.broadcast_to(t0, (B,))
    c_ref, g_ref, g0_ref, p_ref, low = tm.gradient_batch(T[rows], b.Df[rows], b.x[rows], lookup_of(sdf, bx), params, t0b[rows])
    rc, rg = scenes.rel_err(c[rows], g[rows], c_ref, g_ref)
    _, rp = scenes.rel_err(c[rows], p[rows], c_ref, p_ref)
    r0 = float(np.max(np.abs(g0[rows] - g0_ref)) / max(np.max(np.abs(g0_ref)), 1e-300))
    # the smoothness columns are orders of magnitude above the rest: every column against its own max-norm as well
    rcol = max(float(np.max(np.abs(p[rows][:, :, k] - p_ref[:, :, k])) / max(np.max(np.abs(p_ref[:, :, k])), 1e-300))
               for k in range(6))
    later = low[:, 1:].any(axis=1)
    print(f"B={B} m={m} {'poly' if poly else 'const-vel'} x{nbox} {mode}: cost against eval_device {r_eval:.2e}; against "
          f"the twin cost {rc:.2e} gT {rg:.2e} gt0 {r0:.2e} parts {rp:.2e}, column by column {rcol:.2e}; {later.sum()} of "
          f"{len(rows)} twin rows lowered in a later segment; max |[5]| / max |gT| "
          f"{np.max(np.abs(p[:, :, 5])) / np.max(np.abs(g)):.2e}")
    assert later.mean() >= 0.25
    assert r_eval <= TOL and rc <= TOL and rg <= TOL and rp <= TOL and r0 <= TOL and rcol <= TOL
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(g)) and np.all(np.isfinite(p)) and np.all(np.isfinite(g0))
    assert np.any(p[:, :, 4] != 0.0) and np.any(p[:, :, 5] != 0.0)
    _laws(c, g, g0, p)
    if mode == "signed":
        ctx.close()


def test_gt0_against_the_librarys_own_cost(gtop, scene):
    """Central differences of eval_device's cost in the start time (positions do not depend on t0: no float round trip
    interferes), h = GT0_H: within 1e-5 of the max-norm.  The same quotient on the twin, for these rows, stays under a
    quarter of that (tests/test_time_moving_twin.py, tests/golden/TIME_MOVING_ANALYTIC.md)."""
    import torch
    mp, ctx, sdf = scene
    b, T, t0, bx = gt0_case(mp)
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    t0d = _dev(t0)[0]
    try:
        set_boxes(ctx, bx)
        ctx.set_moving_cost(True)
        ctx.set_start_times_device(t0d)
        _, _, g0, _ = gtop.time_gradient_moving_device(ctx, x, Df, Tt)
        torch.cuda.synchronize()
        t0d += GT0_H
        cp = ctx.eval_device(x, Df, Tt)[0].clone()
        torch.cuda.synchronize()
        t0d -= 2 * GT0_H
        cm = ctx.eval_device(x, Df, Tt)[0].clone()
        torch.cuda.synchronize()
    finally:
        _clear(ctx)
    fd = ((cp - cm) / (2 * GT0_H)).cpu().numpy()
    g0 = g0.cpu().numpy()
    dev = np.max(np.abs(g0 - fd)) / np.max(np.abs(fd))
    print(f"gt0 against central differences of eval_device in t0 (h = {GT0_H}): off by {dev:.2e} of the max-norm "
          f"{np.max(np.abs(fd)):.3e}")
    assert np.all(fd != 0.0) and dev <= 1e-5, dev


def _run(gtop, ctx, x, Df, Tt, parts=True, gt0=True):
    """One guarded launch -> [cost, gT, gt0, parts] (clones); guard words stay, an output not given stays untouched."""
    import torch
    Bq, m = x.shape[0], Tt.shape[-1]
    bufs = [torch.full((n + 16,), GUARD, dtype=torch.float64, device="cuda:0") for n in (Bq, Bq * m, Bq, Bq * m * 6)]
    views = [bufs[0][8:8 + Bq], bufs[1][8:8 + Bq * m].view(Bq, m), bufs[2][8:8 + Bq], bufs[3][8:8 + Bq * m * 6].view(Bq, m, 6)]
    gtop.time_gradient_moving_device(ctx, x, Df, Tt, cost=views[0], gT=views[1], gt0=views[2] if gt0 else None,
                                     parts=views[3] if parts else None, want_gt0=False)
    torch.cuda.synchronize()
    for buf in bufs:
        assert torch.all(buf[:8] == GUARD) and torch.all(buf[-8:] == GUARD)
    if not parts:
        assert torch.all(bufs[3] == GUARD)
    if not gt0:
        assert torch.all(bufs[2] == GUARD)
    return [v.clone() for v in views]


def _special_rows(mp):
    """Row 1 leaves the map, row 2 has a segment of 0.02 s on the replay path, and (with special_boxes) a box covers
    samples of row 3: dist = 0 there, and the corner derivative 0."""
    b, T = _batch(4, 5, mp, 4200)
    T = T.copy()
    x = b.x.reshape(4, 3, -1).copy()
    x[1, 2, 3] = mp.origin[2] + mp.map_size[2] + 1.5            # waypoint 2 of row 1: z above the map
    T[2, 2] = 0.02
    return problem.Batch(b.waypoints, T, b.Df, x.reshape(4, -1), 5), T


def special_boxes(b, T, t0):
    """Box 0 covers waypoint 2 of row 3 when the row is there (1.6 m wide, drifting slowly); boxes 1 .. 3 pass the
    waypoints 3 of rows 0 .. 2."""
    p_at = np.stack([_waypoint(b, 3, 2)] + [_waypoint(b, r, 3) + 0.1 for r in range(3)])
    when = np.array([t0 + T[3, :2].sum()] + [t0 + T[r, :3].sum() for r in range(3)])
    vel = np.array([[0.05, -0.04, 0.02], [0.4, -0.3, 0.1], [-0.35, 0.2, 0.1], [0.3, 0.3, -0.1]])
    scale = np.array([[1.6, 1.6, 1.6], [0.8, 0.6, 0.7], [0.6, 0.9, 0.5], [0.7, 0.7, 0.7]])
    return dict(poly=False, p0=p_at - vel * when[:, None], vel=vel, scale=scale)


def test_special_rows(gtop, scene):
    """A row that leaves the map, a 0.02 s segment on the replay path, a row whose samples a box covers."""
    import torch
    mp, ctx, sdf = scene
    b, T = _special_rows(mp)
    t0 = 0.5
    bx = special_boxes(b, T, t0)
    try:
        set_boxes(ctx, bx)
        ctx.set_moving_cost(True)
        ctx.set_start_times(t0)
        c, g, g0, p = _gradient(gtop, ctx, b, T, want_parts=True)
        ce, _ = ctx.eval_device(*_dev(b.x, b.Df.reshape(-1, 18), T))
        torch.cuda.synchronize()
    finally:
        _clear(ctx)
    assert np.max(np.abs(c - ce.cpu().numpy()) / np.abs(c)) <= TOL
    look = lookup_of(sdf, bx)
    c_ref, g_ref, g0_ref, p_ref, low = tm.gradient_batch(T, b.Df, b.x, look, dict(gtop.OPTI_NODE_PARAMS), np.full(4, t0))
    rc, rg = scenes.rel_err(c, g, c_ref, g_ref)
    _, rp = scenes.rel_err(c, p, c_ref, p_ref)
    r0 = float(np.max(np.abs(g0 - g0_ref)) / np.max(np.abs(g0_ref)))
    print(f"special rows against the twin: cost {rc:.2e} gT {rg:.2e} gt0 {r0:.2e} parts {rp:.2e}")
    assert rc <= TOL and rg <= TOL and rp <= TOL and r0 <= TOL and low.any(axis=1).all()
    _laws(c, g, g0, p)
    # the covered sample: the waypoint itself is inside box 0 at its time — dist 0, every corner derivative 0
    d, _, dtau = look.query(_waypoint(b, 3, 2), t0 + T[3, :2].sum())
    assert d == 0.0 and dtau == 0.0 and look.lowered and np.all(look.dcorner == 0.0)


def test_bit_level_laws(gtop, scene):
    """Mode off, on without boxes, every t0 < -sum T: gtop_time_gradient_device's bits and zeros beside them; boxes at
    rest: [4] = [5] = gt0 = 0; a row's bits do not depend on B, its place or time_stride; parts or gt0 NULL change
    nothing else; one derivative under both gradient modes; a NaN row disturbs only itself; guard words stay."""
    import torch
    mp, ctx, sdf = scene
    b, T = _special_rows(mp)
    B, m = 4, 5
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    bx = special_boxes(b, T, 0.5)
    cs, gs, ps = gtop.time_gradient_device(ctx, x, Df, Tt, want_parts=True)
    torch.cuda.synchronize()

    def is_static(out):
        assert torch.equal(out[0], cs) and torch.equal(out[1], gs) and torch.equal(out[3][:, :, :4], ps)
        assert torch.all(out[3][:, :, 4:] == 0.0) and torch.all(out[2] == 0.0)

    try:
        is_static(_run(gtop, ctx, x, Df, Tt))                          # mode off, no boxes
        set_boxes(ctx, bx)
        is_static(_run(gtop, ctx, x, Df, Tt))                          # mode off, boxes set
        ctx.set_moving_boxes(NONE3, NONE3, NONE3)
        ctx.set_moving_cost(True)
        is_static(_run(gtop, ctx, x, Df, Tt))                          # mode on, no boxes
        set_boxes(ctx, bx)
        before = _dev(np.full(B, -(T.sum(1).max() + 1.0)))[0]
        ctx.set_start_times_device(before)                             # every sample before the boxes' clock starts
        is_static(_run(gtop, ctx, x, Df, Tt))
        ctx.set_start_times(0.5)
        ctx.set_moving_boxes(bx["p0"] + 0.5 * bx["vel"], np.zeros_like(bx["vel"]), bx["scale"])   # boxes at rest
        rest = _run(gtop, ctx, x, Df, Tt)
        assert torch.all(rest[3][:, :, 4:] == 0.0) and torch.all(rest[2] == 0.0)
        assert not torch.equal(rest[0], cs)                            # (they are in the field all the same)
        set_boxes(ctx, bx)
        base = _run(gtop, ctx, x, Df, Tt)
        assert not any(bool(torch.any(t == GUARD)) for t in base)
        assert torch.any(base[3][:, :, 4] != 0.0) and torch.any(base[2] != 0.0)
        _laws(*[t.cpu().numpy() for t in base])
        try:
            ctx.set_gradient_mode(True)
            cons = _run(gtop, ctx, x, Df, Tt)
        finally:
            ctx.set_gradient_mode(False)
        assert all(torch.equal(a, c) for a, c in zip(base, cons))
        nop = _run(gtop, ctx, x, Df, Tt, parts=False)
        assert all(torch.equal(nop[k], base[k]) for k in range(3))
        nog = _run(gtop, ctx, x, Df, Tt, gt0=False)
        assert all(torch.equal(nog[k], base[k]) for k in (0, 1, 3))
        # row 3 alone, first, last, in a batch of 130 — and with its times shared through stride 0
        r = 3
        alone = _run(gtop, ctx, x[r:r + 1].contiguous(), Df[r:r + 1].contiguous(), Tt[r:r + 1].contiguous())
        shared = _run(gtop, ctx, x[r:r + 1].contiguous(), Df[r:r + 1].contiguous(), Tt[r].contiguous())
        big, _ = _batch(130, m, mp, 4300)
        for place in (0, 129, 77):
            xb, Dfb, Tb = _dev(big.x, big.Df.reshape(-1, 18), big.T)
            xb[place], Dfb[place], Tb[place] = x[r], Df[r], Tt[r]
            got = _run(gtop, ctx, xb, Dfb, Tb)
            for k in range(4):
                assert torch.equal(got[k][place], base[k][r]), (place, k)
        for k in range(4):
            assert torch.equal(alone[k][0], base[k][r]) and torch.equal(shared[k][0], base[k][r])
        # a NaN row and a T = 0 row: the launch returns, the other rows keep their bits
        xn, Tn = x.clone(), Tt.clone()
        xn[3, 4] = float("nan")
        Tn[0, 1] = 0.0
        bad = _run(gtop, ctx, xn, Df, Tn)
        for k in range(4):
            assert torch.equal(bad[k][1:3], base[k][1:3])
    finally:
        _clear(ctx)


def _optimize(gtop, ctx, b, T, opts, T_lo=None):
    import torch
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    B, m = b.x.shape[0], b.m
    bufs = [torch.full((n + 16,), GUARD, dtype=torch.float64, device="cuda:0") for n in (B * m, B * 8)]
    T_out, info = bufs[0][8:8 + B * m].view(B, m), bufs[1][8:8 + B * 8].view(B, 8)
    lo = None if T_lo is None else _dev(T_lo)[0]
    gtop.optimize_times_moving_device(ctx, gtop.GtopTimeOpt(**opts), x, Df, Tt, T_lo=lo, T_out=T_out, info=info)
    torch.cuda.synchronize()
    for buf in bufs:
        assert torch.all(buf[:8] == GUARD) and torch.all(buf[-8:] == GUARD)
    return T_out.clone(), info.clone()


@pytest.mark.parametrize("B,m,poly,nbox", [(3, 2, False, 1), (65, 7, True, 32), (5, 13, False, 32), (2, 227, True, 1)])
def test_optimizer_laws(gtop, scene, B, m, poly, nbox):
    """F never rises, the bounds hold exactly with and without T_lo (the LIMITS reallocation's output), info[5] is the
    gradient entry's cost at T_out bit for bit, info[7] the sum of T_out, and the host forms give the device forms' bits."""
    import torch
    mp, ctx, sdf = scene
    b, T = _batch(B, m, mp, 8100 + m + B)
    rows = np.arange(B) if B <= 6 else np.r_[0:3, B - 3:B]
    t0 = np.linspace(0.1, 0.9, B)
    b, bx = aimed(b, T, t0, rows, nbox, poly, 8200 + m)
    opts = dict(OPT, t_min=0.0301 if m > 100 else 0.1, max_evals=12)
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    coeff = ctx.coefficients_device(x, Df, Tt)
    seg = ctx.validate_segments_device(coeff, Tt, gtop.GtopLimits())
    T_lim = ctx.reallocate_times_device(gtop.GtopRetime(mode=gtop.GtopRetime.LIMITS, max_vel=1.5, max_acc=2.0), T=Tt,
                                        seg_report=seg)
    torch.cuda.synchronize()
    T_lo = T_lim.cpu().numpy().copy()
    assert np.any(T_lo > T)
    T_lo[:, 0] = 0.01
    T_lo[:, 1] = opts["t_max"] + 1.0
    try:
        set_boxes(ctx, bx)
        ctx.set_moving_cost(True)
        ctx.set_start_times(t0)
        for lo in (None, T_lo):
            T_out, info = _optimize(gtop, ctx, b, T, opts, lo)
            To, io = T_out.cpu().numpy(), info.cpu().numpy()
            assert np.all(np.isfinite(To)) and np.all(np.isfinite(io))
            assert np.all(io[:, 4] <= io[:, 3])                                   # F_out <= F_in
            assert np.all(np.isin(io[:, 0], (3, 4, 5))) and np.all(io[:, 2] >= 1) and np.all(io[:, 2] <= opts["max_evals"])
            assert np.all(io[:, 1] <= io[:, 2] - 1) and np.all(io[:, 6] >= 0)
            lob = np.full_like(To, opts["t_min"]) if lo is None else np.maximum(opts["t_min"], lo)
            pinned = lob > opts["t_max"]
            assert np.array_equal(To[pinned], lob[pinned])
            assert np.all(To[~pinned] >= lob[~pinned]) and np.all(To[~pinned] <= opts["t_max"])
            c, _, _, _ = gtop.time_gradient_moving_device(ctx, x, Df, T_out)
            torch.cuda.synchronize()
            assert torch.equal(c, info[:, 5])                                      # bit for bit
            assert np.max(np.abs(io[:, 4] - (io[:, 5] + opts["rho"] * To.sum(1))) / np.abs(io[:, 4])) <= 1e-13
            assert np.max(np.abs(io[:, 7] - To.sum(1)) / To.sum(1)) <= 1e-14
            assert np.any(io[:, 1] >= 1)                                           # something moved
        # the host forms: the same bits (the per-row start times serve the problem's first rows)
        ctx.set_problem(T, b.Df)
        Bh = min(B, 9)
        Th, ih = gtop.optimize_times_moving(ctx, gtop.GtopTimeOpt(**opts), b.x[:Bh], T_lo[:Bh])
        assert np.array_equal(Th, To[:Bh]) and np.array_equal(ih, io[:Bh])
        ch, gh, g0h, ph = gtop.time_gradient_moving_batch(ctx, b.x[:Bh])
        cd, gd, g0d, pd = _gradient(gtop, ctx, b, T, want_parts=True)
        assert np.array_equal(ch, cd[:Bh]) and np.array_equal(gh, gd[:Bh]) and np.array_equal(ph, pd[:Bh])
        assert np.array_equal(g0h, g0d[:Bh])
    finally:
        _clear(ctx)


def test_optimizer_follows_the_twin(gtop, scene):
    """Codes and counts against the twin's run, as tests/test_gpu_time.py holds the static optimizer to its twin: on
    the hand-derived case of tests/golden/TIME_MOVING_ANALYTIC.md (an empty field, one box, every corner distance
    linear), where no lookup can flip a decision — T_out within 1e-9, the info entries within 1e-6."""
    mp, _, _ = scene
    T, Df, x, p, (p0, vel, scale), t0, _ = analytic_case()
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map([8.0, 8.0, 3.0], [0.0, 0.0, 0.0], 0.2)
        ctx.update_sdf_map(np.array([[7.9, 7.9, 2.9]]))                 # (one voxel far from everything the case reads)
        ctx.set_params(**{k: p[k] for k in ("ws", "wc", "alpha", "r", "d0")})
        ctx.set_moving_boxes(p0, vel, scale)
        ctx.set_moving_cost(True)
        ctx.set_start_times(t0)
        b = problem.Batch(None, None, np.stack([Df, Df]), np.stack([x, x]), len(T))
        Tb = np.stack([T, T * np.array([1.3, 0.7, 1.1])])
        c, g, g0, parts = _gradient(gtop, ctx, b, Tb, want_parts=True)
        # the hand-derived values, at 1e-5
        u, r = ANALYTIC["u"], p["r"]
        for i in range(1):                                              # (row 1 is off the constant-speed times)
            ref = analytic_parts(Tb[i], p, t0)
            q = -(u / r) * ref
            assert np.max(np.abs(parts[i, :, 1] - ref) / ref) <= TOL
            assert np.max(np.abs(parts[i, :, 4] - q) / np.abs(q)) <= TOL
            assert np.max(np.abs(parts[i, :, 5] - np.r_[np.cumsum(q[::-1])[::-1][1:], 0.0])) <= TOL * np.abs(q).sum()
            assert abs(g0[i] - q.sum()) <= TOL * abs(q.sum())
        opts = dict(OPT, rho=1.0, t_min=0.2, t_max=3.0, max_evals=15)
        T_lo = np.tile(np.array([0.0, 5.0, 0.5]), (2, 1))
        T_out, info = _optimize(gtop, ctx, b, Tb, opts, T_lo)
        To, io = T_out.cpu().numpy(), info.cpu().numpy()
        osdf = analytic_case_field()
        osdf.dist[:] = ctx.get_sdf().reshape(-1)
        look = tm.BoxLookup(osdf, p0, vel, scale)
        for i in range(2):
            T_ref, i_ref = tm.optimize_times(Tb[i], Df, x, look, p, T_lo=T_lo[i], t0=t0, **opts)
            print(f"row {i}: code {int(io[i, 0])} after {int(io[i, 2])} evaluations, T_out off the twin's by "
                  f"{np.max(np.abs(To[i] - T_ref)):.2e}")
            assert np.array_equal(io[i, :3], i_ref[:3]), (i, io[i], i_ref)
            assert np.max(np.abs(To[i] - T_ref)) <= 1e-9
            assert np.max(np.abs(io[i, 3:] - i_ref[3:]) / np.maximum(np.abs(i_ref[3:]), 1e-12)) <= 1e-6
    finally:
        ctx.close()


def analytic_case_field():
    from oracle import oracle
    return analytic_case(oracle)[6]


def test_optimizer_returns_the_static_bits_with_the_mode_off(gtop, scene):
    import torch
    mp, ctx, sdf = scene
    b, T = _batch(9, 6, mp, 8300)
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    T_ref, i_ref = gtop.optimize_times_device(ctx, gtop.GtopTimeOpt(**OPT), x, Df, Tt)
    torch.cuda.synchronize()
    T_out, info = _optimize(gtop, ctx, b, T, OPT)
    assert torch.equal(T_out, T_ref) and torch.equal(info, i_ref)
    try:
        ctx.set_moving_cost(True)                                       # on, without boxes: the same
        T_out, info = _optimize(gtop, ctx, b, T, OPT)
        assert torch.equal(T_out, T_ref) and torch.equal(info, i_ref)
    finally:
        _clear(ctx)


def test_timing_gets_a_row_past_a_crossing_box(gtop, scene):
    """The point of the feature: rho = 0, a box crosses the path of every row at the time the row is there; the time
    optimizer changes the rows' timing, and the moving-mode cost of eval_device at T_out is below the cost at T_in —
    no waypoint moved."""
    import torch
    mp, ctx, sdf = scene
    B, m = 8, 5
    b, T = _batch(B, m, mp, 8400)
    t0 = 0.3
    w = 3
    p_at = np.stack([_waypoint(b, r, w) for r in range(B)])
    when = t0 + T[:, :w].sum(1)
    vel = np.random.default_rng(5).uniform(0.6, 1.0, (B, 3)) * np.array([1.0, -1.0, 0.0])
    bx = dict(poly=False, p0=p_at - vel * when[:, None], vel=vel, scale=np.full((B, 3), 0.8))
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    try:
        set_boxes(ctx, bx)
        ctx.set_moving_cost(True)
        ctx.set_start_times(t0)
        c_in = ctx.eval_device(x, Df, Tt)[0].clone()
        T_out, info = _optimize(gtop, ctx, b, T, dict(OPT, rho=0.0, max_evals=30))
        c_out = ctx.eval_device(x, Df, T_out)[0].clone()
        torch.cuda.synchronize()
    finally:
        _clear(ctx)
    c_in, c_out, To = c_in.cpu().numpy(), c_out.cpu().numpy(), T_out.cpu().numpy()
    print("cost in  ", np.array2string(c_in, precision=3), "\ncost out ", np.array2string(c_out, precision=3),
          "\nlargest change of a segment time per row", np.array2string(np.max(np.abs(To - T), axis=1), precision=3))
    assert np.all(c_out < c_in) and np.all(np.max(np.abs(To - T), axis=1) > 1e-3)
    assert np.max(np.abs(info[:, 5].cpu().numpy() - c_out) / c_out) <= TOL


def test_one_captured_graph_replays_the_eager_bits(gtop, scene):
    """refresh_box_predictions_device -> moving-mode optimize_device_ex -> optimize_times_moving_device -> the report,
    captured once: the replay gives the eager run's bits, and a history rewritten in place between replays is picked up."""
    import torch
    from grad_traj_optimization_amd import prediction as gp
    from tests import predict_twin as pt
    from tests.test_gpu_prediction import HORIZON, INFLATE, observed, opts_of
    from tests.test_gpu_prediction import dev as pdev
    mp, ctx, sdf = scene
    B, m, N, H = 40, 6, 5, 20
    b, T = _batch(B, m, mp, 8500)
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    x0, Df, Tt, lbt, ubt = _dev(b.x, b.Df.reshape(-1, 18), T, lb, ub)
    hist_a, count_a, head_a, first, scale = observed(b, N, H, seed=91)
    hist_b, count_b, head_b, _, _ = observed(b, N, H, seed=92)
    h, c, hd = pdev(hist_a), pdev(count_a, torch.int32), pdev(head_a, torch.int32)
    sc = pdev(scale)
    popts = opts_of(pt.POLYFIT, lam=0.05, horizon=HORIZON, inflate=INFLATE)
    topts = gtop.GtopTimeOpt(**dict(OPT, max_evals=10))
    pinfo = torch.zeros(N, 12, dtype=torch.float64, device="cuda:0")
    out = [torch.zeros(s, dtype=torch.float64, device="cuda:0") for s in ((B, m), (B, 8), (B, 12))]
    limits = gtop.GtopLimits(margin=0.3, use_boxes=True)

    def cycle(xw):
        gp.refresh_box_predictions_device(ctx, h, c, popts, hd, scale=sc, info=pinfo)
        _, cost, nev, code = ctx.optimize_device_ex(xw, Df, Tt, lbt, ubt, 8)
        gtop.optimize_times_moving_device(ctx, topts, xw, Df, Tt, T_out=out[0], info=out[1])
        coeff = ctx.coefficients_device(xw, Df, out[0])
        ctx.validate_device(coeff, out[0], limits, report=out[2])
        return cost, nev, code

    def eager(hist, count, head):
        ctx.set_moving_box_polynomials(*first)
        h.copy_(pdev(hist)); c.copy_(pdev(count, torch.int32)); hd.copy_(pdev(head, torch.int32))
        xe = x0.clone()
        res = cycle(xe)
        torch.cuda.synchronize()
        return [t.clone() for t in (*out, pinfo, xe, *res)]

    try:
        ctx.set_moving_cost(True)
        ctx.set_start_times(0.2)
        want_b = eager(hist_b, count_b, head_b)
        want_a = eager(hist_a, count_a, head_a)
        assert not torch.equal(want_a[0], Tt) and not torch.equal(want_a[0], want_b[0])
        for t in out:
            t.zero_()
        ctx.set_moving_box_polynomials(*first)
        xg = x0.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            res = cycle(xg)
        for want, (hist, count, head) in ((want_a, (hist_a, count_a, head_a)), (want_b, (hist_b, count_b, head_b)),
                                          (want_a, (hist_a, count_a, head_a))):
            ctx.set_moving_box_polynomials(*first)      # (same length: the buffer stays where the capture saw it)
            h.copy_(pdev(hist)); c.copy_(pdev(count, torch.int32)); hd.copy_(pdev(head, torch.int32))
            xg.copy_(x0)
            graph.replay()
            torch.cuda.synchronize()
            for k, (a, w) in enumerate(zip((*out, pinfo, xg, *res), want)):
                assert torch.equal(a, w), k
    finally:
        _clear(ctx)


def test_refusals_launch_nothing_and_the_static_header_still_refuses(gtop, scene):
    import torch
    from grad_traj_optimization_amd import timeopt as gt
    from grad_traj_optimization_amd import timeopt_moving as gm
    mp, ctx, sdf = scene
    L = gm.time_moving_library()
    b, T = _batch(3, 4, mp, 5600)
    B, m = 3, 4
    x, Df, Tt = _dev(b.x, b.Df.reshape(-1, 18), T)
    outs = [torch.full((n,), GUARD, dtype=torch.float64, device="cuda:0") for n in (B, B * m, B, B * m * 6, B * m, B * 8)]
    pc, pg, p0_, pp, pT, pi = (t.data_ptr() for t in outs)
    px, pD, pTt = x.data_ptr(), Df.data_ptr(), Tt.data_ptr()
    ok = gt.GtopTimeOpt(**OPT)

    def grad(B=B, m=m, px=px, pD=pD, pT_=pTt, stride=m, pc=pc, pg=pg):
        return L.gtop_time_gradient_moving_device(ctx._h, B, m, px, pD, pT_, stride, pc, pg, p0_, pp, None)

    def opt(o=ok, B=B, m=m, px=px, pD=pD, pT_=pTt, stride=m, plo=None, pout=pT, pinfo=pi):
        return L.gtop_optimize_times_moving_device(ctx._h, None if o is None else C.byref(o), B, m, px, pD, pT_, stride,
                                                   plo, pout, pinfo, None)

    def invalid_calls():
        for rc in (grad(m=1), grad(m=228), grad(B=-1), grad(stride=3), grad(stride=1), grad(px=None), grad(pD=None),
                   grad(pT_=None), grad(pc=None), grad(pg=None),
                   opt(m=1), opt(m=228), opt(B=-1), opt(stride=2), opt(px=None), opt(pD=None), opt(pT_=None),
                   opt(pout=None), opt(pinfo=None), opt(o=None), opt(pout=pTt)):
            assert rc == ERR_INVALID
        for bad in (dict(reserved=1), dict(rho=-1.0), dict(rho=np.nan), dict(t_min=0.03), dict(t_min=5.0, t_max=4.0),
                    dict(t_max=np.inf), dict(first_move=0.0), dict(first_move=np.nan), dict(ftol_rel=-1e-3),
                    dict(xtol_abs=np.nan), dict(max_evals=0)):
            assert opt(o=gt.GtopTimeOpt(**dict(OPT, **bad))) == ERR_INVALID, bad
        assert grad(B=0) == 0 and opt(B=0) == 0

    bx = special_boxes(*_special_rows(mp), 0.5)
    try:
        invalid_calls()                                                     # mode off
        ctx.set_moving_cost(True)
        set_boxes(ctx, bx)
        invalid_calls()                                                     # mode on, boxes set
        ctx.set_problem(T, b.Df)
        # the refusals of a moving-mode evaluation: a start-time count that fits neither 1, B nor the problem's batch
        ctx.set_start_times(np.array([0.1, 0.2]))
        assert grad() == ERR_INVALID and opt() == ERR_INVALID
        for call in (lambda: gtop.time_gradient_moving_batch(ctx, b.x), lambda: gtop.optimize_times_moving(ctx, ok, b.x)):
            with pytest.raises(gtop.GtopError) as e:
                call()
            assert e.value.code == ERR_INVALID
        ctx.set_start_times(None)
        # a negative extent; more than 32 boxes
        ctx.set_moving_boxes(bx["p0"], bx["vel"], bx["scale"] * np.array([1.0, -1.0, 1.0]))
        assert grad() == ERR_INVALID and opt() == ERR_INVALID
        many = np.tile(bx["p0"], (9, 1))[:33]
        ctx.set_moving_boxes(many, np.zeros_like(many), np.ones_like(many))
        assert grad() == ERR_INVALID and opt() == ERR_INVALID
        with pytest.raises(gtop.GtopError) as e:
            gtop.time_gradient_moving_batch(ctx, b.x)
        assert e.value.code == ERR_INVALID
        torch.cuda.synchronize()
        assert all(bool(torch.all(t == GUARD)) for t in outs)
        # gtop_time.h still refuses with the mode on; this header serves
        set_boxes(ctx, bx)
        with pytest.raises(gtop.GtopError) as e:
            gtop.time_gradient_device(ctx, x, Df, Tt)
        assert e.value.code == ERR_STATE
        with pytest.raises(gtop.GtopError) as e:
            gtop.optimize_times_device(ctx, ok, x, Df, Tt)
        assert e.value.code == ERR_STATE
        with pytest.raises(ValueError):
            gtop.time_gradient_moving_device(ctx, x, Df, Tt, gt0=outs[1])
        assert grad() == 0 and opt() == 0
        torch.cuda.synchronize()
        assert not any(bool(torch.any(t == GUARD)) for t in outs)
    finally:
        _clear(ctx)
    # no parameters, no field: GTOP_ERR_STATE
    bare = gtop.GtopContext(device=0)
    try:
        assert L.gtop_time_gradient_moving_device(bare._h, B, m, px, pD, pTt, m, pc, pg, p0_, pp, None) == ERR_STATE
        assert L.gtop_optimize_times_moving_device(bare._h, C.byref(ok), B, m, px, pD, pTt, m, None, pT, pi, None) == ERR_STATE
    finally:
        bare.close()
