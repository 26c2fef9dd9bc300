"""The swarm term at the limits of its segment and sample ranges (tests/swarm_limit_cases.py): the shapes at which
swarm_rows_kernel takes a second pass over the free variables (m >= 9) and over kstart[] (m >= 64), stages the moments
over several 256-sample stages with segment boundaries inside them, skips 64-item passes, fills Gs[] (m = 227) and
meets segments that own no sample; at which sep_sample_kernel enters its stride loop (one, two and three tiles of
rows) and bisects over 65 536 samples — S, the gradient and the active count against tests/swarm_twin.py bit for bit,
each case showing from the twin's own walk that the edge it is named for is there, with guard words round every output
and the workspace, and the sampled positions the kernel leaves in the workspace against the twin's, sample by sample.

Then the `add` form of the rows kernel, which every round of the optimizer uses: one evaluation of
gtop_optimize_swarm_device reports fl(c_b + S_b), one float64 addition, by bits; and the serial restatement of
tests/test_gpu_swarm.py at 9, 65 and 118 segments."""
import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import swarm_limit_cases as lc
from tests import swarm_twin as sw
from tests.test_gpu_swarm import (bare, dev, device_rows, follows_the_serial_restatement, gathered_waypoints,  # noqa: F401
                                  grid_for, same, scene, start_list)

pytestmark = pytest.mark.gpu

GUARD_WORDS = 64


def workspace_positions(work, side, B, n):
    """pos [npad][3][Bpad] of the trial (side 0) or frozen (side 1) rows as the sample kernel left it in the workspace
    (the layout csrc/gtop_sep_sample.h states), as (B, npad, 3), and the same for the padding rows."""
    tiles, npad, _ = lc.sample_blocks(B, n)
    Bpad = tiles * lc.TILE
    words = npad * 3 * Bpad
    p = work[side * words * 8:(side + 1) * words * 8].cpu().numpy().view(np.float64).reshape(npad, 3, Bpad)
    return p[:, :, :B].transpose(2, 0, 1), p[:, :, B:]


@pytest.mark.parametrize("case", lc.LIMIT_CASES, ids=lc.case_id)
def test_device_equals_twin_at_the_limits(gtop, bare, case):
    import torch
    B, m, n, shared, t0_kind, hold, frozen, _ = case
    ctx = bare
    x, Df, T = sw.crossing_rows(B, m, 1000 + B + m, shared_T=shared)
    t0 = start_list(t0_kind, B, B + n)
    t_lo, dt = grid_for(T, t0, n)
    coeff, ch = device_rows(ctx, x, Df, T)
    fz = fh = None
    if frozen:
        xf, _, _ = sw.crossing_rows(B, m, 2000 + B + m, shared_T=shared)
        fz, fh = device_rows(ctx, xf, Df, T)
    opts = gtop.GtopSwarmOpts(t_lo=t_lo, dt=dt, n_samples=n, w=3.0, radius=1.0, hold_ends=bool(hold))
    # guard words round every output, guard bytes round the workspace (and 0x5A in it: a sample the kernel does not
    # write is then no NaN)
    need, nvar, G = gtop.swarm_workspace_bytes(B, m, n), 9 * (m - 1), GUARD_WORDS
    bufs = {k: torch.full((size + 2 * G,), -7.25, device="cuda:0", dtype=torch.float64)
            for k, size in (("S", B), ("g", B * nvar), ("a", B))}
    work = torch.full((need + 2 * G,), 0x5A, device="cuda:0", dtype=torch.uint8)
    ctx.set_start_times(t0)
    try:
        gtop.swarm_gradient_device(ctx, opts, coeff, dev(T), coeff_frozen=fz, S=bufs["S"][G:G + B],
                                   grad=bufs["g"][G:G + B * nvar].view(B, nvar), active=bufs["a"][G:G + B],
                                   work=work[G:G + need])
        torch.cuda.synchronize()
    finally:
        ctx.set_start_times(None)
    for k, size in (("S", B), ("g", B * nvar), ("a", B)):
        assert (bufs[k][:G] == -7.25).all() and (bufs[k][G + size:] == -7.25).all(), k
    assert (work[:G] == 0x5A).all() and (work[G + need:] == 0x5A).all()
    S, g, act = (bufs[k][G:G + size].cpu().numpy() for k, size in (("S", B), ("g", B * nvar), ("a", B)))
    g = g.reshape(B, nvar)

    # the case shows the edge it is named for, read from the twin's own walk of these rows
    pos, flown, _, seg = sw.sample_rows(ch, T, t0, t_lo, dt, n, hold)
    missing, figures = lc.edge_faults(case, seg, flown)
    print(lc.case_id(case), figures)
    assert missing == [], (missing, figures)

    # the positions the sample kernel left: the twin's where the row is flown, NaN elsewhere, on the padding samples and
    # on the padding rows
    for side, c in ((0, ch), (1, fh)):
        if c is None:
            continue
        want, fl = (pos, flown) if side == 0 else sw.sample_rows(c, T, t0, t_lo, dt, n, hold)[:2]
        got, padding_rows = workspace_positions(work[G:G + need], side, B, n)
        assert np.isnan(got[:, n:]).all() and np.isnan(padding_rows).all(), side
        assert np.isnan(got[:, :n][~fl]).all(), (side, np.argwhere(~np.isnan(got[:, :n][~fl]))[:4])
        assert same(got[:, :n][fl], want[fl]), (side, np.argwhere(got[:, :n][fl] != want[fl])[:4])

    St, gt, at, _ = sw.swarm_terms(ch, T, t0, t_lo, dt, n, hold, 3.0, 1.0, frozen=fh)
    assert at.sum() > 0 and (B <= 2 or (at == 0).sum() < B)                  # the case has active terms
    assert np.array_equal(act, at.astype(np.float64))
    assert same(S, St), np.max(np.abs(S - St))
    assert same(g, gt), (np.max(np.abs(g - gt)), np.argwhere(g != gt)[:4])


def gathered_problem(gtop, mp, B, m, seed):
    """(x0, Df (B, 18), T, lb, ub) of B robots gathered about the map's centre, x0 inside its bounds."""
    rng = np.random.default_rng(seed)
    wp = gathered_waypoints(mp, B, m, rng, inside=True)
    T = problem.segment_times(wp)
    Df, Dp = problem.initial_derivatives(wp)
    x0 = Dp.reshape(B, -1) + rng.normal(0.0, 0.05, (B, 9 * (m - 1)))
    lb, ub = gtop.GtopContext.default_bounds(wp)
    assert np.all(x0 >= lb) and np.all(x0 <= ub)
    return x0, Df.reshape(B, 18), T, lb, ub


# (B, m, n_samples, the start-time kind, the fusion modes of the rounds)
ADD_CASES = [(3, 9, 48, 0, (0, 1, 2)), (65, 13, 64, "B", (2,)), (3, 65, 130, 0, (2,)), (3, 118, 130, 0, (2,))]


@pytest.mark.parametrize("B,m,n,t0_kind,modes", ADD_CASES, ids=[f"B{c[0]}-m{c[1]}" for c in ADD_CASES])
def test_one_evaluation_is_one_addition(gtop, scene, B, m, n, t0_kind, modes):
    """gtop_optimize_swarm_device with one sweep of one evaluation: the rows kernel's add = 1 form wrote
    f[b] = f[b] + S_b on top of the context's own cost c_b, so min_cost[b] is fl(c_b + S_b) by bits — c_b what the same
    call reports at w = 0, S_b the gradient call's figure against the frozen copy of the same rows — and x comes back
    as it went in."""
    import torch
    mp, ctx, _ = scene
    x0, Df, T, lb, ub = gathered_problem(gtop, mp, B, m, 700 + m)
    t0 = start_list(t0_kind, B, B + m)
    Dft, Tt, lbt, ubt = dev(Df), dev(T), dev(lb), dev(ub)
    t_lo, dt = 0.0, float(np.max(T.sum(axis=1)) + (np.max(t0) if t0 is not None else 0.0)) / (n - 1)
    kw = dict(t_lo=t_lo, dt=dt, n_samples=n, radius=1.5, hold_ends=True)
    stop = gtop.GtopSwarmStop(1, 1)
    ctx.set_start_times(t0)
    try:
        coeff = ctx.coefficients_device(dev(x0), Dft, Tt)
        S, _, act = gtop.swarm_gradient_device(ctx, gtop.GtopSwarmOpts(w=40.0, **kw), coeff, Tt, coeff_frozen=coeff,
                                               want_active=True)
        torch.cuda.synchronize()
        S, act = S.cpu().numpy(), act.cpu().numpy()
        assert (act > 0).sum() >= 2 and (S > 0).sum() >= 2                    # the term takes part
        for mode in modes:
            ctx.set_optimizer_fusion(mode)
            x_alone, c_alone, _ = gtop.optimize_swarm_device(ctx, gtop.GtopSwarmOpts(w=0.0, **kw), stop, dev(x0), Dft, Tt,
                                                             lbt, ubt)
            x_swarm, c_swarm, _ = gtop.optimize_swarm_device(ctx, gtop.GtopSwarmOpts(w=40.0, **kw), stop, dev(x0), Dft, Tt,
                                                             lbt, ubt)
            torch.cuda.synchronize()
            c = c_alone.cpu().numpy()
            want = c + S                                                     # one float64 addition per row
            got = c_swarm.cpu().numpy()
            assert np.isfinite(c).all() and not same(want, c)
            assert same(got, want), (mode, np.argwhere(got != want)[:4], np.max(np.abs(got - want)))
            assert same(x_swarm.cpu().numpy(), x0) and same(x_alone.cpu().numpy(), x0), mode
    finally:
        ctx.set_optimizer_fusion(2)
        ctx.set_start_times(None)


@pytest.mark.parametrize("m,n,evals", [(9, 48, 6), (65, 130, 6), (118, 130, 6), (9, 48, 12), (65, 130, 12)])
def test_optimizer_follows_the_serial_restatement_at_long_rows(gtop, scene, oracle_mod, m, n, evals):
    """The serial restatement of tests/test_gpu_swarm.py where the rows kernel adds its gradient over a second pass of
    the variables (m = 9), a second pass of kstart[] (m = 65) and at the optimizer's largest segment count (m = 118,
    kept: the oracle's generator and the six evaluations of three rows take about six seconds of CPU), at the same
    1e-6, with the paths held inside the map.  After six evaluations the least cost is still the start cost at these
    shapes (every trial point so far was worse), so those runs hold the first evaluation and the refusal of the trial
    points; after twelve every row has moved to under 0.9 of its start cost, which is asserted, and the result hangs
    on the gradient the rows kernel added to."""
    costs, f_start = follows_the_serial_restatement(gtop, scene, oracle_mod, m, B=3, sweeps=1, evals=evals, n=n, inside=True)
    print(m, evals, "least cost / start cost", (costs / f_start).tolist())
    if evals == 12:
        assert np.all(costs < 0.9 * f_start)
