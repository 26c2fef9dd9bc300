"""Seeded fuzz of the trajectory report and the selection: 60 draws over maps, lengths, batch sizes, sampling steps, box
lists (0 .. 40 boxes, so lists past the 32 boxes of the moving-obstacle cost's limit are exercised, and 70 and 129, which
the report kernel restages 64 at a time inside its sample loop and the query kernel 128 at a time), start-time
forms and limits; each draw runs the exact comparisons of tests/test_gpu_validate.py (entries 0 .. 6 and 11 against
the composed entry points, 7 .. 10 against the twin's bound, the selection against the twin's rule)."""
import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import validate_twin as vt
from tests.test_gpu_validate import _boxes, check_exact, check_vel_acc, composed, make_ctx, set_boxes, with_out_of_map_row

pytestmark = pytest.mark.gpu

GRIDS = [(24, 20, 16), (48, 40, 24), (40, 64, 20), (72, 30, 28)]


@pytest.mark.parametrize("chunk", range(6))
def test_fuzz_report_and_selection(gtop, chunk):
    compared = 0
    for seed in range(10 * chunk, 10 * chunk + 10):
        rng = np.random.default_rng(1000 + seed)
        grid = GRIDS[rng.integers(len(GRIDS))]
        mp = problem.make_map(grid, density=float(rng.uniform(0.0, 0.06)), seed=seed)
        m = int(rng.choice([2, 3, 4, 6, 9, 13, 21]))
        B = int(rng.integers(1, 20))
        dt = float(rng.choice([0.01, 0.02, 0.05, 0.013]))
        b = problem.make_trajectories(B, m, mp, seed=seed + 500, boundary="random" if rng.uniform() < 0.5 else None)
        if rng.uniform() < 0.4:
            b = with_out_of_map_row(b, mp)
        n = len(b.x)
        nbox = int(rng.choice([0, 1, 5, 8, 31, 32, 33, 40, 70, 129]))
        boxes = _boxes(b, rng, nbox) if nbox else None
        form = rng.integers(3)
        t0 = [None, float(rng.uniform(0.0, 5.0)), rng.uniform(0.0, 5.0, n)][form]
        use_boxes = int(rng.uniform() < 0.75)
        margin = float(rng.choice([0.0, 0.2, 0.3, 0.6, -2.0]))
        sel = dict(max_vel=float(rng.choice([0.0, 2.0, 3.0])), max_acc=float(rng.choice([0.0, 2.0, 4.0, -1.0])),
                   per_axis=bool(rng.integers(2)), allow_out_of_map=bool(rng.integers(2)))
        ctx = make_ctx(gtop, mp)
        try:
            ctx.set_problem(b.T, b.Df)
            set_boxes(ctx, boxes)
            ctx.set_start_times(t0)
            cost, _ = ctx.eval_batch(b.x)
            if rng.uniform() < 0.3:
                cost[rng.integers(n)] = [np.nan, np.inf, -np.inf][rng.integers(3)]
            lim = gtop.GtopLimits(margin=margin, use_boxes=use_boxes, **sel)
            rep, ok, best = ctx.validate_batch(b.x, lim, cost=cost, dt_sample=dt)
            exp, rows = composed(ctx, mp, b, b.x, dt, margin, use_boxes, t0)
            assert rows == n, seed
            check_exact(rep, exp)
            check_vel_acc(ctx, b, b.x, rep, dt)
            ok_t, best_t = vt.select(rep, cost, **sel)
            assert np.array_equal(ok, ok_t) and np.array_equal(best, best_t), (seed, best, best_t)
            compared += n
        finally:
            ctx.close()
    assert compared >= 10
