"""The binding's one stream rule on the device: every method with a `stream` parameter gives the same result, bit for
bit, on torch's current stream (None), on a side stream named by its handle and on the same side stream given as the
torch Stream object.  Well-formed arguments only: what the binding refuses is tested without a GPU
(tests/test_binding_args.py)."""
import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests.test_gpu_validate import MARGIN, make_ctx

pytestmark = pytest.mark.gpu

GRID, B, DT = (48, 40, 24), 3, 0.02


@pytest.fixture(scope="module")
def world(gtop):
    mp = problem.make_map(GRID, density=0.04, seed=17)
    ctx = make_ctx(gtop, mp)
    yield mp, ctx
    ctx.close()


def three_ways(prepare, launch):
    """prepare() -> fresh arguments, made on the current stream; launch(args, stream) -> the tensors to compare, or a
    function that reads them once the stream is idle.  The side stream waits for the current one before each of its
    launches and is synchronised behind it."""
    import torch
    side = torch.cuda.Stream()
    seen = []
    for form in ("current", "handle", "object"):
        args = prepare()
        if form == "current":
            out = launch(args, None)
            torch.cuda.current_stream().synchronize()
        else:
            side.wait_stream(torch.cuda.current_stream())
            out = launch(args, side.cuda_stream if form == "handle" else side)
            side.synchronize()
        seen.append([o.cpu().numpy() for o in out] if not callable(out) else [out()])
    for other in seen[1:]:
        assert len(other) == len(seen[0]) > 0
        for a, b in zip(seen[0], other):
            assert a.dtype == b.dtype and a.shape == b.shape and a.size > 0 and np.array_equal(a, b, equal_nan=True)
    return seen[0]


def _problem(gtop, mp, m, shared_T):
    import torch
    dev = torch.device("cuda:0")
    b = problem.make_trajectories(B, m, mp, seed=23 + m)
    lb, ub = (torch.tensor(a, device=dev) for a in gtop.GtopContext.default_bounds(b.waypoints))
    T = torch.tensor(b.T[0] if shared_T else b.T, device=dev)
    return b, torch.tensor(b.x, device=dev), torch.tensor(b.Df.reshape(-1, 18), device=dev), T, lb, ub


@pytest.mark.parametrize("shared_T", (False, True), ids=("T(B,m)", "T(m,)"))
@pytest.mark.parametrize("m", (2, 3))
def test_every_stream_form_gives_the_same_bits(world, gtop, m, shared_T):
    import torch
    mp, ctx = world
    b, x, Df, T, lb, ub = _problem(gtop, mp, m, shared_T)
    wp = torch.tensor(b.waypoints, device=x.device)
    lim = gtop.GtopLimits(margin=MARGIN, max_vel=1.0, max_acc=1.0)
    none = lambda: ()

    cost, grad = three_ways(none, lambda a, s: ctx.eval_device(x, Df, T, stream=s))
    assert np.all(cost > 0)
    three_ways(none, lambda a, s: ctx.setup_paths_device(wp, stream=s))
    three_ways(lambda: x.clone(), lambda xc, s: (ctx.min_jerk_start_device(xc, Df, T, stream=s),))
    three_ways(none, lambda a, s: (ctx.coefficients_device(x, Df, T, stream=s),))
    coeff = ctx.coefficients_device(x, Df, T)
    three_ways(none, lambda a, s: (ctx.eval_trajectories_device(coeff, T, DT, stream=s),))
    three_ways(none, lambda a, s: ctx.sample_trajectories_device(coeff, T, DT, 64, stream=s))
    report, = three_ways(none, lambda a, s: (ctx.validate_device(coeff, T, lim, DT, stream=s),))
    seg, = three_ways(none, lambda a, s: (ctx.validate_segments_device(coeff, T, lim, DT, stream=s),))
    report_d, cost_d, seg_d = (torch.tensor(a, device=x.device) for a in (report, cost, seg))
    three_ways(none, lambda a, s: ctx.select_best_device(report_d, cost_d, gtop.GtopLimits(margin=-1.0), stream=s))
    length = gtop.GtopRetime(mode=0)
    three_ways(none, lambda a, s: (ctx.reallocate_times_device(length, x=x, Df=Df, stream=s),))
    limits = gtop.GtopRetime(mode=1, max_vel=1.0, max_acc=1.0, scale_x=1)
    three_ways(lambda: x.clone(), lambda xc, s: (ctx.reallocate_times_device(limits, x=xc, T=T, seg_report=seg_d, stream=s), xc))
    three_ways(lambda: x.clone(), lambda xc, s: ctx.optimize_device(xc, Df, T, lb, ub, 6, stream=s))
    three_ways(lambda: x.clone(), lambda xc, s: ctx.optimize_device_ex(xc, Df, T, lb, ub, 6, stream=s))


def test_field_queries_map_updates_and_copies_on_every_stream_form(world, gtop):
    import torch
    mp, ctx = world
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    none = lambda: ()
    pos = torch.tensor(mp.origin + rng.uniform(0.05, 0.95, (37, 3)) * mp.map_size, device=dev)
    time = torch.full((37,), -1.0, dtype=torch.float64, device=dev)
    three_ways(none, lambda a, s: ctx.edt_query_device(pos, time, stream=s))

    src = torch.arange(64, dtype=torch.float64, device=dev)
    copied, = three_ways(lambda: torch.zeros(64, dtype=torch.float64, device=dev),
                         lambda dst, s: (ctx.push_rows(src, [dst.data_ptr()], stream=s), dst)[1:])
    assert np.array_equal(copied, np.arange(64.0))

    side = torch.cuda.Stream()
    for s in (None, side.cuda_stream, side):
        mm = torch.tensor([2 ** 63 - 1, 0], dtype=torch.int64, device=dev)
        side.wait_stream(torch.cuda.current_stream())
        ctx.clock_stamp(mm, stream=s)
        torch.cuda.synchronize()
        lo, hi = mm.tolist()
        assert 0 < lo == hi < 2 ** 63 - 1

    # a context of its own: the module's field stays as the other test reads it
    own = make_ctx(gtop, mp)
    pts = torch.tensor(mp.obstacle_points()[::2], device=dev)
    three_ways(none, lambda a, s: (own.update_sdf_map_device(pts, stream=s), own.get_sdf)[1])
    lo, hi = mp.origin + 0.2 * mp.map_size, mp.origin + 0.7 * mp.map_size
    inside = torch.tensor(lo + rng.uniform(0.0, 1.0, (20, 3)) * (hi - lo), device=dev)
    three_ways(none, lambda a, s: (own.update_sdf_map_window_device(lo, hi, inside, stream=s), own.get_sdf)[1])
    own.close()
