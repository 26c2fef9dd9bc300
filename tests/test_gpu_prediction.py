"""Predictions fitted from observation histories on the device (include/gtop_prediction.h; csrc/gtop_prediction.hip)
through grad_traj_optimization_amd.prediction.

(1) Device = twin (tests/predict_twin.py), bit for bit, for both modes at the chunk edges of the kernel's sums
    (H = 2, 6, 7, 64, 65, 130), counts 0, 1, 2, 5, 6, H mixed in one batch with wrapped heads and every status; rows of
    objects that were not fitted keep their sentinel; guard words behind every output; a permuted batch gives permuted
    rows.
(2) refresh_box_predictions_device: the queries, the report and one moving-cost evaluation behind it give the bits
    they give after the host setter is called with the fit's coef, t_range and the inflated scale, at N = 5 and at
    N = 40 (where the cost refuses and the queries serve); scale = None keeps the extents; GTOP_ERR_STATE without a
    polynomial list of N boxes, the list in force unchanged.
(3) One captured graph of refresh + query follows a history buffer rewritten in place."""
import numpy as np
import pytest

from grad_traj_optimization_amd import prediction as gp
from grad_traj_optimization_amd import problem
from tests import predict_twin as pt

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
GUARD, SENTINEL = -12345.0, 7.0
VARIANT = dict(degree=3, lam=0.25, horizon=1.5, regularise_horizon=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def opts_of(mode, degree=5, lam=1.0, horizon=0.0, regularise_horizon=0, inflate=0.0):
    return gp.GtopPredictOpts(mode=mode, degree=degree, lambda_=lam, horizon=horizon,
                              regularise_horizon=regularise_horizon, inflate=inflate)


def guarded(shape, fill):
    """(the whole buffer, the output's view of it): 8 guard words behind the output."""
    import torch
    n = int(np.prod(shape))
    whole = torch.full((n + 8,), GUARD, dtype=torch.float64, device="cuda:0")
    whole[:n] = fill
    return whole, whole[:n].view(*shape)


@pytest.fixture(scope="module")
def ctx(gtop):
    c = gtop.GtopContext(device=0)
    yield c
    c.close()


def run_device(ctx, hist, count, head, opts, local=True):
    import torch
    N = hist.shape[0]
    outs = [guarded((N, 18), SENTINEL), guarded((N, 2), SENTINEL), guarded((N, 12), SENTINEL), guarded((N, 20), SENTINEL)]
    gp.fit_predictions_device(ctx, dev(hist), dev(count, torch.int32), opts, None if head is None else dev(head, torch.int32),
                              outs[0][1], outs[1][1], outs[2][1], outs[3][1] if local else None)
    torch.cuda.synchronize()
    for whole, _ in outs:
        assert np.all(whole[-8:].cpu().numpy() == GUARD)
    return [view.cpu().numpy() for _, view in outs]


@pytest.mark.parametrize("mode", [pt.POLYFIT, pt.CONST_VEL])
@pytest.mark.parametrize("H", [2, 6, 7, 64, 65, 130])
@pytest.mark.parametrize("N", [1, 3, 65])
def test_device_equals_twin(ctx, N, H, mode):
    hist, count, head = pt.make_batch(N, H)
    want = pt.fit_batch(N, H, mode, sentinel=SENTINEL)
    got = run_device(ctx, hist, count, head, opts_of(mode))
    for g, w, what in zip(got, want, ("coef", "t_range", "info", "local")):
        assert same_bits(g, w), (what, np.argwhere(bits(g) != bits(w))[:4])
    status = want[2][:, 0]
    untouched = status >= pt.EMPTY
    assert np.all(got[0][untouched] == SENTINEL) and np.all(got[1][untouched] == SENTINEL)
    assert np.all(got[3][untouched] == SENTINEL)
    if N == 65:
        present = set(status.astype(int))
        assert present == ({pt.OK, pt.LOWERED, pt.EMPTY, pt.BAD} if mode == pt.CONST_VEL or H > 2 else
                           {pt.LOWERED, pt.EMPTY, pt.BAD}), present
    if N > 1:                                               # a permuted batch gives permuted rows
        perm = np.random.default_rng(N + H).permutation(N)
        again = run_device(ctx, hist[perm], count[perm], head[perm], opts_of(mode))
        for g, a in zip(got, again):
            assert same_bits(a, g[perm])


@pytest.mark.parametrize("mode", [pt.POLYFIT, pt.CONST_VEL])
def test_options_and_optional_arguments(ctx, mode):
    """A lower degree, another lambda, a horizon inside the regulariser; no head (every ring starts at slot 0), no local."""
    N, H = 65, 65
    hist, count, head = pt.make_batch(N, H)
    want = pt.fit_batch(N, H, mode, sentinel=SENTINEL, **VARIANT)
    got = run_device(ctx, hist, count, head, opts_of(mode, **VARIANT))
    assert all(same_bits(g, w) for g, w in zip(got, want))
    assert np.all(want[1][want[2][:, 0] <= pt.LOWERED, 1] == want[2][want[2][:, 0] <= pt.LOWERED, 4] + 1.5)
    flat = np.stack([np.roll(hist[n], -(int(head[n]) % H), axis=0) for n in range(N)])     # the rings unwrapped
    unwrapped = run_device(ctx, flat, count, None, opts_of(mode, **VARIANT), local=False)
    assert all(same_bits(u, w) for u, w in zip(unwrapped[:3], want[:3]))
    assert np.all(unwrapped[3] == SENTINEL)                 # local = NULL: not written
    inf = run_device(ctx, hist, count, head, opts_of(mode, horizon=np.inf))
    fitted = inf[2][:, 0] <= pt.LOWERED
    assert np.all(np.isposinf(inf[1][fitted, 1])) and same_bits(inf[0], pt.fit_batch(N, H, mode, sentinel=SENTINEL)[0])


def test_refusals_of_the_device_entry(ctx, gtop):
    import torch
    hist, count, head = pt.make_batch(3, 7)
    h, c = dev(hist), dev(count, torch.int32)
    for bad in (dict(mode=2), dict(degree=0), dict(degree=6), dict(lam=-1.0), dict(lam=np.nan), dict(horizon=-0.5),
                dict(horizon=np.nan), dict(inflate=-1.0), dict(inflate=np.inf), dict(regularise_horizon=2),
                dict(regularise_horizon=1, horizon=np.inf)):
        kw = dict(mode=0)
        kw.update(bad)
        with pytest.raises(gtop.GtopError) as e:
            gp.fit_predictions_device(ctx, h, c, opts_of(**kw))
        assert e.value.code == ERR_INVALID, bad
    o = opts_of(0)
    o.reserved = 1
    with pytest.raises(gtop.GtopError) as e:
        gp.fit_predictions_device(ctx, h, c, o)
    assert e.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        gp.fit_predictions_device(ctx, h, c[:2], opts_of(0))
    with pytest.raises(ValueError):
        gp.fit_predictions_device(ctx, h.cpu(), c, opts_of(0))
    shifted = torch.zeros(h.numel() + 1, dtype=torch.float64, device=h.device)[1:].view(*h.shape)
    with pytest.raises(gtop.GtopError) as e:                # a history that is not 16-byte aligned
        gp.fit_predictions_device(ctx, shifted, c, opts_of(0))
    assert e.value.code == ERR_INVALID
    coef, t_range, info, local = gp.fit_predictions_device(ctx, h[:0], c[:0], opts_of(0))   # N = 0: nothing launched
    assert coef.shape == (0, 18) and info.shape == (0, 12) and local is None


# ---- the refresh of the context's box list ----
PARAMS = dict(alpha=10.0, r=0.5, d0=0.8)
HORIZON, INFLATE = 2.5, 1.5


@pytest.fixture(scope="module")
def world(gtop):
    mp = problem.make_map((48, 40, 24), density=0.03, seed=3)
    b = problem.make_trajectories(4, 6, mp, seed=4)
    c = gtop.GtopContext(device=0)
    c.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    c.update_sdf_map(mp.obstacle_points())
    c.set_params(**PARAMS)
    c.set_problem(b.T, b.Df)
    yield mp, b, c
    c.close()


def observed(b, N, H, seed):
    """Histories of N objects that cross the trajectories' waypoints about when they are flown: the last observation is
    taken up to 1.5 s before, so the prediction matters.  Object 1 has no samples (its row must stay); object 2 has
    three.  -> (hist, count, head, first list (coef, scale, t_range), new scale)"""
    rng = np.random.default_rng(seed)
    hist = np.full((N, H, 4), np.nan)
    count = rng.integers(6, H + 1, N).astype(np.int32)
    count[1 % N], count[2 % N] = 0, 3
    head = rng.integers(0, H, N).astype(np.int32)
    for n in range(N):
        j, w = rng.integers(0, len(b.x)), rng.integers(1, b.m)
        when = b.T[j][:w].sum()
        vel = rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 1.0, 0.2])
        acc = rng.uniform(-0.5, 0.5, 3) * np.array([1.0, 1.0, 0.2])
        t = np.sort(rng.uniform(when - 2.5, when - rng.uniform(0.2, 1.5), count[n]))
        for i in range(count[n]):
            u = t[i] - when
            hist[n, (head[n] + i) % H, :3] = b.waypoints[j, w] + vel * u + 0.5 * acc * u * u + 0.02 * rng.normal(size=3)
            hist[n, (head[n] + i) % H, 3] = t[i]
    coef = np.zeros((N, 3, 6))
    coef[:, :, 0] = rng.uniform(0.0, 5.0, (N, 3))
    first = (coef, rng.uniform(0.5, 1.0, (N, 3)), np.stack([np.zeros(N), np.full(N, 10.0)], axis=1))
    return hist, count, head, first, rng.uniform(1.0, 2.0, (N, 3))


def consumers(gtop, ctx, b, pos, tau, coeff, T, expect_cost):
    """edt_query_device, validate_device with boxes and one moving-cost evaluation with the list in force."""
    import torch
    dist, grad = ctx.edt_query_device(pos, tau)
    report = ctx.validate_device(coeff, T, gtop.GtopLimits(margin=0.3, use_boxes=True))
    out = dict(dist=dist, grad=grad, report=report)
    x, Df = dev(b.x), dev(b.Df.reshape(-1, 18))
    if expect_cost:
        out["cost"], out["cost_grad"] = ctx.eval_device(x, Df, T)
    else:
        with pytest.raises(gtop.GtopError) as e:            # a list too long for the cost term: refused, as today
            ctx.eval_device(x, Df, T)
        assert e.value.code == ERR_INVALID
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("N", [5, 40])
def test_refresh_is_the_host_setter_with_the_fit(gtop, world, N):
    import torch
    mp, b, ctx = world
    H = 20
    hist, count, head, first, scale = observed(b, N, H, seed=70 + N)
    opts = opts_of(pt.POLYFIT, lam=0.05, horizon=HORIZON, inflate=INFLATE)
    coef, t_range, info, _ = gp.fit_predictions(hist, count, opts, head=head)
    fitted = info[:, 0] <= pt.LOWERED
    assert fitted.sum() == N - 1 and not fitted[1 % N]
    assert info[fitted, 6:9].max() > 1e-3                   # the fit misses by more than rounding: inflate matters
    # what the setter must be given to say the same: the fitted rows, the others as they stood
    coef_set, scale_keep, tr_set = (a.copy() for a in first)
    coef_set[fitted], tr_set[fitted] = coef[fitted].reshape(-1, 3, 6), t_range[fitted]
    scale_new = scale_keep.copy()
    scale_new[fitted] = 2.0 * pt.half_extents(scale, INFLATE, info)[fitted]
    rng = np.random.default_rng(N)
    x, Df, T = dev(b.x), dev(b.Df.reshape(-1, 18)), dev(b.T)
    coeff = ctx.coefficients_device(x, Df, T)
    npos = 400
    pos = dev(np.concatenate([b.waypoints.reshape(-1, 3)[rng.integers(0, b.waypoints.size // 3, npos)]
                              + rng.normal(size=(npos, 3)) * 0.5]))
    tau = dev(rng.uniform(0.0, 8.0, npos))
    h, c, hd = dev(hist), dev(count, torch.int32), dev(head, torch.int32)
    ctx.set_moving_cost(True)
    try:
        cost = N <= gtop.GtopContext.MOVING_COST_MAX_BOXES
        ctx.set_moving_box_polynomials(*first)
        before = consumers(gtop, ctx, b, pos, tau, coeff, T, cost)
        info_dev = gp.refresh_box_predictions_device(ctx, h, c, opts, hd, scale=dev(scale))
        got = consumers(gtop, ctx, b, pos, tau, coeff, T, cost)
        assert same_bits(info_dev.cpu().numpy(), info)
        assert ctx.moving_box_kind() == (gtop.GtopContext.BOXES_POLYNOMIAL, N)
        ctx.set_moving_box_polynomials(coef_set, scale_new, tr_set)
        want = consumers(gtop, ctx, b, pos, tau, coeff, T, cost)
        for name in want:
            assert same_bits(got[name], want[name]), name
        assert not same_bits(before["dist"], want["dist"]) and not same_bits(before["report"], want["report"])
        if cost:
            assert not same_bits(before["cost"], want["cost"])
        # scale = None keeps the extents in force
        ctx.set_moving_box_polynomials(*first)
        gp.refresh_box_predictions_device(ctx, h, c, opts, hd)
        kept = consumers(gtop, ctx, b, pos, tau, coeff, T, cost)
        ctx.set_moving_box_polynomials(coef_set, scale_keep, tr_set)
        want_kept = consumers(gtop, ctx, b, pos, tau, coeff, T, cost)
        for name in want_kept:
            assert same_bits(kept[name], want_kept[name]), name
        assert not same_bits(want_kept["dist"], want["dist"])
        # a bad extent: that object is BAD and its row stays
        bad_scale = scale.copy()
        bad_scale[0, 1] = -1.0
        ctx.set_moving_box_polynomials(*first)
        info_bad = gp.refresh_box_predictions_device(ctx, h, c, opts, hd, scale=dev(bad_scale)).cpu().numpy()
        assert info_bad[0, 0] == pt.BAD and np.all(info_bad[0, 2:] == 0.0) and same_bits(info_bad[1:], info[1:])
        one_stays = consumers(gtop, ctx, b, pos, tau, coeff, T, cost)
        cs, ss, ts = coef_set.copy(), scale_new.copy(), tr_set.copy()
        cs[0], ss[0], ts[0] = first[0][0], first[1][0], first[2][0]
        ctx.set_moving_box_polynomials(cs, ss, ts)
        want_one = consumers(gtop, ctx, b, pos, tau, coeff, T, cost)
        for name in want_one:
            assert same_bits(one_stays[name], want_one[name]), name
    finally:
        ctx.set_moving_cost(False)
        ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))


def test_refresh_needs_a_polynomial_list_of_n_boxes(gtop, world):
    import torch
    mp, b, ctx = world
    N, H = 5, 20
    hist, count, head, first, scale = observed(b, N, H, seed=75)
    h, c, hd = dev(hist), dev(count, torch.int32), dev(head, torch.int32)
    opts = opts_of(pt.POLYFIT, horizon=HORIZON)
    rng = np.random.default_rng(5)
    pos, tau = dev(rng.uniform(0.0, 5.0, (200, 3))), dev(rng.uniform(0.0, 8.0, 200))
    none = np.zeros((0, 3))

    def refused():
        dist0 = ctx.edt_query_device(pos, tau)[0].cpu().numpy()
        kind0 = ctx.moving_box_kind()
        info = torch.full((N, 12), SENTINEL, dtype=torch.float64, device="cuda:0")
        with pytest.raises(gtop.GtopError) as e:
            gp.refresh_box_predictions_device(ctx, h, c, opts, hd, scale=dev(scale), info=info)
        assert e.value.code == ERR_STATE
        torch.cuda.synchronize()
        assert np.all(info.cpu().numpy() == SENTINEL)       # nothing written
        assert ctx.moving_box_kind() == kind0 and same_bits(ctx.edt_query_device(pos, tau)[0].cpu().numpy(), dist0)

    try:
        ctx.set_moving_boxes(none, none, none)              # no list
        refused()
        ctx.set_moving_boxes(first[0][:, :, 0], np.zeros((N, 3)), first[1])      # a constant-velocity list
        refused()
        ctx.set_moving_box_polynomials(first[0][:4], first[1][:4], first[2][:4])   # a list of another length
        refused()
        ctx.set_moving_box_polynomials(*first)
        with pytest.raises(gtop.GtopError) as e:            # bad options come first
            gp.refresh_box_predictions_device(ctx, h, c, opts_of(pt.POLYFIT, degree=9), hd)
        assert e.value.code == ERR_INVALID
        gp.refresh_box_predictions_device(ctx, h, c, opts, hd)
        torch.cuda.synchronize()
    finally:
        ctx.set_moving_boxes(none, none, none)


def test_one_graph_of_refresh_and_query_follows_the_history(gtop, world):
    import torch
    mp, b, ctx = world
    N, H = 5, 20
    hist_a, count_a, head_a, first, scale = observed(b, N, H, seed=81)
    hist_b, count_b, head_b, _, _ = observed(b, N, H, seed=82)
    opts = opts_of(pt.CONST_VEL, horizon=HORIZON, inflate=INFLATE)
    rng = np.random.default_rng(9)
    pos = dev(b.waypoints.reshape(-1, 3)[rng.integers(0, b.waypoints.size // 3, 300)] + rng.normal(size=(300, 3)) * 0.5)
    tau = dev(rng.uniform(0.0, 8.0, 300))
    h, c, hd = dev(hist_a), dev(count_a, torch.int32), dev(head_a, torch.int32)
    sc = dev(scale)
    info = torch.zeros(N, 12, dtype=torch.float64, device="cuda:0")

    def expected(hist, count, head):
        coef, t_range, inf, _ = gp.fit_predictions(hist, count, opts, head=head)
        fitted = inf[:, 0] <= pt.LOWERED
        cs, ss, ts = (a.copy() for a in first)
        cs[fitted], ts[fitted] = coef[fitted].reshape(-1, 3, 6), t_range[fitted]
        ss[fitted] = 2.0 * pt.half_extents(scale, INFLATE, inf)[fitted]
        ctx.set_moving_box_polynomials(cs, ss, ts)
        d, g = ctx.edt_query_device(pos, tau)
        torch.cuda.synchronize()
        return d.cpu().numpy(), g.cpu().numpy(), inf

    try:
        want_a = expected(hist_a, count_a, head_a)
        want_b = expected(hist_b, count_b, head_b)
        assert not same_bits(want_a[0], want_b[0])
        ctx.set_moving_box_polynomials(*first)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # warm-up outside the capture
            gp.refresh_box_predictions_device(ctx, h, c, opts, hd, scale=sc, info=info)
            ctx.edt_query_device(pos, tau)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gp.refresh_box_predictions_device(ctx, h, c, opts, hd, scale=sc, info=info)
            dist, grad = ctx.edt_query_device(pos, tau)
        ctx.set_moving_box_polynomials(*first)      # (same length: the buffer stays where the capture saw it)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(dist.cpu().numpy(), want_a[0]) and same_bits(grad.cpu().numpy(), want_a[1])
        assert same_bits(info.cpu().numpy(), want_a[2])
        ctx.set_moving_box_polynomials(*first)
        h.copy_(dev(hist_b))            # the buffers rewritten in place: the replay follows the new history
        c.copy_(dev(count_b, torch.int32))
        hd.copy_(dev(head_b, torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(dist.cpu().numpy(), want_b[0]) and same_bits(grad.cpu().numpy(), want_b[1])
        assert same_bits(info.cpu().numpy(), want_b[2])
    finally:
        ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
