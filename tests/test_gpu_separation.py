"""Pairwise separation and distinct-candidate selection on the device (include/gtop_separation.h; csrc/gtop_separation.hip)
through grad_traj_optimization_amd.separation.

(1) Device = twin (tests/separation_twin.py), bit for bit, for pair_min, pair_max and the row summaries: B on both
    sides of the pair kernel's 64-row tile, n_samples on both sides of its 8-sample chunk, m, shared and per-row T,
    every kind of start times, both kinds of ends, a row flown nowhere, random and scene coefficients.
(2) The known answers of tests/test_separation_twin.py through the device form and the host form.
(3) Laws on the device's output.  (4) The selection.  (5) Guard words, refusals, one graph."""
import ctypes as C

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from grad_traj_optimization_amd import separation as gs
from tests import scenes
from tests import separation_twin as sw
from tests import test_separation_twin as tw

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
GUARD = -12345.0
TILE, CHUNK = 64, 8          # the pair kernel's tile edge and sample chunk (csrc/gtop_separation.hip: kSepTile, kSepChunk)


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0", dtype=dtype)


bits, same_bits = tw.bits, tw.same_bits


@pytest.fixture(scope="module")
def ctx(gtop):
    """A context with a field, which the sampled report of the selection test needs (separation reads none): 24^3
    voxels of 0.5 m about the origin, every distance 10 m."""
    c = gtop.GtopContext(device=0)
    c.set_sdf(np.full((24, 24, 24), 10.0), (24, 24, 24), (-6.0, -6.0, -6.0), 0.5)
    yield c
    c.set_start_times(None)
    c.close()


def run_device(ctx, coeff, T, opts, t0=None):
    """(pair_min, pair_max, rows) as host arrays, under start times t0 (None, a scalar, or one per row)."""
    import torch
    ctx.set_start_times(t0)
    try:
        out = gs.separation_device(ctx, dev(coeff), dev(T), opts)
        torch.cuda.synchronize()
    finally:
        ctx.set_start_times(None)
    return tuple(o.cpu().numpy() for o in out)


def scene_rows(ctx, B, seed):
    """(coeff (B, 6, 18), T (B, 6)): the first seven waypoints of the opti_node scene, jittered per row, through
    gtop_coefficients_device."""
    import torch
    rng = np.random.default_rng(seed)
    wp = scenes.OPTI_NODE_PATH[None, :7] + rng.uniform(-0.4, 0.4, (B, 7, 3))
    T = problem.segment_times(wp)
    Df, Dp = problem.initial_derivatives(wp)
    x = Dp.reshape(B, -1) + rng.normal(0.0, 0.05, (B, Dp[0].size))
    coeff = ctx.coefficients_device(dev(x), dev(Df.reshape(B, 18)), dev(T))
    torch.cuda.synchronize()
    return coeff.cpu().numpy(), T


def start_times_of(kind, B, seed, nowhere=None):
    """None, one shared value, or one per row; row `nowhere` starts after the grid has ended."""
    if kind == "none":
        return None
    if kind == "one":
        return 0.375
    t0 = np.random.default_rng(seed).uniform(0.0, 1.0, B)
    if nowhere is not None:
        t0[nowhere] = 1000.0
    return t0


# (B, n_samples, m, shared T, start times, hold_ends, source, the row flown nowhere).  B: 1, 2, one below / at / one
# above the tile edge, two tiles plus 2; n_samples: 1, one below / at / one above the chunk, three chunks plus 1, and
# 16 400 and 5 480, past the sample kernel's grid; m: 2, 3, 13 (6 from the scene)
CASES = [
    (1, 1, 2, False, "none", False, "random", None),
    (2, CHUNK - 1, 3, True, "one", True, "random", None),
    (TILE - 1, CHUNK, 13, False, "rows", False, "random", None),
    (TILE, CHUNK + 1, 2, True, "rows", True, "random", None),
    (TILE + 1, 3 * CHUNK + 1, 3, False, "rows", False, "random", 17),
    (2 * TILE + 2, 3 * CHUNK + 1, 13, False, "rows", False, "random", 2 * TILE),
    (2 * TILE + 2, CHUNK + 1, 3, True, "none", False, "random", None),
    (2 * TILE + 2, 1, 2, False, "one", True, "random", None),
    (TILE + 1, 3 * CHUNK + 1, 6, False, "rows", False, "scene", None),
    (2 * TILE + 2, CHUNK, 6, False, "rows", True, "scene", 5),
    # the sample kernel's stride loop (csrc/gtop_sep_sample.h: more than 4096 blocks of 4 samples over the tiles), on one
    # tile of rows and on three with a padded last one: the edges of tests/swarm_limit_cases.py where pair_min and the
    # row summaries read the positions
    (3, 16400, 3, False, "rows", False, "random", None),
    (2 * TILE + 2, 5480, 3, False, "rows", False, "random", 2 * TILE),
]


@pytest.mark.parametrize("B,n,m,shared,t0kind,hold,source,nowhere", CASES)
def test_device_equals_twin_bit_for_bit(ctx, B, n, m, shared, t0kind, hold, source, nowhere):
    seed = 1000 + 7 * B + n
    if source == "scene":
        coeff, T = scene_rows(ctx, B, seed)
        dt = float(T.sum(axis=1).max()) / max(n - 1, 1)
    else:
        coeff, T = sw.random_rows(B, m, seed, shared_T=shared)
        dt = 0.8 * m / max(n - 1, 1)
    assert coeff.shape == (B, m, 18)
    t0 = start_times_of(t0kind, B, seed + 1, nowhere)
    radius = 1.0
    opts = gs.GtopSepOpts(t_lo=0.125, dt=dt, n_samples=n, radius=radius, hold_ends=hold)
    pmin, pmax, rows = run_device(ctx, coeff, T, opts, t0)
    want_min, want_max, want_rows = sw.separation(coeff, T, t0, 0.125, dt, n, hold_ends=hold, radius=radius)
    assert same_bits(pmin, want_min), np.argwhere(bits(pmin) != bits(want_min))[:5]
    assert same_bits(pmax, want_max), np.argwhere(bits(pmax) != bits(want_max))[:5]
    assert same_bits(rows, want_rows), (rows[:3], want_rows[:3])
    assert not tw.laws_fail(pmin, pmax)
    if nowhere is not None and not hold:
        assert rows[nowhere].tolist() == [np.inf, -1, -1, 0, 0, 0]
        assert np.all(pmin[nowhere] == np.inf) and np.all(pmax[:, nowhere] == -np.inf)
    if nowhere is not None and hold:            # held, it stands at its start through the whole grid
        assert rows[nowhere, 5] == n and rows[nowhere, 4] == B - 1
    if B > 2 and n > 1:
        assert np.isfinite(pmin).sum() > B and np.any(rows[:, 3] > 0)          # not vacuous


@pytest.mark.parametrize("name", ["head_on", "late_start", "late_start_held", "no_overlap"])
def test_known_answers_device_and_host_forms(ctx, name):
    """The rows of sw.known_rows() as a problem: Df and x that give exactly those coefficients (every number dyadic)."""
    import torch
    (kw, take), = [(kw, take) for case, kw, take, *_ in tw.known_answers() if case == name]
    want = [np.array(w, dtype=np.float64) for w in
            next(c[3:] for c in tw.known_answers() if c[0] == name)]
    known, T = sw.known_rows()
    Df = np.array([[[0, 1, 0, 4, 1, 0], [0] * 6, [0] * 6],
                   [[4, -1, 0, 0, -1, 0], [0.5, 0, 0, 0.5, 0, 0], [0] * 6],
                   [[8, 0, 0, 8, 0, 0]] * 3], dtype=np.float64)[take]
    x = np.array([[2, 1, 0, 0, 0, 0, 0, 0, 0], [2, -1, 0, 0.5, 0, 0, 0, 0, 0], [8, 0, 0] * 3], dtype=np.float64)[take]
    B = len(take)
    coeff = ctx.coefficients_device(dev(x), dev(Df.reshape(B, 18)), dev(T))
    torch.cuda.synchronize()
    assert np.array_equal(coeff.cpu().numpy(), known[take]), coeff.cpu().numpy()
    t0 = None if kw["t0"] is None else [kw["t0"][i] for i in take]
    opts = gs.GtopSepOpts(t_lo=0.0, dt=0.25, n_samples=17, radius=kw["radius"], hold_ends=kw["hold_ends"])
    got = run_device(ctx, coeff.cpu().numpy(), T, opts, t0)
    print(name, got)
    for g, w, what in zip(got, want, ("pair_min", "pair_max", "rows")):
        assert same_bits(g, w), (name, what, g, w)
    ctx.set_problem(T, Df)
    ctx.set_start_times(t0)
    try:
        host = gs.separation_batch(ctx, x, opts)
    finally:
        ctx.set_start_times(None)
    for h, g, what in zip(host, got, ("pair_min", "pair_max", "rows")):
        assert same_bits(h, g), (name, what, h, g)


def test_laws_and_independence_of_the_batch(ctx):
    B, m, n = 2 * TILE + 2, 3, 3 * CHUNK + 1
    coeff, T = sw.random_rows(B, m, 77)
    t0 = start_times_of("rows", B, 78)
    opts = gs.GtopSepOpts(t_lo=0.0, dt=0.1, n_samples=n, radius=0.75)
    pmin, pmax, rows = run_device(ctx, coeff, T, opts, t0)
    assert not tw.laws_fail(pmin, pmax)
    for i in range(B):
        others = np.delete(pmin[i], i)
        assert rows[i, 0] == others.min() and rows[i, 3] == np.count_nonzero(others < 0.75)
        assert rows[i, 4] == np.count_nonzero(np.isfinite(others))
    # pairs inside one tile, across two tiles, and in the ragged last tile, recomputed as batches of two
    for i, j in ((3, 40), (10, TILE + 5), (TILE - 1, TILE), (1, 2 * TILE + 1), (2 * TILE, 2 * TILE + 1)):
        two = [i, j]
        smin, smax, srows = run_device(ctx, coeff[two], T[two], opts, t0[two])
        assert same_bits(smin[0, 1], pmin[i, j]) and same_bits(smax[0, 1], pmax[i, j]), (i, j)
        assert same_bits(smin[1, 0], pmin[j, i]) and srows[0, 5] == rows[i, 5] and srows[1, 5] == rows[j, 5]
    # a permutation of the rows permutes the matrices
    perm = np.random.default_rng(79).permutation(B)
    qmin, qmax, qrows = run_device(ctx, coeff[perm], T[perm], opts, t0[perm])
    assert same_bits(qmin, pmin[np.ix_(perm, perm)]) and same_bits(qmax, pmax[np.ix_(perm, perm)])
    assert same_bits(qrows[:, [0, 2, 3, 4, 5]], rows[perm][:, [0, 2, 3, 4, 5]])
    # twice the same call: the same bits
    again = run_device(ctx, coeff, T, opts, t0)
    assert same_bits(again[0], pmin) and same_bits(again[1], pmax) and same_bits(again[2], rows)


def run_select(ctx, passed, cost, pair_max, gap, K):
    import torch
    p = None if passed is None else dev(passed, torch.uint8)
    chosen, count = gs.select_distinct_device(ctx, p, dev(cost), dev(pair_max), gap, K)
    torch.cuda.synchronize()
    return chosen.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("seed,B", [(21, 40), (22, 40), (23, 40), (24, 300), (25, 700)])
def test_selection_against_the_twin(ctx, seed, B):
    passed, cost, pair_max, gap, K = tw.selection_case(seed, B)
    assert np.isnan(cost).any() and np.isinf(cost).any()
    for p in (passed, None):                                            # d_pass = NULL: every row of finite cost
        chosen, count = run_select(ctx, p, cost, pair_max, gap, K)
        want, want_count = sw.select_distinct(p, cost, pair_max, gap, K)
        assert count == want_count and chosen.tolist() == want.tolist(), (chosen, want)
        assert sw.selection_faults(p, cost, pair_max, gap, K, chosen, count) == []
    # min_gap = 0 with every pair overlapping: the K cheapest passing rows in (cost, index) order
    open_max = np.where(np.isfinite(pair_max), pair_max, 1.0)
    eligible = np.flatnonzero((passed != 0) & np.isfinite(cost))
    order = eligible[np.lexsort((eligible, cost[eligible]))]
    for K2 in (1, 8, 64):
        chosen, count = run_select(ctx, passed, cost, open_max, 0.0, K2)
        k = min(K2, len(order))
        assert count == k and chosen.tolist() == order[:k].tolist() + [-1] * (K2 - k)
    # K larger than the number of eligible rows: the fill
    few = np.zeros_like(passed)
    few[order[:3]] = 1
    chosen, count = run_select(ctx, few, cost, open_max, 0.0, 8)
    assert count == 3 and chosen.tolist() == order[:3].tolist() + [-1] * 5
    # nothing eligible; a NaN gap entry fails the test
    chosen, count = run_select(ctx, np.zeros_like(passed), cost, open_max, 0.0, 4)
    assert count == 0 and chosen.tolist() == [-1] * 4
    nan_max = np.full_like(open_max, np.nan)
    chosen, count = run_select(ctx, passed, cost, nan_max, 0.0, 4)
    assert count == 1 and chosen.tolist() == [int(order[0]), -1, -1, -1]


def test_selection_on_a_report_and_an_empty_batch(gtop, ctx):
    """chosen[0] is best[0] of select_best_device on the same report and cost; the separation's own pair_max feeds the
    selection; B = 0."""
    import torch
    B = TILE + 1
    coeff, T = scene_rows(ctx, B, 91)
    c, t = dev(coeff), dev(T)
    lim = gtop.GtopLimits(allow_out_of_map=True)
    rep = ctx.validate_device(c, t, lim, dt_sample=0.01)
    cost_h = np.random.default_rng(92).integers(0, 9, B).astype(np.float64)
    cost_h[[0, 7, 20, 33, TILE]] = np.inf                                # rows that cannot pass: the selection wants a cost
    cost = dev(cost_h)
    ok, best = ctx.select_best_device(rep, cost, lim)
    opts = gs.GtopSepOpts(t_lo=0.0, dt=float(T.sum(axis=1).max()) / 31, n_samples=32, hold_ends=True)
    _, pmax, _ = gs.separation_device(ctx, c, t, opts)
    chosen, count = gs.select_distinct_device(ctx, ok, cost, pmax, 0.3, 6)
    torch.cuda.synchronize()
    okh, pm = ok.cpu().numpy(), pmax.cpu().numpy()
    print("passing", best.tolist(), "chosen", chosen.tolist())
    assert 0 < best[1].item() < B and chosen[0].item() == best[0].item()
    want, want_count = sw.select_distinct(okh, cost.cpu().numpy(), pm, 0.3, 6)
    assert count.item() == want_count >= 2 and chosen.cpu().numpy().tolist() == want.tolist()
    picked = chosen.cpu().numpy()[:want_count]
    sub = pm[np.ix_(picked, picked)]
    assert np.all(sub[~np.eye(want_count, dtype=bool)] >= 0.3) and np.all(okh[picked] != 0)
    # B = 0: count 0 and every entry -1; the separation launches nothing
    e = torch.empty(0, dtype=torch.float64, device=c.device)
    ch0 = torch.full((5,), 7, dtype=torch.int32, device=c.device)
    n0 = torch.full((1,), 7, dtype=torch.int32, device=c.device)
    gs.select_distinct_device(ctx, None, e, e.reshape(0, 0), 0.0, 5, chosen=ch0, count=n0)
    torch.cuda.synchronize()
    assert ch0.tolist() == [-1] * 5 and n0.tolist() == [0]
    p0, q0, r0 = gs.separation_device(ctx, e.reshape(0, 3, 18), e.reshape(0, 3), opts)
    assert p0.shape == (0, 0) and q0.shape == (0, 0) and r0.shape == (0, 6)


def test_guard_words_around_every_output_and_the_workspace(ctx):
    import torch
    B, m, n = TILE + 1, 3, CHUNK + 1
    coeff, T = sw.random_rows(B, m, 55)
    opts = gs.GtopSepOpts(t_lo=0.0, dt=0.2, n_samples=n, radius=1.0)
    f64 = dict(dtype=torch.float64, device="cuda:0")
    mats = [torch.full((B * B + 16,), GUARD, **f64) for _ in range(2)]
    rbuf = torch.full((B * 6 + 16,), GUARD, **f64)
    need = gs.separation_workspace_bytes(B, n)
    wbuf = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    views = [b[8:-8].reshape(B, B) for b in mats] + [rbuf[8:-8].reshape(B, 6)]
    gs.separation_device(ctx, dev(coeff), dev(T), opts, *views, work=wbuf[128:128 + need])
    torch.cuda.synchronize()
    for buf in (*mats, rbuf):
        assert torch.all(buf[:8] == GUARD) and torch.all(buf[-8:] == GUARD) and not torch.any(buf[8:-8] == GUARD)
    assert torch.all(wbuf[:128] == 0xA5) and torch.all(wbuf[128 + need:] == 0xA5)
    want = sw.separation(coeff, T, None, 0.0, 0.2, n, radius=1.0)
    for v, w in zip(views, want):
        assert same_bits(v.cpu().numpy(), w)
    # the selection's outputs
    cost = dev(np.arange(B, 0, -1.0))
    cbuf = torch.full((8 + 4,), 7, dtype=torch.int32, device="cuda:0")
    nbuf = torch.full((3,), 7, dtype=torch.int32, device="cuda:0")
    gs.select_distinct_device(ctx, None, cost, views[1].contiguous(), 0.0, 8, chosen=cbuf[2:10], count=nbuf[1:2])
    torch.cuda.synchronize()
    assert cbuf[:2].tolist() == [7, 7] and cbuf[10:].tolist() == [7, 7] and nbuf.tolist() == [7, 8, 7]
    assert cbuf[2:10].tolist() == list(range(B - 1, B - 9, -1))


def test_refusals_launch_nothing(gtop, ctx):
    import torch
    B, m, n = 3, 3, 9
    coeff, T = sw.random_rows(B, m, 5)
    c, t = dev(coeff), dev(T)
    f64 = dict(dtype=torch.float64, device=c.device)
    pmin, pmax, rows = torch.full((B, B), GUARD, **f64), torch.full((B, B), GUARD, **f64), torch.full((B, 6), GUARD, **f64)
    need = gs.separation_workspace_bytes(B, n)
    work = torch.full((need,), 0xA5, dtype=torch.uint8, device=c.device)
    L, h = gs.sep_library(), ctx._h
    good = gs.GtopSepOpts(t_lo=0.0, dt=0.25, n_samples=n, radius=1.0)

    def refused(code, fn):
        with pytest.raises(gtop.GtopError) as ei:
            fn()
        assert ei.value.code == code, ei.value

    o = lambda **kw: gs.GtopSepOpts(**{**dict(t_lo=0.0, dt=0.25, n_samples=n, radius=1.0), **kw})
    bad_opts = [o(t_lo=np.nan), o(t_lo=np.inf), o(dt=np.nan), o(dt=np.inf), o(dt=0.0), o(dt=-0.25), o(n_samples=0),
                o(n_samples=65537), o(n_samples=-1), o(reserved=(1, 0)), o(reserved=(0, 1))]
    for hold in (2, -1):
        b = o()
        b.hold_ends = hold
        bad_opts.append(b)
    for bad in bad_opts:
        refused(ERR_INVALID, lambda: gs.separation_device(ctx, c, t, bad, pmin, pmax, rows, work=work))
    vp = lambda a: a.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (
        ("B", B), ("m", m), ("coeff", vp(c)), ("T", vp(t)), ("stride", m), ("opt", good), ("pmin", vp(pmin)),
        ("pmax", vp(pmax)), ("rows", vp(rows)), ("work", vp(work)), ("bytes", need), ("stream", None))]
    for kw in (dict(opt=None), dict(B=-1), dict(B=4097), dict(m=1), dict(m=228), dict(stride=1), dict(stride=m + 1),
               dict(coeff=None), dict(T=None), dict(pmin=None), dict(pmax=None), dict(rows=None), dict(work=None),
               dict(bytes=need - 1), dict(bytes=0)):
        assert L.gtop_separation_device(h, *args(**kw)) == ERR_INVALID, kw
    # a start-time count that is not 0, 1 or B
    ctx.set_start_times([0.0, 1.0])
    try:
        refused(ERR_INVALID, lambda: gs.separation_device(ctx, c, t, good, pmin, pmax, rows, work=work))
    finally:
        ctx.set_start_times(None)
    # a NaN radius is "none counted", not refused
    got = gs.separation_device(ctx, c, t, o(radius=np.nan))
    off = gs.separation_device(ctx, c, t, o(radius=0.0))
    assert all(torch.equal(a, b) for a, b in zip(got, off)) and torch.all(got[2][:, 3] == 0)
    # the host form: no problem, then too many rows, bad options, missing buffers
    x = np.zeros((B, 9 * (m - 1)))
    bare = gtop.GtopContext(device=0)
    try:
        refused(ERR_STATE, lambda: gs.separation_batch(bare, x, good))
    finally:
        bare.close()
    ctx.set_problem(np.asarray(T), np.zeros((B, 3, 6)))
    refused(ERR_INVALID, lambda: gs.separation_batch(ctx, np.tile(x, (2, 1)), good))
    refused(ERR_INVALID, lambda: gs.separation_batch(ctx, x, bad_opts[0]))
    dp = lambda a: a.ctypes.data_as(gs._dp)
    hm, hx, hr = np.full((B, B), GUARD), np.full((B, B), GUARD), np.full((B, 6), GUARD)
    assert L.gtop_separation_batch(h, 0, dp(x), good, dp(hm), dp(hx), dp(hr)) == ERR_INVALID
    assert L.gtop_separation_batch(h, B, None, good, dp(hm), dp(hx), dp(hr)) == ERR_INVALID
    assert L.gtop_separation_batch(h, B, dp(x), None, dp(hm), dp(hx), dp(hr)) == ERR_INVALID
    assert L.gtop_separation_batch(h, B, dp(x), good, None, dp(hx), dp(hr)) == ERR_INVALID
    assert L.gtop_separation_batch(h, B, dp(x), good, dp(hm), None, dp(hr)) == ERR_INVALID
    assert L.gtop_separation_batch(h, B, dp(x), good, dp(hm), dp(hx), None) == ERR_INVALID
    assert np.all(hm == GUARD) and np.all(hx == GUARD) and np.all(hr == GUARD)
    # the selection
    cost = torch.zeros(B, **f64)
    ok = torch.ones(B, dtype=torch.uint8, device=c.device)
    pm = torch.ones(B, B, **f64)
    chosen = torch.full((4,), 7, dtype=torch.int32, device=c.device)
    count = torch.full((1,), 7, dtype=torch.int32, device=c.device)
    sel = lambda **kw: [kw.get(k, v) for k, v in (
        ("B", B), ("pass", vp(ok)), ("cost", vp(cost)), ("pm", vp(pm)), ("gap", 0.0), ("K", 4), ("chosen", vp(chosen)),
        ("count", vp(count)), ("stream", None))]
    for kw in (dict(K=0), dict(K=65), dict(K=-1), dict(gap=np.nan), dict(gap=np.inf), dict(gap=-np.inf), dict(B=-1),
               dict(B=4097), dict(cost=None), dict(pm=None), dict(chosen=None), dict(count=None)):
        assert L.gtop_select_distinct_device(h, *sel(**kw)) == ERR_INVALID, kw
    torch.cuda.synchronize()
    assert all(torch.all(b == GUARD) for b in (pmin, pmax, rows)) and torch.all(work == 0xA5)
    assert chosen.tolist() == [7] * 4 and count.tolist() == [7]


def test_one_graph_replays_to_the_eager_bits(ctx):
    """coefficients -> separation -> selection, captured once as a linear graph; the start times are read at replay."""
    import torch
    B, K = TILE + 1, 6
    rng = np.random.default_rng(303)
    wp = scenes.OPTI_NODE_PATH[None, :7] + rng.uniform(-0.4, 0.4, (B, 7, 3))
    T = problem.segment_times(wp)
    Df, Dp = problem.initial_derivatives(wp)
    x = dev(Dp.reshape(B, -1) + rng.normal(0.0, 0.05, (B, Dp[0].size)))
    Dfd, Td = dev(Df.reshape(B, 18)), dev(T)
    n = 3 * CHUNK + 1
    opts = gs.GtopSepOpts(t_lo=0.0, dt=float(T.sum(axis=1).max()) / (n - 1), n_samples=n, radius=0.5)
    f64 = dict(dtype=torch.float64, device=x.device)
    coeff = torch.empty(B, 6, 18, **f64)
    pmin, pmax, rows = torch.zeros(B, B, **f64), torch.zeros(B, B, **f64), torch.zeros(B, 6, **f64)
    work = torch.zeros(gs.separation_workspace_bytes(B, n), dtype=torch.uint8, device=x.device)
    cost = dev(rng.integers(0, 9, B).astype(np.float64))
    chosen = torch.zeros(K, dtype=torch.int32, device=x.device)
    count = torch.zeros(1, dtype=torch.int32, device=x.device)
    t0_a, t0_b = rng.uniform(0.0, 1.0, B), rng.uniform(0.0, 2.0, B)
    t0 = dev(t0_a)
    ctx.set_start_times_device(t0)

    def chain():
        ctx.coefficients_device(x, Dfd, Td, coeff=coeff)
        gs.separation_device(ctx, coeff, Td, opts, pmin, pmax, rows, work=work)
        gs.select_distinct_device(ctx, None, cost, pmax, 0.3, K, chosen=chosen, count=count)

    outs = (coeff, pmin, pmax, rows, chosen, count)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # warm-up outside the capture
            chain()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        eager_a = [o.clone() for o in outs]
        want = sw.separation(coeff.cpu().numpy(), T, t0_a, 0.0, opts.dt, n, radius=0.5)
        assert all(same_bits(e.cpu().numpy(), w) for e, w in zip(eager_a[1:4], want))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager_a):
            assert torch.equal(o, e)
        # the start-time buffer rewritten in place: the replay gives the bits of an eager run with the new times
        t0.copy_(dev(t0_b))
        graph.replay()
        torch.cuda.synchronize()
        replay_b = [o.clone() for o in outs]
        chain()
        torch.cuda.synchronize()
        for o, e in zip(outs, replay_b):
            assert torch.equal(o, e)
        want_b = sw.separation(coeff.cpu().numpy(), T, t0_b, 0.0, opts.dt, n, radius=0.5)
        assert all(same_bits(e.cpu().numpy(), w) for e, w in zip(replay_b[1:4], want_b))
        assert not torch.equal(replay_b[1], eager_a[1])
    finally:
        ctx.set_start_times_device(None)
