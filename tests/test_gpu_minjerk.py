"""The minimum-jerk start point on the device (gtop_min_jerk_start_device / gtop_min_jerk_start, csrc/gtop_minjerk.hip)
against the exact arithmetic of tests/minjerk_twin.py.

THE VALUE CRITERION.  For every checked trajectory, axis and unknown row i, with the device's u taken as rationals, the
exact residual r_i = sum_j K_ij u_j + c_i satisfies |r_i| <= 2^12 * 2^-53 * mag_i, mag_i = sum_j |K_ij u_j| + the
magnitudes of the row's known terms (position terms on the exact waypoint differences).  2^12 u is this project's
entrywise standard (tests/test_gpu_entrywise.py); a plain numpy elimination stays below 11 u on the same inputs
(tests/test_minjerk_twin.py).

Worst ratio |r_i| / (u mag_i) seen on the MI355X over every case below: 6.9 (m = 171, T in [0.05, 8], per-trajectory
times); m = 2: 2.0, m = 13: 2.9, m = 64: 4.3, m = 227: 4.7 — against the bound of 4096."""
import ctypes as C

import numpy as np
import pytest

from tests import minjerk_plan
from tests import minjerk_twin as mt

pytestmark = pytest.mark.gpu

GUARD = 64                      # doubles in front of and behind x
GUARD_VALUE = -1234.5678
OK, ERR_INVALID, ERR_STATE = 0, 1, 4


@pytest.fixture(scope="module")
def ctx(gtop):
    c = gtop.GtopContext(device=0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _batch(base, B, shared):
    """Row b of the batch = base row b mod 4 (T one shared vector when `shared`)."""
    T4, Df4, x4 = base
    idx = np.arange(B) % mt.BASE_ROWS
    return (T4[0].copy() if shared else T4[idx].copy()), Df4[idx].copy(), x4[idx].copy()


def _run(ctx, T, Df, x, stream=None):
    """x through the device form with guard words on both sides; returns the new x (numpy) after checking that the
    guards, Df and T are untouched."""
    import torch
    dev = torch.device("cuda:0")
    B, n = x.shape
    buf = torch.full((2 * GUARD + B * n,), GUARD_VALUE, dtype=torch.float64, device=dev)
    xt = buf[GUARD:GUARD + B * n].view(B, n)
    xt.copy_(torch.tensor(x, device=dev))
    Dft, Tt = torch.tensor(Df, device=dev), torch.tensor(T, device=dev)
    torch.cuda.synchronize()
    ctx.min_jerk_start_device(xt, Dft, Tt, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.all(out[:GUARD] == GUARD_VALUE) and np.all(out[GUARD + B * n:] == GUARD_VALUE), "guard words written"
    assert np.array_equal(_bits(Dft.cpu().numpy()), _bits(Df)) and np.array_equal(_bits(Tt.cpu().numpy()), _bits(T))
    return out[GUARD:GUARD + B * n].reshape(B, n).copy()


def _positions(m, x):
    return np.asarray(x).reshape(-1, 3, m - 1, 3)[:, :, :, 0]


def test_segment_counts_straddle_every_switch_of_the_plan():
    lanes = {m: p["lanes"] for m, p in zip(mt.SEGMENTS, minjerk_plan.plans([(1, m) for m in mt.SEGMENTS]))}
    assert (lanes[43], lanes[44], lanes[86], lanes[87], lanes[171], lanes[172]) == (64, 32, 32, 16, 16, 8)
    every = minjerk_plan.plans([(1, m) for m in range(2, 228)])
    switches = [p["m"] for prev, p in zip(every, every[1:]) if p["lanes"] != prev["lanes"]]
    assert all(m in mt.SEGMENTS and m - 1 in mt.SEGMENTS for m in switches) and len(switches) == 3


@pytest.mark.parametrize("m,t_range,shared", mt.cases())
def test_value_criterion_and_row_independence(ctx, m, t_range, shared):
    """B in {1, 3, 65, 130}; rows 0, 63, 64 and B - 1 are held to the value criterion exactly, every row from the
    fifth on equals the row whose inputs it repeats bit for bit (its index, the batch and the workgroup it falls in do
    not matter), positions / Df / T / guard words are untouched.  The shared-time cases run on a stream of their own.

    Worst ratio seen on the MI355X: 6.9, in the case (171, "wide", False); every case prints its own with -s."""
    import torch
    base = mt.base_rows(m, t_range, shared)
    stream = torch.cuda.Stream() if shared else None
    worst = 0.0
    first = None
    for B in mt.BATCHES:
        T, Df, x = _batch(base, B, shared)
        out = _run(ctx, T, Df, x, stream=stream)
        assert np.array_equal(_bits(_positions(m, out)), _bits(_positions(m, x))), "a position entry changed"
        assert np.all(np.isfinite(out))
        for b in range(mt.BASE_ROWS, B):
            assert np.array_equal(_bits(out[b]), _bits(out[b % mt.BASE_ROWS])), (B, b)
        if first is None:
            first = out[0].copy()
        assert np.array_equal(_bits(out[0]), _bits(first)), "row 0 depends on the batch"
        for b in sorted({0, 63, 64, B - 1}):
            if b < B:
                Tb = T if shared else T[b]
                worst = max(worst, mt.worst_ratio(Tb, Df[b], x[b], out[b]))
    print(f"m = {m} {t_range} shared = {shared}: worst |r| / (u mag) = {worst:.1f}")
    assert worst <= mt.BOUND_K


@pytest.mark.parametrize("m", [2, 6, 13])
def test_analytic_constant_velocity(ctx, m):
    """tests/golden/MINJERK_ANALYTIC.md: v_k = (3, 0, 0), a_k = 0, to 2^12 u kappa_inf(K) 3."""
    T, Df, x_in, x_want = mt.analytic(m)
    out = _run(ctx, T[None], Df[None], x_in[None])[0]
    K = np.array([[float(v) for v in row] for row in mt.dense(T)])
    kappa = np.linalg.cond(K, np.inf)
    bound = 2.0 ** 12 * 2.0 ** -53 * kappa * 3.0
    err = float(np.max(np.abs(out - x_want)))
    print(f"m = {m}: kappa_inf = {kappa:.3g}, max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("m", [2, 3, 6])
def test_minimum_of_the_librarys_own_cost(gtop, m):
    """With ws = 1, wc = 0 the evaluation's cost is the smoothness term: at the result it is strictly less than at
    x +- 2^-10 e_i for every velocity and acceleration entry i."""
    import torch
    from grad_traj_optimization_amd import problem
    dev = torch.device("cuda:0")
    c = gtop.GtopContext(device=0, params=dict(ws=1.0, wc=0.0))
    try:
        mp = problem.make_map((24, 24, 12), density=0.02, seed=5)
        c.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        c.update_sdf_map(mp.obstacle_points())
        T4, Df4, x4 = mt.base_rows(m, "narrow", False)
        xs = torch.tensor(x4[1:2], device=dev)
        Df, T = torch.tensor(Df4[1:2], device=dev), torch.tensor(T4[1:2], device=dev)
        c.min_jerk_start_device(xs, Df, T)
        n = 9 * (m - 1)
        va = [i for i in range(n) if i % 3 != 0]
        rows = xs.repeat(1 + 2 * len(va), 1)
        for r, i in enumerate(va):
            rows[1 + 2 * r, i] += 2.0 ** -10
            rows[2 + 2 * r, i] -= 2.0 ** -10
        B = rows.shape[0]
        cost, _ = c.eval_device(rows.contiguous(), Df.repeat(B, 1).contiguous(), T.repeat(B, 1).contiguous())
        torch.cuda.synchronize()
        cost = cost.cpu().numpy()
        assert np.all(np.isfinite(cost)) and np.all(cost[1:] > cost[0]), (cost[0], cost[1:].min())
        print(f"m = {m}: cost {cost[0]:.6g}, least increase {cost[1:].min() - cost[0]:.3g}")
    finally:
        c.close()


def test_host_form_and_refusals(gtop, ctx):
    import torch
    dev = torch.device("cuda:0")
    m, B = 6, 65
    n = 9 * (m - 1)
    T, Df, x = _batch(mt.base_rows(m, "wide", False), B, False)
    want = _run(ctx, T, Df, x)
    h = gtop.GtopContext(device=0)
    L = gtop.load_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    try:
        keep = x.copy()
        assert L.gtop_min_jerk_start(h._h, 1, dp(keep)) == ERR_STATE           # no problem set
        assert np.array_equal(_bits(keep), _bits(x))
        h.set_problem(T, Df)
        got = h.min_jerk_start(x)
        assert got is not x and np.array_equal(_bits(got), _bits(want)), "host form differs from the device form"
        assert np.array_equal(_bits(h.min_jerk_start(x)), _bits(want)), "a repeated call differs"
        assert np.array_equal(_bits(h.min_jerk_start(x[:3])), _bits(want[:3]))   # the first B rows of the problem
        for bad_B in (0, -1, B + 1):
            assert L.gtop_min_jerk_start(h._h, bad_B, dp(keep)) == ERR_INVALID
        assert L.gtop_min_jerk_start(h._h, B, None) == ERR_INVALID
        assert np.array_equal(_bits(keep), _bits(x))
        # the device form: refusals launch nothing, B = 0 succeeds and leaves x as it was
        xt, Dft, Tt = (torch.tensor(a, device=dev) for a in (x, Df, T))
        vp = lambda t: C.c_void_p(t.data_ptr())
        call = lambda B_, m_, px, pd, pt, stride: L.gtop_min_jerk_start_device(h._h, B_, m_, px, pd, pt, stride, None)
        assert call(0, m, vp(xt), vp(Dft), vp(Tt), m) == OK
        assert call(-1, m, vp(xt), vp(Dft), vp(Tt), m) == ERR_INVALID
        for bad_m in (1, 0, 228):
            assert call(B, bad_m, vp(xt), vp(Dft), vp(Tt), bad_m) == ERR_INVALID
        assert call(B, m, vp(xt), vp(Dft), vp(Tt), 3) == ERR_INVALID
        assert call(B, m, None, vp(Dft), vp(Tt), m) == ERR_INVALID
        assert call(B, m, vp(xt), None, vp(Tt), m) == ERR_INVALID
        assert call(B, m, vp(xt), vp(Dft), None, m) == ERR_INVALID
        torch.cuda.synchronize()
        assert np.array_equal(_bits(xt.cpu().numpy()), _bits(x))
    finally:
        h.close()


def test_zero_segment_time_stays_in_its_row(ctx):
    m, B = 6, 5
    T, Df, x = _batch(mt.base_rows(m, "narrow", False), B, False)
    want = _run(ctx, T, Df, x)
    T0 = T.copy()
    T0[2, 3] = 0.0
    with np.errstate(all="ignore"):
        got = _run(ctx, T0, Df, x)
    others = [0, 1, 3, 4]
    assert np.array_equal(_bits(got[others]), _bits(want[others]))
    assert np.array_equal(_bits(_positions(m, got)), _bits(_positions(m, x)))
    va = np.asarray(got[2]).reshape(3, m - 1, 3)[:, :, 1:]
    assert not np.any(np.isfinite(va)), va


def test_captured_launch_follows_the_positions(ctx):
    import torch
    dev = torch.device("cuda:0")
    m, B = 7, 65
    T, Df, x = _batch(mt.base_rows(m, "narrow", True), B, True)
    x2 = _batch(mt.base_rows(m, "wide", False), B, False)[2]
    Dft, Tt = torch.tensor(Df, device=dev), torch.tensor(T, device=dev)
    want = [ctx.min_jerk_start_device(torch.tensor(v, device=dev), Dft, Tt).clone() for v in (x, x2)]   # eager (and warm)
    torch.cuda.synchronize()
    assert not torch.equal(want[0], want[1])
    xg = torch.tensor(x, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.min_jerk_start_device(xg, Dft, Tt)
    for k in (1, 0, 1):
        xg.copy_(torch.tensor((x, x2)[k], device=dev))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, want[k]), k
