"""tests/time_moving_twin.py — the numpy restatement of include/gtop_time_moving.h — against what it restates: its
cost is the evaluation twins' (moving_twin, box_poly_twin), gT and gt0 are the derivatives of that cost (central
differences on a smooth time-dependent field; the pass's mutants miss), the box lookup's time derivative is the
derivative of the C oracle's evaluateEDTWithGrad in tau (the lookup's mutants miss), the hand-derived case of
tests/golden/TIME_MOVING_ANALYTIC.md, and the optimizer's laws."""
import math

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import box_poly_twin
from tests import consistent_twin as ct
from tests import moving_twin
from tests import time_moving_twin as tm
from tests import time_twin as tt
from tests.test_consistent_gradient import DYN, PARAMS, _fd_path, _scene

MODES = [dict(), DYN, dict(DYN, step=1)]
IDS = ["plain", "dyn", "dyn-step1"]


def scene_boxes(b, seed, nbox=3):
    """Constant-velocity boxes that start at waypoints of the rows and drift: some samples of most rows are lowered."""
    rng = np.random.default_rng(seed)
    B, m = b.x.shape[0], b.m
    wp = b.x.reshape(B, 3, m - 1, 3)[:, :, :, 0]                      # (B, axis, waypoint)
    rows = rng.integers(0, B, nbox)
    p0 = np.stack([wp[r, :, rng.integers(0, m - 1)] for r in rows]) + rng.uniform(-0.3, 0.3, (nbox, 3))
    vel = rng.uniform(-0.4, 0.4, (nbox, 3))
    scale = rng.uniform(0.4, 1.2, (nbox, 3))
    return p0, vel, scale


@pytest.mark.parametrize("extra", MODES, ids=IDS)
def test_cost_is_the_evaluation_twins(oracle_mod, extra):
    """The pass's cost against moving_twin.cost_grad's and box_poly_twin.cost_grad's on random maps, with shared and
    per-row start times: 1e-12, the bound tests/test_time_twin.py holds time_twin to against consistent_twin."""
    b, sdf = _scene(oracle_mod, B=6)
    p = dict(PARAMS, **extra)
    p0, vel, scale = scene_boxes(b, 5)
    when = np.array([0.4, 0.9, 1.3])
    coef = box_poly_twin.coefficients(p0 + vel * when[:, None], vel, np.full((3, 3), 0.2), when)
    t_range = np.array([[0.2, 1.4], [0.0, 2.5], [0.5, 9.0]])
    worst, n_low = 0.0, 0
    for i in range(len(b.x)):
        t0 = 0.3 * i
        c_ref, _, info = moving_twin.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, p, p0, vel, scale, t0)
        c, gT, gt0, parts, low = tm.cost_gradT(b.T[i], b.Df[i], b.x[i], tm.BoxLookup(sdf, p0, vel, scale), p, t0)
        worst = max(worst, abs(c - c_ref) / abs(c_ref))
        n_low += int(low.any())
        assert low.any() == info["lowered"].any()
        c_ref, _, _ = box_poly_twin.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, p, coef, scale, t_range, t0)
        c, gT, gt0, parts, _ = tm.cost_gradT(b.T[i], b.Df[i], b.x[i], tm.PolyBoxLookup(sdf, coef, scale, t_range), p, t0)
        worst = max(worst, abs(c - c_ref) / abs(c_ref))
        # the laws of the parts
        assert abs((parts[:, 0].sum() + parts[:, 1].sum() + 1e-3) - c) <= 1e-13 * abs(c)
        assert np.array_equal(gT, (parts[:, 2] + parts[:, 3]) + parts[:, 5]) and np.all(np.isfinite(parts))
        assert parts[-1, 5] == 0.0 and gt0 == parts[0, 5] + parts[0, 4]
        assert np.array_equal(parts[:-1, 5], np.cumsum(parts[::-1, 4])[::-1][1:])
    print(f"cost against the evaluation twins: {worst:.2e}; rows with box-lowered samples: {n_low}")
    assert worst <= 1e-12 and n_low >= 3


def test_static_lookup_gives_the_static_twin(oracle_mod):
    """No time dependence: time_twin's numbers, the added columns 0."""
    b, sdf = _scene(oracle_mod, B=2)
    c0, g0, p0 = tt.cost_gradT(b.T[0], b.Df[0], b.x[0], sdf, PARAMS)
    c, g, gt0, parts, _ = tm.cost_gradT(b.T[0], b.Df[0], b.x[0], tm.StaticLookup(sdf), PARAMS, t0=0.7)
    assert c == c0 and np.array_equal(g, g0) and np.array_equal(parts[:, :4], p0)
    assert gt0 == 0.0 and np.all(parts[:, 4:] == 0.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("extra", [dict(), DYN, dict(DYN, alpha=0.0)], ids=["plain", "dyn", "dyn-alpha0"])
def test_gT_and_gt0_are_the_derivatives_of_the_cost_and_the_mutants_are_not(monkeypatch, extra, seed):
    """Central differences in T and in t0 (h = 1e-6) of the evaluation twin's cost — consistent_twin.cost_grad over the
    lookup at moving_twin's sample times — with the float round trips switched off, on a plane that moves along its
    normal with a speed that changes in time: within 1e-5 of the max-norm (the bound of tests/test_time_twin.py, for
    its reason: the 1e-5 of vel_norm biases one term by 1e-5/|v|).  With alpha = 0 the lookup carries no weight and
    nothing of the pass's mutants is live; in the two modes where the collision term is live each of them misses the
    bound by ten times."""
    monkeypatch.setattr(ct, "to_float", lambda v: v)
    T, Df, x = _fd_path(4, seed)
    p = dict(PARAMS, **extra)
    plane, t0, h = tm.MovingPlane(), 0.35, 1e-6
    fd = np.zeros(len(T) + 1)
    for s in range(len(T)):
        Tp, Tm = T.copy(), T.copy()
        Tp[s] += h
        Tm[s] -= h
        fd[s] = (tm.eval_cost(Tp, Df, x, plane, p, t0) - tm.eval_cost(Tm, Df, x, plane, p, t0)) / (2 * h)
    fd[-1] = (tm.eval_cost(T, Df, x, plane, p, t0 + h) - tm.eval_cost(T, Df, x, plane, p, t0 - h)) / (2 * h)
    scale = np.max(np.abs(fd[:-1]))
    _, gT, gt0, _, _ = tm.cost_gradT(T, Df, x, plane, p, t0)
    dev = np.max(np.abs(np.r_[gT, gt0] - fd)) / scale
    print(f"central differences in T and t0: off by {dev:.2e} of the max-norm (gt0 {gt0:.3e} against {fd[-1]:.3e})")
    assert dev <= 1e-5, dev
    for mutant in tm.PASS_MUTANTS:
        _, gm, g0m, _, _ = tm.cost_gradT(T, Df, x, plane, p, t0, mutant=mutant)
        off = np.max(np.abs(np.r_[gm, g0m] - fd)) / scale
        print(f"  mutant {mutant}: off by {off:.2e}")
        if p["alpha"] != 0.0:
            assert off >= 1e-4, (mutant, off)
        else:
            assert off <= 1e-5, (mutant, off)


def _near_box_points(rng, centre, scale, n, reach=1.5):
    """Points within `reach` of the surface of the box (outside it, or inside near a face)."""
    half = 0.5 * scale
    pts = centre + rng.uniform(-(half + reach), half + reach, (n, 3))
    return pts


DTAU_BOUND, DTAU_H, NEAR = 1e-7, 1e-6, 1e-4


@pytest.mark.parametrize("kind", ["const_vel", "polynomial"])
@pytest.mark.parametrize("obstacles", [False, True], ids=["empty", "obstacles"])
def test_box_lookup_dtau_is_the_derivative_of_the_oracles_lookup(oracle_mod, kind, obstacles):
    """dtau against central differences in tau (h = 1e-6) of the C oracle's evaluateEDTWithGrad
    (box_poly_twin.edt_query for a polynomial list), at points within 1.5 m of a box's surface: 1e-7 absolute —
    rounding gives u |d| / h ~ 1e-9 and truncation less, two orders of headroom.  A point is left out only where the
    derivative has a jump within reach of h: a corner coordinate within 1e-4 m of a box face, a static / box tie within
    1e-4 m, a polynomial's t1 or t2 within 1e-4 s.  The boxes stand far enough apart that no two of them reach the
    same corner.  Both lookup mutants miss the bound by ten times."""
    mp = problem.make_map((48, 40, 24), density=0.04 if obstacles else 0.0, seed=31)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    lo, size = np.asarray(mp.origin), np.asarray(mp.map_size)
    rng = np.random.default_rng(77 + obstacles)
    # three boxes on a diagonal of the map, 3.5 m apart at least for the whole of the times drawn
    frac = np.array([[0.22, 0.25, 0.3], [0.5, 0.55, 0.6], [0.78, 0.8, 0.35]])
    p0 = lo + frac * size
    vel = np.array([[0.3, -0.2, 0.1], [-0.25, 0.3, -0.1], [0.2, 0.25, 0.15]])
    scale = np.array([[0.6, 0.9, 0.5], [1.0, 0.4, 0.7], [0.5, 0.5, 0.9]])
    if kind == "polynomial":
        acc = np.array([[0.1, 0.0, -0.1], [0.0, -0.15, 0.1], [-0.1, 0.1, 0.0]])
        coef = box_poly_twin.coefficients(p0, vel, acc, np.zeros(3))
        coef[:, :, 3] = 0.01 * rng.standard_normal((3, 3))
        t_range = np.array([[0.3, 1.1], [0.0, 0.8], [0.6, 5.0]])

        def make(mutant=None):
            return tm.PolyBoxLookup(sdf, coef, scale, t_range, mutant)

        def oracle_dist(pos, tau):
            return box_poly_twin.edt_query(sdf, pos, tau, coef, scale, t_range)[0][0]
    else:
        def make(mutant=None):
            return tm.BoxLookup(sdf, p0, vel, scale, mutant)

        def oracle_dist(pos, tau):
            return sdf.edt_query(pos, tau, p0, vel, scale)[0][0]
    look, mutants = make(), {m: make(m) for m in tm.LOOKUP_MUTANTS}
    n, left_out, compared, live, worst = 0, 0, 0, 0, 0.0
    miss = {m: 0.0 for m in mutants}
    for _ in range(220):
        for b in range(3):
            tau = float(rng.uniform(0.05, 1.5))
            centre = look.boxes_at(tau)[0][b]
            pos = _near_box_points(rng, centre, scale[b], 1)[0]
            pos = np.clip(pos, lo + 0.3, lo + size - 0.3)
            n += 1
            d, g, dtau = look.query(pos, tau)
            mg = look.margins
            if mg["face"] < NEAR or mg["tie"] < NEAR or mg["time"] < NEAR:
                left_out += 1
                continue
            fd = (oracle_dist(pos, tau + DTAU_H) - oracle_dist(pos, tau - DTAU_H)) / (2 * DTAU_H)
            assert d == oracle_dist(pos, tau)
            worst = max(worst, abs(dtau - fd))
            compared += 1
            live += bool(look.lowered and np.any(look.dcorner != 0.0) and dtau != 0.0)
            for name, mut in mutants.items():
                miss[name] = max(miss[name], abs(mut.query(pos, tau)[2] - fd))
    print(f"{kind}, {'obstacles' if obstacles else 'empty map'}: {compared} of {n} points compared, {left_out} left "
          f"out, {live} with a box-lowered corner and dtau != 0; worst |dtau - fd| {worst:.2e}; mutants miss by "
          + ", ".join(f"{k} {v:.2e}" for k, v in miss.items()))
    assert left_out <= 0.02 * n, (left_out, n)
    assert live >= 200, live
    assert worst <= DTAU_BOUND, worst
    assert miss["bad_sign_above"] >= 10 * DTAU_BOUND
    if kind == "polynomial":
        assert miss["no_interval_zero"] >= 10 * DTAU_BOUND
    else:
        assert miss["no_interval_zero"] <= DTAU_BOUND      # (nothing to zero: the mutant is the lookup)


# ---- scenes shared with tests/test_gpu_time_moving.py ----------------------------------------------------------------
def _with_waypoint(b, rows, w, point):
    """The batch with waypoint w (1 .. m - 1) of `rows` moved to `point`."""
    x = b.x.reshape(b.x.shape[0], 3, -1).copy()
    x[rows, :, 3 * (w - 1)] = point
    return problem.Batch(b.waypoints, b.T, b.Df, x.reshape(b.x.shape[0], -1), b.m)


def _waypoint(b, r, w):
    return b.x.reshape(b.x.shape[0], 3, -1)[r, :, 3 * (w - 1)]


def aimed(b, T, t0, rows, nbox, poly, seed):
    """A batch and a box list aimed at it: every box is at an interior waypoint w >= 1 of one of `rows` (cyclically) at
    the time that row is there, so samples of the segments around it — segment w is a later one — are lowered.  A list
    of one box: the waypoint of all of `rows` is moved to one common point, which the box crosses when the first row is there.
    A polynomial list's intervals end inside the flight.  -> (batch, dict(kind, args of the setter, twin lookup))"""
    rng = np.random.default_rng(seed)
    B, m = b.x.shape[0], b.m
    Tb = np.broadcast_to(T, (B, m))
    t0 = np.broadcast_to(np.asarray(t0, dtype=np.float64), (B,))
    w_of = lambda i: 1 + (i % (m - 1)) if m > 2 else 1
    if nbox == 1:
        b = _with_waypoint(b, rows, w_of(1), _waypoint(b, rows[0], w_of(1)).copy())
    p_at, when, vel = np.zeros((nbox, 3)), np.zeros(nbox), np.zeros((nbox, 3))
    for i in range(nbox):
        r, w = rows[i % len(rows)], w_of(1 if nbox == 1 else i)
        p_at[i] = _waypoint(b, r, w) + (0.0 if nbox == 1 else rng.uniform(-0.2, 0.2, 3))
        when[i] = t0[r] + Tb[r, :w].sum()
        vel[i] = rng.uniform(-0.5, 0.5, 3)
    scale = rng.uniform(0.4, 1.0, (nbox, 3))
    if poly:
        acc = rng.uniform(-0.3, 0.3, (nbox, 3))
        coef = box_poly_twin.coefficients(p_at, vel, acc, when)
        t_range = np.stack([np.maximum(when - rng.uniform(1.0, 2.0, nbox), 0.0), when + rng.uniform(0.1, 0.4, nbox)], axis=1)
        return b, dict(poly=True, coef=coef, scale=scale, t_range=t_range)
    return b, dict(poly=False, p0=p_at - vel * when[:, None], vel=vel, scale=scale)


def lookup_of(sdf, bx):
    if bx["poly"]:
        return tm.PolyBoxLookup(sdf, bx["coef"], bx["scale"], bx["t_range"])
    return tm.BoxLookup(sdf, bx["p0"], bx["vel"], bx["scale"])



GT0_H = 1e-4


def gt0_case(mp):
    """The rows of the start-time test: 6 rows of 5 segments on the map `mp`, per-row start times, 8 constant-velocity
    boxes aimed at them -> (batch, T, t0, boxes)."""
    b = problem.make_trajectories(6, 5, mp, seed=9100, step_len=(1.0, 2.0), boundary="random")
    t0 = np.linspace(0.3, 1.3, 6)
    b, bx = aimed(b, b.T, t0, np.arange(6), 8, False, 9200)
    return b, b.T, t0, bx


def test_gt0_quotient_on_the_twin(oracle_mod):
    """The quotient tests/test_gpu_time_moving.py forms on the device — central differences of the evaluation's cost in
    t0 at h = GT0_H against gt0 — formed on the twin for the same rows: under a quarter of the 1e-5 the device is held
    to (tests/golden/TIME_MOVING_ANALYTIC.md records the figure)."""
    mp = problem.make_map((60, 50, 30), density=0.03, seed=11)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_points(mp.obstacle_points())
    b, T, t0, bx = gt0_case(mp)
    look = lookup_of(sdf, bx)
    p = dict(PARAMS)                                                # (= OPTI_NODE_PARAMS: what the device test runs)
    g0, fd = np.zeros(6), np.zeros(6)
    for i in range(6):
        g0[i] = tm.cost_gradT(T[i], b.Df[i], b.x[i], look, p, t0[i])[2]
        fd[i] = (tm.eval_cost(T[i], b.Df[i], b.x[i], look, p, t0[i] + GT0_H)
                 - tm.eval_cost(T[i], b.Df[i], b.x[i], look, p, t0[i] - GT0_H)) / (2 * GT0_H)
    dev = np.max(np.abs(g0 - fd)) / np.max(np.abs(fd))
    print(f"gt0 against central differences in t0 on the twin (h = {GT0_H}): off by {dev:.2e} of the max-norm "
          f"{np.max(np.abs(fd)):.3e}; gt0 = {np.array2string(g0, precision=3)}")
    assert np.all(g0 != 0.0) and dev <= 0.25e-5, dev


# ---- tests/golden/TIME_MOVING_ANALYTIC.md ---------------------------------------------------------------------------
ANALYTIC = dict(u=-0.3, X0=5.0, sx=1.0, x0=2.0, vy=1.5, t0=0.25, T=np.array([0.8, 1.1, 0.6]), y0=1.0, z0=1.5)


def analytic_case(oracle_mod=None):
    """The hand-derived case: (T, Df, x, p, boxes (p0, vel, scale), t0, and — given the oracle — an empty field)."""
    A = ANALYTIC
    T = A["T"]
    m = len(T)
    y = A["y0"] + A["vy"] * np.r_[0.0, np.cumsum(T)]
    Df = np.zeros((3, 6))
    Df[0, [0, 3]] = A["x0"]
    Df[1] = [y[0], A["vy"], 0.0, y[m], A["vy"], 0.0]
    Df[2, [0, 3]] = A["z0"]
    x = np.zeros((3, 3 * m - 3))
    for w in range(1, m):
        x[0, 3 * (w - 1)] = A["x0"]
        x[1, 3 * (w - 1):3 * w] = [y[w], A["vy"], 0.0]
        x[2, 3 * (w - 1)] = A["z0"]
    p = dict(PARAMS, ws=0.0)
    boxes = (np.array([[A["X0"], 3.0, 1.5]]), np.array([[A["u"], 0.0, 0.0]]), np.array([[A["sx"], 40.0, 40.0]]))
    sdf = None
    if oracle_mod is not None:
        sdf = oracle_mod.Sdf.from_map_size([0.0, 0.0, 0.0], 0.2, [8.0, 8.0, 3.0])   # empty: 10000 everywhere
    return T, Df, x.reshape(-1), p, boxes, A["t0"], sdf


def analytic_parts(T, p, t0):
    """parts[s][1] in closed form: wc vn dt cd(tau_s + 1e-3) (1 - q^30) / (1 - q), q = exp(-u dt / r)."""
    A = ANALYTIC
    vn = A["vy"] + 1e-5
    out, start = np.zeros(len(T)), t0
    for s, Ts in enumerate(T):
        dt = Ts / 30.0
        d_first = (A["X0"] + A["u"] * (start + 1e-3) - 0.5 * A["sx"]) - A["x0"]
        cd = p["alpha"] * math.exp(-(d_first - p["d0"]) / p["r"])
        q = math.exp(-A["u"] * dt / p["r"])
        out[s] = p["wc"] * vn * dt * cd * (1 - q ** 30) / (1 - q)
        start += Ts
    return out


def test_hand_derived_case(oracle_mod):
    """One box approaching along x over a path that holds x: d dist / d tau = u, grad = (-1, 0, 0), so
    parts[s][4] = -(u / r) parts[s][1], [5] their sums over the later segments, gt0 = -(u / r) sum_s parts[s][1], and
    parts[s][1] a geometric sum: 1e-12."""
    T, Df, x, p, (p0, vel, scale), t0, sdf = analytic_case(oracle_mod)
    u, r = ANALYTIC["u"], p["r"]
    c, gT, gt0, parts, low = tm.cost_gradT(T, Df, x, tm.BoxLookup(sdf, p0, vel, scale), p, t0)
    ref = analytic_parts(T, p, t0)
    assert low.all()
    assert np.max(np.abs(parts[:, 1] - ref) / ref) <= 1e-12
    q = -(u / r) * ref
    assert np.max(np.abs(parts[:, 4] - q) / np.abs(q)) <= 1e-12
    R = np.r_[np.cumsum(q[::-1])[::-1][1:], 0.0]
    assert np.max(np.abs(parts[:, 5] - R)) <= 1e-12 * np.max(np.abs(R))
    assert abs(gt0 - q.sum()) <= 1e-12 * abs(q.sum())
    assert abs(c - (ref.sum() + 1e-3)) <= 1e-12 * c
    # the path does not change with T (constant velocity, waypoints held): the own term is the lookup's alone plus the
    # weight dt's — checked through the law gT = ([2] + [3]) + [5]
    assert np.array_equal(gT, (parts[:, 2] + parts[:, 3]) + parts[:, 5])


def test_optimizer_laws(oracle_mod):
    """Bounds held exactly, F never rises, info consistent — tests/test_time_twin.py's laws with boxes in the field."""
    b, sdf = _scene(oracle_mod, B=3, m=4)
    p = dict(PARAMS)
    p0, vel, scale = scene_boxes(b, 9)
    look = tm.BoxLookup(sdf, p0, vel, scale)
    kw = dict(rho=1.0, t_min=0.2, t_max=2.5, first_move=0.05, ftol_rel=1e-7, xtol_abs=1e-10, max_evals=12)
    for i in range(len(b.x)):
        T_lo = np.array([0.1, 3.0, 0.9 * b.T[i][2], 0.0])             # below t_min; pinned (> t_max); active; none
        trace = []
        T_out, info = tm.optimize_times(b.T[i], b.Df[i], b.x[i], look, p, T_lo=T_lo, t0=0.2, trace=trace, **kw)
        assert np.all(np.diff(trace) <= 0.0)                                       # F monotone
        lo = np.maximum(kw["t_min"], T_lo)
        assert T_out[1] == 3.0                                                     # pinned: untouched by the descent
        free = np.array([0, 2, 3])
        assert np.all(T_out[free] >= lo[free]) and np.all(T_out[free] <= kw["t_max"])   # bounds exact
        assert info[0] in (tm.FTOL, tm.XTOL, tm.MAXEVAL) and 1 <= info[2] <= kw["max_evals"]
        c = tm.cost_gradT(T_out, b.Df[i], b.x[i], look, p, 0.2)[0]
        assert info[5] == c and info[4] <= info[3] and info[7] == T_out.sum()
        assert abs(info[4] - (info[5] + kw["rho"] * T_out.sum())) <= 1e-15 * abs(info[4])
        assert info[3] == trace[0] and info[4] == trace[-1] and len(trace) == info[1] + 1
        T1, info1 = tm.optimize_times(b.T[i], b.Df[i], b.x[i], look, p, T_lo=T_lo, t0=0.2, **dict(kw, max_evals=1))
        clamped = np.where(lo > kw["t_max"], lo, np.clip(b.T[i], lo, kw["t_max"]))
        assert np.array_equal(T1, clamped) and info1[0] == tm.MAXEVAL and info1[2] == 1 and info1[1] == 0
    # without time dependence the run is time_twin's, number for number
    T_ref, i_ref = tt.optimize_times(b.T[0], b.Df[0], b.x[0], sdf, p, **kw)
    T_st, i_st = tm.optimize_times(b.T[0], b.Df[0], b.x[0], tm.StaticLookup(sdf), p, t0=0.4, **kw)
    assert np.array_equal(T_ref, T_st) and np.array_equal(i_ref, i_st)
