"""The trajectory report and the selection (include/gtop.h: gtop_validate_*, gtop_select_best_device) restated in
numpy, independently of the library, from pieces that are already tested: the C oracle's getTraj (oracle.traj_samples)
for the sample points, its evaluateEDTWithGrad (oracle.Sdf.edt_query) for the distances, and numpy's polynomial
arithmetic (Horner, np.polyval on the differentiated coefficients — not the kernel's evaluation order) for velocity and
acceleration.  The sample times replay PolynomialTraj::getTraj (polynomial_traj.hpp:69-78): eval_t accumulated from 0 by
dt while eval_t <= time_sum, the segment walk of :48-51 with the last segment extended."""
import numpy as np

N_REPORT = 12


def sample_times(T, dt=0.01):
    """(eval_t (N,), segment (N,), local time (N,), time_sum) of every getTraj sample."""
    T = np.asarray(T, dtype=np.float64)
    time_sum = np.float64(0.0)
    for s in range(len(T)):
        time_sum = time_sum + T[s]
    dt = np.float64(dt)
    ts, segs, loc = [], [], []
    t = np.float64(0.0)
    while t <= time_sum:
        u, idx = t, 0
        while idx < len(T) - 1 and T[idx] <= u:
            u = u - T[idx]
            idx += 1
        ts.append(t)
        segs.append(idx)
        loc.append(u)
        t = t + dt
    return np.array(ts), np.array(segs, dtype=np.int64), np.array(loc), float(time_sum)


def kinematics(coeff, T, dt=0.01):
    """Velocity and acceleration of every sample: dict(t, seg, loc, time_sum, v (N, 3), a (N, 3), sv (N, 3), sa (N, 3));
    sv / sa = the sum of the absolute values of the derivative's terms at the sample (what a rounding bound scales by)."""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6)
    t, seg, loc, time_sum = sample_times(T, dt)
    N = len(t)
    v, a, sv, sa = (np.zeros((N, 3)) for _ in range(4))
    j = np.arange(6)
    for k in range(3):
        for s in np.unique(seg):
            rows = seg == s
            c = coeff[s, k]
            dc = (j * c)[1:]                  # ascending coefficients of p'
            ddc = (j * (j - 1) * c)[2:]       # ... of p''
            u = loc[rows]
            v[rows, k] = np.polyval(dc[::-1], u)
            a[rows, k] = np.polyval(ddc[::-1], u)
            sv[rows, k] = np.abs(dc) @ np.abs(u)[None, :] ** np.arange(5)[:, None]
            sa[rows, k] = np.abs(ddc) @ np.abs(u)[None, :] ** np.arange(4)[:, None]
    return dict(t=t, seg=seg, loc=loc, time_sum=time_sum, v=v, a=a, sv=sv, sa=sa)


def out_of_map(points, map_min, map_max):
    """isInMap's complement, sdf_map.cpp:55-69"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.any((points < map_min + 1e-4) | (points > map_max - 1e-4), axis=1)


def reduce_report(t, dist, oom, kin, margin):
    """The 12 entries from the per-sample quantities (dist already -1 where out of the map)."""
    r = np.zeros(N_REPORT)
    r[0] = len(t)
    i = int(np.argmin(dist))          # the first of equal minima
    r[1], r[2], r[3] = dist[i], t[i], i
    below = np.flatnonzero(dist <= margin)
    r[4] = len(below)
    r[5] = t[below[0]] if len(below) else -1.0
    r[6] = np.count_nonzero(oom)
    r[7] = np.sqrt((kin["v"] ** 2).sum(axis=1)).max()
    r[8] = np.sqrt((kin["a"] ** 2).sum(axis=1)).max()
    r[9] = np.abs(kin["v"]).max()
    r[10] = np.abs(kin["a"]).max()
    r[11] = kin["time_sum"]
    return r


def report(oracle_mod, coeff, T, osdf, margin, p0=None, vel=None, scale=None, t0=0.0, use_boxes=False, dt=0.01,
           max_samples=8192):
    """One trajectory's report and its per-sample data: (r (12,), dict(points, dist, tau, out, **kinematics))."""
    none = np.zeros((0, 3))
    p0, vel, scale = (none if a is None else np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (p0, vel, scale))
    kin = kinematics(coeff, T, dt)
    n, pts = oracle_mod.traj_samples(coeff, T, dt, max_samples)
    assert n == len(kin["t"]) <= max_samples, (n, len(kin["t"]))
    tau = np.float64(t0) + kin["t"] if use_boxes else np.full(n, -1.0)
    dist, _ = osdf.edt_query(pts, tau, p0, vel, scale)
    oom = out_of_map(pts, np.array(osdf.c.min_range[:]), np.array(osdf.c.max_range[:]))
    assert np.all(dist[oom] == -1.0)
    return reduce_report(kin["t"], dist, oom, kin, margin), dict(points=pts, dist=dist, tau=tau, out=oom, **kin)


# Rounding errors, in units of eps times the sum S of the absolute values of a derivative's (at most 5) terms, of any
# two evaluations of it that use one multiplication for the integer factor, products for the powers and a sum of the
# terms in some order or a Horner scheme: per term at most 1 (factor) + 3 (a power of up to t^4 by products) + 1
# (the product) roundings, and at most 4 additions each touching a partial sum no larger than S — under 9 eps S for
# one evaluation, 18 for the difference of two.  A norm adds 3 squares, 2 additions and a square root on each side:
# under 4 eps of the norm, which is at most S summed over the axes.  26 in all; doubled for the second-order terms
# left out: 52, taken as 64.
VEL_ACC_EPS = 64


def vel_acc_bounds(kin, rel=1e-12):
    """Absolute tolerances for entries 7..10 of one trajectory's report: `rel` times the sum of the absolute values of
    the derivative's terms (at most 5) at a sample — for a norm summed over the axes (||e||_2 <= ||e||_1) — at the
    sample where that is largest."""
    return np.array([rel * kin["sv"].sum(axis=1).max(), rel * kin["sa"].sum(axis=1).max(),
                     rel * kin["sv"].max(), rel * kin["sa"].max()])


def select(rep, cost, max_vel=0.0, max_acc=0.0, per_axis=False, allow_out_of_map=False):
    """(pass (B,) bool, best (2,) int32): include/gtop.h's rule, vectorised."""
    rep = np.asarray(rep, dtype=np.float64).reshape(-1, N_REPORT)
    cost = np.asarray(cost, dtype=np.float64).reshape(-1)
    velf = rep[:, 9] if per_axis else rep[:, 7]
    accf = rep[:, 10] if per_axis else rep[:, 8]
    ok = rep[:, 4] == 0
    if not allow_out_of_map:
        ok &= rep[:, 6] == 0
    if max_vel > 0:
        ok &= velf <= max_vel
    if max_acc > 0:
        ok &= accf <= max_acc
    ok &= np.isfinite(cost)
    best = np.array([-1, int(ok.sum())], dtype=np.int32)
    if ok.any():
        c = np.where(ok, cost, np.inf)
        best[0] = int(np.argmin(c))       # the first of equal minima
    return ok, best


def select_loop(rep, cost, max_vel=0.0, max_acc=0.0, per_axis=False, allow_out_of_map=False):
    """The same rule as a plain loop (what the vectorised form and the kernel are checked against)."""
    ok, best_i, best_c, n = [], -1, None, 0
    for b in range(len(cost)):
        r, c = rep[b], float(cost[b])
        good = r[4] == 0
        if r[6] != 0 and not allow_out_of_map:
            good = False
        if max_vel > 0 and not (r[9 if per_axis else 7] <= max_vel):
            good = False
        if max_acc > 0 and not (r[10 if per_axis else 8] <= max_acc):
            good = False
        if c != c or c in (float("inf"), float("-inf")):
            good = False
        ok.append(good)
        if good:
            n += 1
            if best_c is None or c < best_c:
                best_i, best_c = b, c
    return np.array(ok, dtype=bool), np.array([best_i, n], dtype=np.int32)


def selection_cases():
    """Constructed (name, report (B, 12), cost (B,), limits dict) inputs: ties, a NaN cost, an inf cost, nobody
    passing, each limit switched off and on."""
    rng = np.random.default_rng(17)
    B = 300
    rep = np.zeros((B, N_REPORT))
    rep[:, 0] = 500
    rep[:, 1] = rng.uniform(0.1, 2.0, B)
    rep[:, 4] = rng.integers(0, 3, B) * (rng.uniform(size=B) < 0.3)
    rep[:, 6] = rng.integers(0, 2, B) * (rng.uniform(size=B) < 0.2)
    rep[:, 9] = rng.uniform(0.5, 4.0, B)
    rep[:, 7] = rep[:, 9] * rng.uniform(1.0, 1.7, B)
    rep[:, 10] = rng.uniform(0.5, 6.0, B)
    rep[:, 8] = rep[:, 10] * rng.uniform(1.0, 1.7, B)
    cost = rng.uniform(10.0, 20.0, B)
    cases = []
    for name, lim in (("all limits off", dict()),
                      ("velocity norm", dict(max_vel=3.0)),
                      ("acceleration norm", dict(max_acc=4.0)),
                      ("per axis", dict(max_vel=3.0, max_acc=4.0, per_axis=True)),
                      ("norms", dict(max_vel=3.0, max_acc=4.0)),
                      ("out of map allowed", dict(allow_out_of_map=True)),
                      ("negative limits are off", dict(max_vel=-1.0, max_acc=-2.0))):
        cases.append((name, rep.copy(), cost.copy(), lim))
    # ties: the least cost three times among passing rows, once more in a failing row in front of them
    r, c = rep.copy(), cost.copy()
    r[[40, 90, 170, 250], 4] = 0
    r[[40, 90, 170, 250], 6] = 0
    r[40, 4] = 2
    c[[40, 90, 170, 250]] = 1.0
    cases.append(("ties", r, c, dict()))
    # NaN and +-inf costs below every finite one do not win and do not pass
    r, c = rep.copy(), cost.copy()
    r[:20, 4] = 0
    r[:20, 6] = 0
    c[3], c[5], c[7] = np.nan, -np.inf, np.inf
    cases.append(("nan and inf costs", r, c, dict()))
    # nobody passes: every row violates the margin; and: every cost is NaN
    r = rep.copy()
    r[:, 4] = 1
    cases.append(("nobody passes (margin)", r, cost.copy(), dict()))
    cases.append(("nobody passes (costs)", rep.copy(), np.full(B, np.nan), dict()))
    cases.append(("nobody passes (velocity)", rep.copy(), cost.copy(), dict(max_vel=0.1)))
    # a single row
    cases.append(("one row passing", rep[:1] * 0, np.array([2.5]), dict()))
    return cases
