"""The oracle's rounding-error magnitudes (oracle.eval_batch_mag) are sound and sharp — on the CPU, against the callback
evaluated exactly (mpmath, 40 digits) from the same float-rounded sample positions and field values.

Sound: for every row whose decisions are not within rounding of their thresholds (the cell choice, the in-map test,
the sample count; oracle.MARGINS), every entry of the C oracle and of the numpy twin lies within
KAPPA64 * u64 * magnitude (+ the flip allowance of the float-rounded coordinates) of the exact value — the bound
tests/test_gpu_entrywise.py holds the kernels to.  Sharp: three deliberately wrong twins, each of which passes every
1e-5 check of the suite, fail it.

The exact evaluation: coefficients A_s^-1 d from the exact inverse of each segment's Hermite matrix, the smoothness as
sum_s c_s' Q_s c_s with its coefficient-space gradient mapped back through A_s^-T, the reference's sample times (its
doubles, t += dt) with the weight dt = T / 30 exact, positions / velocities / accelerations rounded to float from their
exact values, the trilinear lookup, exp and sqrt in 40 digits.

The same for the two later semantics of include/gtop.h, through oracle.eval_batch_ext: gradient mode 1 (the consistent
gradient of tests/consistent_twin.py: plain, DYN, DYN with steep scale lengths) and the time-aware lookup (1 and 8
boxes, constant-velocity and polynomial lists, non-zero start times, validity intervals that end inside the trajectory's
span; also together with mode 1 and DYN).  There the exact evaluation forms box centres, faces and distances in 40
digits from the same double inputs — the polynomial's time clamped, then the powers summed exactly — at the exact sum
t0 + T[0] + ... + T[s-1] + t.  The extended oracle agrees with the three twins to 1e-12, a wrong twin per semantic
fails the bound (what each says about the bound's resolution is in its test's docstring), and Horner without fma —
a change of rounding only — passes."""
import math

import mpmath
import numpy as np
import pytest

from oracle import np_twin
from tests import box_poly_twin, consistent_twin, moving_twin

U64 = 2.0 ** -53
KAPPA64 = 2 ** 12
TIE = 2 ** 9 * U64

mp = mpmath.mp


def _col(m, wp, der):
    if wp == 0:
        return der
    if wp == m:
        return 3 + der
    return 6 + 3 * (wp - 1) + der


def exact_box_distance(pt, tau, boxes):
    """minDistToAllBox (src/edt_environment.cpp:26-73) in the working precision: pt, tau mpf; boxes: the dict of
    oracle.eval_batch_ext — constant velocity (p0, vel, scale) or polynomial (coef, scale, t_range); the centre, the
    faces and the distance from the same double inputs, the polynomial's time clamped BEFORE the evaluation."""
    M = mpmath.mpf
    scale = np.asarray(boxes["scale"], float).reshape(-1, 3)
    best = M(10000000)
    for b in range(len(scale)):
        d2 = M(0)
        for i in range(3):
            if "coef" in boxes:
                tc = tau
                if boxes.get("t_range") is not None:
                    t1, t2 = (M(float(v)) for v in np.asarray(boxes["t_range"], float).reshape(-1, 2)[b])
                    tc = min(max(tau, t1), t2)
                cf = np.asarray(boxes["coef"], float).reshape(-1, 3, 6)[b, i]
                c = sum(M(float(cf[j])) * tc ** j for j in range(6))
            else:
                c = M(float(boxes["p0"][b][i])) + M(float(boxes["vel"][b][i])) * tau
            h = M(float(scale[b, i])) / 2
            bmin, bmax = c - h, c + h
            di = M(0) if bmin <= pt[i] <= bmax else min(abs(pt[i] - bmin), abs(pt[i] - bmax))
            d2 += di * di
        best = min(best, mpmath.sqrt(d2))
    return best


def exact_cost_grad(T, Df, x, sdf, p, mode=0, boxes=None, t0=0.0):
    """The callback in 40-digit arithmetic (see the module docstring).  sdf: np_twin.Sdf.  mode 1: the consistent
    gradient (tests/consistent_twin.py).  boxes: every collision sample's corner values are min'ed with the exact
    distance from the corner voxel's centre to the nearest box at tau = t0 + T[0] + ... + T[s-1] + t, the sum exact."""
    with mpmath.workdps(40):
        m = len(T)
        ndp = 3 * m - 3
        d = np.hstack([np.asarray(Df, float).reshape(3, 6), np.asarray(x, float).reshape(3, ndp)])
        D = [[mpmath.mpf(float(v)) for v in d[a]] for a in range(3)]
        ws = 0.0 if p["step"] == 1 else p["ws"]
        wc = p["wc"]
        dyn = p.get("enable_dyn", 0) and p["step"] == 2
        cost = mpmath.mpf(0)
        grad = [[mpmath.mpf(0)] * ndp for _ in range(3)]
        origin = [mpmath.mpf(float(v)) for v in sdf.origin]
        res = mpmath.mpf(sdf.res)
        lo = [float(v) + 1e-4 for v in sdf.min_range]           # (the reference's doubles)
        hi = [float(v) - 1e-4 for v in sdf.max_range]
        r, d0, alpha = (mpmath.mpf(p[k]) for k in ("r", "d0", "alpha"))
        cs_tot = cc_tot = cv_tot = ca_tot = mpmath.mpf(0)
        seg_start = mpmath.mpf(float(t0))
        for s in range(m):
            Ts = mpmath.mpf(float(T[s]))
            A = mpmath.zeros(6, 6)
            for i in range(3):
                A[2 * i, i] = math.factorial(i)
                for j in range(i, 6):
                    A[2 * i + 1, j] = (math.factorial(j) // math.factorial(j - i)) * Ts ** (j - i)
            Ai = mpmath.inverse(A)
            cols = [_col(m, s + (row & 1), row >> 1) for row in range(6)]   # local row -> global column of d
            c = [[sum(Ai[i, row] * D[a][cols[row]] for row in range(6)) for i in range(6)] for a in range(3)]
            h = [[mpmath.mpf(0)] * 6 for _ in range(3)]                      # coefficient-space gradient
            Q = [[(i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2) // (i + j - 5)) * Ts ** (i + j - 5) if i >= 3 and j >= 3
                  else 0 for j in range(6)] for i in range(6)]
            for a in range(3):
                qc = [sum(Q[i][j] * c[a][j] for j in range(6)) for i in range(6)]
                cs_tot += sum(c[a][i] * qc[i] for i in range(6))
                for i in range(6):
                    h[a][i] += ws * 2 * qc[i]
            if abs(wc) >= 1e-4:
                dt_d = float(T[s]) / 30.0
                dt = Ts / 30
                t = 1e-3
                while t < float(T[s]):
                    tm = mpmath.mpf(t)
                    Tm = [tm ** i for i in range(6)]
                    TV = [i * tm ** (i - 1) if i else mpmath.mpf(0) for i in range(6)]
                    TVV = [i * (i - 1) * tm ** (i - 2) if i >= 2 else mpmath.mpf(0) for i in range(6)]
                    fl = lambda v: mpmath.mpf(float(np.float32(float(v))))
                    pos = [fl(sum(c[a][i] * Tm[i] for i in range(6))) for a in range(3)]
                    vel = [fl(sum(c[a][i] * TV[i] for i in range(6))) for a in range(3)]
                    vn = mpmath.sqrt(sum(v * v for v in vel)) + mpmath.mpf(1e-5)
                    if any(pos[a] < lo[a] or pos[a] > hi[a] for a in range(3)):
                        dist, g = mpmath.mpf(-1), [mpmath.mpf(0)] * 3
                    else:
                        idx = [int(mpmath.floor((pos[a] - res / 2 - origin[a]) / res)) for a in range(3)]
                        df = [(pos[a] - ((idx[a] + mpmath.mpf(0.5)) * res + origin[a])) / res for a in range(3)]
                        v = {}
                        for cx in range(2):
                            for cy in range(2):
                                for cz in range(2):
                                    ii = [min(max(idx[0] + cx, 0), sdf.grid[0] - 1), min(max(idx[1] + cy, 0), sdf.grid[1] - 1),
                                          min(max(idx[2] + cz, 0), sdf.grid[2] - 1)]
                                    v[cx, cy, cz] = mpmath.mpf(float(sdf.dist[ii[0], ii[1], ii[2]]))
                                    tau = seg_start + tm
                                    if boxes is not None and tau >= 0:
                                        pt = [(idx[a] + o + mpmath.mpf(0.5)) * res + origin[a]
                                              for a, o in enumerate((cx, cy, cz))]
                                        v[cx, cy, cz] = min(v[cx, cy, cz], exact_box_distance(pt, tau, boxes))
                        dx, dy, dz = df
                        v00 = (1 - dx) * v[0, 0, 0] + dx * v[1, 0, 0]
                        v01 = (1 - dx) * v[0, 0, 1] + dx * v[1, 0, 1]
                        v10 = (1 - dx) * v[0, 1, 0] + dx * v[1, 1, 0]
                        v11 = (1 - dx) * v[0, 1, 1] + dx * v[1, 1, 1]
                        v0 = (1 - dy) * v00 + dy * v10
                        v1 = (1 - dy) * v01 + dy * v11
                        dist = (1 - dz) * v0 + dz * v1
                        g = [sum(((1 - dz) if zz == 0 else dz) * ((1 - dy) if yy == 0 else dy) * (v[1, yy, zz] - v[0, yy, zz])
                                 for yy in range(2) for zz in range(2)) / res,
                             ((1 - dz) * (v10 - v00) + dz * (v11 - v01)) / res,
                             (v1 - v0) / res]
                    e = mpmath.exp(-(dist - d0) / r)
                    cd, gd = alpha * e, -(alpha / r) * e
                    cc_tot += wc * cd * vn * dt
                    for k in range(3):
                        for i in range(6):
                            w1 = gd * g[k] * vn if mode == 1 else gd * g[k] * cd * vn
                            h[k][i] += wc * (w1 * Tm[i] + cd * (vel[k] / vn) * TV[i]) * dt
                    if dyn:
                        acc = [fl(sum(c[a][i] * TVV[i] for i in range(6))) for a in range(3)]
                        av, rv, v0p = (mpmath.mpf(p[k]) for k in ("alpha_v", "r_v", "v0"))
                        aa, ra, a0p = (mpmath.mpf(p[k]) for k in ("alpha_a", "r_a", "a0"))
                        cv = ca = None
                        S = mpmath.mpf(0)
                        for k in range(3):
                            cv = av * mpmath.exp((abs(vel[k]) - v0p) / rv)
                            cv_tot += cv * vn * dt
                            ca = aa * mpmath.exp((abs(acc[k]) - a0p) / ra)
                            ca_tot += ca * vn * dt
                            S += cv + ca
                        for k in range(3):
                            gv = (av / rv) * mpmath.exp((abs(vel[k]) - v0p) / rv)
                            ga = (aa / ra) * mpmath.exp((abs(acc[k]) - a0p) / ra)
                            for i in range(6):
                                if mode == 1:
                                    h[k][i] += (gv * mpmath.sign(vel[k]) * vn + S * (vel[k] / vn)) * TV[i] * dt
                                    h[k][i] += ga * mpmath.sign(acc[k]) * vn * TVV[i] * dt
                                    continue
                                h[k][i] += (gv * vn * TV[i] + cv * (vel[k] / vn) * TV[i]) * dt
                                h[k][i] += (ga * vn * TVV[i] + ca * (vel[k] / vn) * TV[i]) * dt
                    t += dt_d
            seg_start += Ts
            for a in range(3):   # A_s^-T back to the free variables
                for row in range(6):
                    col = cols[row]
                    if col >= 6:
                        grad[a][col - 6] += sum(Ai[i, row] * h[a][i] for i in range(6))
        cost = ws * cs_tot + cc_tot + cv_tot + ca_tot + mpmath.mpf(1e-3)
        return cost, [[gi + mpmath.mpf(1e-5) for gi in grad[a]] for a in range(3)]


def _map(kind, origin, grid=(14, 12, 8), res=0.25, seed=0):
    rng = np.random.default_rng(seed)
    ix, iy, iz = np.meshgrid(*(np.arange(n) for n in grid), indexing="ij")
    if kind == "constant":
        dist = np.full(grid, 0.7)
    elif kind == "linear":
        dist = 0.3 + 0.11 * ix - 0.05 * iy + 0.07 * iz
    elif kind == "signed":
        dist = rng.uniform(-1.0, 2.0, size=grid)
    else:
        dist = rng.uniform(0.0, 2.5, size=grid)
    return np.asarray(origin, float), res, grid, dist


def _case(m, kind, origin, T_first, seed, rows=2, T_range=(0.3, 0.9)):
    org, res, grid, dist = _map(kind, origin, seed=seed)
    rng = np.random.default_rng(seed)
    size = np.array(grid) * res
    lo, hi = org + 0.4, org + size - 0.4
    Ts, Dfs, xs = [], [], []
    for _ in range(rows):
        wp = lo + rng.random((m + 1, 3)) * (hi - lo)
        T = rng.uniform(*T_range, size=m)
        T[0] = T_first
        Df = np.zeros((3, 6))
        Df[:, 0], Df[:, 3] = wp[0], wp[m]
        Df[:, 1], Df[:, 2] = rng.normal(0, 0.3, 3), rng.normal(0, 0.3, 3)
        dp = np.zeros((3, 3 * m - 3))
        for k in range(1, m):
            dp[:, 3 * (k - 1)] = wp[k]
            dp[:, 3 * (k - 1) + 1] = rng.normal(0, 0.5, 3)
            dp[:, 3 * (k - 1) + 2] = rng.normal(0, 0.5, 3)
        Ts.append(T)
        Dfs.append(Df)
        xs.append(dp.reshape(-1))
    return (org, res, grid, dist), np.array(Ts), np.array(Dfs), np.array(xs)


KW = [dict(), dict(step=1), dict(wc=0.0), dict(wc=5e-5),
      dict(enable_dyn=1, alpha_v=1.0, r_v=4.0, v0=2.5, alpha_a=1.0, r_a=15.0, a0=3.5),
      # tests/test_gpu_consistent_gradient.py's STEEP block: gv sgn(v), ga sgn(a) weigh as much as the rest
      dict(enable_dyn=1, alpha_v=2.0, r_v=0.5, v0=2.5, alpha_a=1.5, r_a=1.0, a0=3.5)]
CASES = [(m, kind, origin, T0, kw_i)
         for i, (m, kind, origin, T0) in enumerate([
             (2, "random", (0.0, 0.0, 0.0), 2.0), (3, "constant", (-1.0, -1.5, 0.0), 0.0299),
             (4, "linear", (-500.0, 300.0, 0.0), 0.0301), (5, "signed", (0.0, 0.0, 0.0), 0.5),
             (6, "random", (-500.0, 300.0, 0.0), 0.0299), (7, "linear", (0.0, 0.0, 0.0), 2.0),
             (13, "random", (-1.0, -1.5, 0.0), 0.0301)])
         for kw_i in ([0, 4] if m in (3, 6) else [i % 5])]
# the consistent gradient (mode 1) and the time-aware lookup: (m, field, origin, T[0], KW index, extra); extra: mode,
# boxes = (list kind, number of boxes), t0.  Half of a polynomial list's boxes carry a t_range that ends inside the
# trajectory's time span (_boxes).
CASES += [
    (3, "random", (0.0, 0.0, 0.0), 0.5, 0, dict(mode=1)),
    (6, "random", (0.0, 0.0, 0.0), 0.5, 1, dict(mode=1)),       # (step 1: the collision gradient alone)
    (5, "signed", (-1.0, -1.5, 0.0), 0.5, 4, dict(mode=1)),
    (4, "random", (0.0, 0.0, 0.0), 0.5, 5, dict(mode=1)),
    (2, "random", (0.0, 0.0, 0.0), 2.0, 0, dict(boxes=("cv", 1), t0=1.3)),
    (6, "random", (-500.0, 300.0, 0.0), 0.5, 1, dict(boxes=("cv", 8), t0=2.7)),      # (step 1: no d'Rd at |d| = 500)
    (4, "constant", (0.0, 0.0, 0.0), 0.5, 1, dict(boxes=("poly", 1), t0=0.4)),
    (5, "random", (0.0, 0.0, 0.0), 0.5, 0, dict(boxes=("poly", 8), t0=1.1)),
    (7, "random", (-1.0, -1.5, 0.0), 0.5, 4, dict(mode=1, boxes=("cv", 8), t0=0.9)),
    (3, "signed", (0.0, 0.0, 0.0), 0.5, 5, dict(mode=1, boxes=("poly", 8), t0=0.5)),
    (13, "random", (-1.0, -1.5, 0.0), 0.0301, 0, dict(mode=1, boxes=("cv", 8), t0=0.25)),
    # segments of about a second, collision term alone: A_s^-T cancels least there, so the bound is at its sharpest
    (4, "linear", (0.0, 0.0, 0.0), 1.0, 1, dict(mode=1, T_range=(0.9, 1.3))),
    (4, "constant", (0.0, 0.0, 0.0), 1.0, 1, dict(boxes=("cv", 8), t0=0.6, T_range=(0.9, 1.3))),
    (3, "linear", (0.0, 0.0, 0.0), 1.0, 1, dict(boxes=("poly", 8), t0=0.6, T_range=(0.9, 1.3))),
]


def _waypoints(Df, x, m):
    """(rows, m + 1, 3): the waypoint positions _case put into Df and x."""
    Df, x = np.asarray(Df).reshape(-1, 3, 6), np.asarray(x).reshape(len(x), 3, 3 * m - 3)
    wp = np.empty((len(x), m + 1, 3))
    wp[:, 0], wp[:, m] = Df[:, :, 0], Df[:, :, 3]
    for k in range(1, m):
        wp[:, k] = x[:, :, 3 * (k - 1)]
    return wp


def _boxes(kind, nbox, T, Df, x, t0, seed):
    """Boxes aimed as tests/test_gpu_moving_cost.py::_aimed_boxes aims them — box k is at a waypoint of a row when that
    row's trajectory is.  A polynomial list: that motion with an acceleration and small cubic .. quintic terms, and on
    every second box a validity interval that ends 0.05 s after the rendezvous, inside the trajectory's span."""
    rng = np.random.default_rng(seed)
    m = T.shape[1]
    wp = _waypoints(Df, x, m)
    j, w = rng.integers(0, len(x), nbox), rng.integers(1, m, nbox)
    vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * np.array([1.0, 1.0, 0.2])
    when = np.array([t0 + T[jj][:ww].sum() for jj, ww in zip(j, w)])
    scale = rng.uniform(1.0, 2.0, (nbox, 3))
    if kind == "cv":
        return dict(p0=wp[j, w] - vel * when[:, None], vel=vel, scale=scale)
    coef = box_poly_twin.coefficients(wp[j, w], vel, rng.uniform(-1.0, 1.0, (nbox, 3)), when)
    coef[:, :, 3:] = rng.normal(0.0, 1.0, (nbox, 3, 3)) * np.array([2e-2, 3e-3, 4e-4])
    coef[:, :, 0] -= sum(coef[:, :, i] * when[:, None] ** i for i in (3, 4, 5))     # (still at the waypoint at `when`)
    t_range = np.tile([-np.inf, np.inf], (nbox, 1))
    t_range[::2] = np.stack([when[::2] - 0.3, when[::2] + 0.05], axis=1)
    return dict(coef=coef, scale=scale, t_range=t_range)


def _parts(case):
    extra = case[5] if len(case) > 5 else {}
    return case[:5], extra.get("mode", 0), extra.get("boxes"), extra.get("t0", 0.0)


@pytest.fixture(scope="module")
def evaluated(oracle_mod):
    """Every case: the oracle with its magnitudes, the exact values, the inputs."""
    out = []
    for j, case in enumerate(CASES):
        (m, kind, origin, T0, kw_i), mode, box_spec, t0 = _parts(case)
        T_range = case[5].get("T_range", (0.3, 0.9)) if len(case) > 5 else (0.3, 0.9)
        (org, res, grid, dist), T, Df, x = _case(m, kind, origin, T0, seed=30 + j, rows=1 if m == 13 else 2, T_range=T_range)
        kw = dict(KW[kw_i])
        sdf = oracle_mod.Sdf(org, res, grid, dist.reshape(-1))
        twin_sdf = np_twin.Sdf(org, res, grid, dist)
        p = dict(oracle_mod.OPTI_NODE_PARAMS)
        p.update(kw)
        boxes = _boxes(*box_spec, T, Df, x, t0, seed=60 + j) if box_spec else None
        lowered = None
        if len(case) == 5:
            ref = oracle_mod.eval_batch_mag(T, Df, x, sdf, oracle_mod.make_params(**kw))
        else:
            *ref, lowered = oracle_mod.eval_batch_ext(T, Df, x, sdf, oracle_mod.make_params(**kw), mode=mode, boxes=boxes,
                                                      t0=t0)
            ref = tuple(ref)
        exact = []
        for b in range(len(x)):
            c, g = exact_cost_grad(T[b], Df[b], x[b], twin_sdf, p, mode, boxes, t0)
            exact.append((float(c), np.array([float(v) for a in range(3) for v in g[a]])))
        out.append(dict(case=case, T=T, Df=Df, x=x, p=p, sdf=twin_sdf, osdf=sdf, ref=ref, exact=exact, mode=mode,
                        boxes=boxes, t0=t0, lowered=lowered, new=len(case) > 5))
    return out


def _excess(c, g, e, ref, b):
    """|value - exact| beyond the flip allowance, in units of u64 * magnitude: (cost, largest gradient entry)."""
    _, _, cm, gm, _, cf, gf = ref
    rc = max(abs(c - e[0]) - cf[b], 0.0) / (U64 * cm[b])
    rg = np.max(np.maximum(np.abs(g - e[1]) - gf[b], 0.0) / (U64 * gm[b]))
    return rc, rg


def _tie(ref, b):
    mg = ref[4][b]
    return bool(mg[1] < TIE or mg[2] < TIE or mg[3] < TIE)


def test_mag_outputs_leave_the_evaluation_alone(oracle_mod):
    (org, res, grid, dist), T, Df, x = _case(6, "random", (0.0, 0.0, 0.0), 0.5, seed=3, rows=4)
    sdf = oracle_mod.Sdf(org, res, grid, dist.reshape(-1))
    for kw in KW:
        prm = oracle_mod.make_params(**kw)
        c, g, _ = oracle_mod.eval_batch(T, Df, x, sdf, prm)
        c2, g2, cm, gm, mg, cf, gf = oracle_mod.eval_batch_mag(T, Df, x, sdf, prm)
        assert np.array_equal(c, c2) and np.array_equal(g, g2)
        assert (cm >= np.abs(c)).all() and (gm >= np.abs(g)).all()      # a magnitude bounds its value
        assert (cf >= 0).all() and (gf >= 0).all() and (mg >= 0).all()


def test_the_bound_holds_for_the_oracle(evaluated):
    worst, ties = 0.0, 0
    for ev in evaluated:
        for b, e in enumerate(ev["exact"]):
            if _tie(ev["ref"], b):
                ties += 1
                continue
            rc, rg = _excess(ev["ref"][0][b], ev["ref"][1][b], e, ev["ref"], b)
            worst = max(worst, rc, rg)
            assert rc <= KAPPA64 and rg <= KAPPA64, (ev["case"], b, rc, rg)
    assert ties <= 1, ties
    assert worst > 0          # (the comparison is not vacuous: the oracle does round)


class _Unfused(box_poly_twin.PolyLookup):
    """The polynomial centre by Horner with a separate multiply and add per step: the same value up to rounding."""

    def query(self, pos):
        tau = self.taus[self.k]
        if tau >= 0.0:
            self.p0 = box_poly_twin.centres(self.coef, tau, self.t_range, fma_=lambda a, b, c: a * b + c)
        return moving_twin.TimedLookup.query(self, pos)


class _ScaledGradient:
    """A lookup whose field gradient is off by a relative `eps`: the distance, and with it the cost, is untouched."""

    def __init__(self, inner, eps):
        self.inner, self.eps = inner, eps

    def query(self, pos):
        d, g = self.inner.query(pos)
        return d, np.asarray(g) * (1.0 + self.eps)


def _lookup(ev, b, boxes=None, poly_lookup=box_poly_twin.PolyLookup):
    """The duck-typed sdf of consistent_twin.cost_grad for row b: the static field, or the time-aware lookup."""
    boxes = ev["boxes"] if boxes is None else boxes
    if boxes is None:
        return ev["sdf"]
    taus = moving_twin.sample_times(ev["T"][b], ev["t0"])
    if "coef" in boxes:
        return poly_lookup(ev["osdf"], taus, boxes["coef"], boxes["scale"], boxes.get("t_range"))
    return moving_twin.TimedLookup(ev["osdf"], taus, boxes["p0"], boxes["vel"], boxes["scale"])


def _twin(ev, b, look=None):
    if not ev["new"]:
        c, g, _ = np_twin.cost_grad(ev["T"][b], ev["Df"][b], ev["x"][b], ev["sdf"], ev["p"])
        return c, g
    c, g, _ = consistent_twin.cost_grad(ev["T"][b], ev["Df"][b], ev["x"][b], look or _lookup(ev, b), ev["p"], ev["mode"])
    return c, g


def _normwise(c, g, c_ref, g_ref):
    return abs(c - c_ref) / abs(c_ref), float(np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref)))


def test_the_twin_agrees_within_the_bound(evaluated):
    for ev in evaluated:
        for b, e in enumerate(ev["exact"]):
            if _tie(ev["ref"], b):
                continue
            c, g = _twin(ev, b)
            rc, rg = _excess(c, g, e, ev["ref"], b)
            assert rc <= KAPPA64 and rg <= KAPPA64, (ev["case"], b, rc, rg)
            # and the two restatements within the bound of each other (twice: each is within it of the exact value)
            rc2, rg2 = _excess(c, g, (ev["ref"][0][b], ev["ref"][1][b]), ev["ref"], b)
            assert rc2 <= 2 * KAPPA64 and rg2 <= 2 * KAPPA64, (ev["case"], b, rc2, rg2)


@pytest.mark.parametrize("mutation", ["no float round trip", "no +1e-5 in vn", "no +1e-5 in the gradient"])
def test_the_bound_catches_wrong_twins(evaluated, monkeypatch, mutation):
    """Each of these passes the 1e-5 normwise checks; the entrywise bound must fail on at least one case."""
    if mutation == "no float round trip":
        monkeypatch.setattr(np_twin, "to_float", lambda v: float(v))
    elif mutation == "no +1e-5 in vn":
        monkeypatch.setattr(np_twin, "VN_EPS", 0.0)
    else:
        monkeypatch.setattr(np_twin, "GRAD_EPS", 0.0)
    worst = 0.0
    for ev in evaluated:
        if ev["new"]:      # (the cases of the later semantics have their own wrong twins below)
            continue
        for b, e in enumerate(ev["exact"]):
            if _tie(ev["ref"], b):
                continue
            c, g = _twin(ev, b)
            worst = max(worst, *_excess(c, g, e, ev["ref"], b))
    assert worst > KAPPA64, (mutation, worst)


def test_the_extended_oracle_agrees_with_the_twins(evaluated):
    """oracle.eval_batch_ext against tests/consistent_twin.py (mode 1), tests/moving_twin.py (constant-velocity boxes)
    and tests/box_poly_twin.py (polynomial boxes), to the 1e-12 normwise the device is held to against them; and every
    moving case is one a static lookup could not pass: each row has collision samples with a box-lowered corner."""
    for ev in evaluated:
        if not ev["new"]:
            continue
        for b in range(len(ev["x"])):
            look = _lookup(ev, b)
            c, g = _twin(ev, b, look)
            rc, rg = _normwise(c, g, ev["ref"][0][b], ev["ref"][1][b])
            assert rc <= 1e-12 and rg <= 1e-12, (ev["case"], b, rc, rg)
            if ev["boxes"] is not None:
                assert ev["lowered"][b] == int(np.sum(look.lowered)) > 0, (ev["case"], b, ev["lowered"][b])
                if "coef" in ev["boxes"]:    # a validity interval ends inside this row's time span
                    t2 = ev["boxes"]["t_range"][:, 1]
                    assert np.any((t2 > look.taus[0]) & (t2 < look.taus[-1])), ev["case"]


def test_mode_1_leaves_the_cost_and_the_idle_axes_alone(oracle_mod):
    """The cost statements are the same in both modes (bit-equal); an axis on which nothing moves (sgn(+-0) = 0, zero
    velocity and acceleration of zero magnitude) gets nothing but the callback's +1e-5, with magnitude 1e-5 and no
    allowance."""
    (org, res, grid, dist), T, Df, x = _case(4, "constant", (-1.0, -1.5, -1.0), 0.5, seed=5, rows=2)
    Df[:, 1:, :] = 0.0                                   # y, z: every waypoint at 0 (inside the map), nothing moves
    xs = x.reshape(2, 3, -1).copy()
    xs[:, 1:, :] = 0.0
    x = xs.reshape(2, -1)
    sdf = oracle_mod.Sdf(org, res, grid, np.zeros(dist.size))   # (a zero field: no corner magnitude either)
    prm = oracle_mod.make_params(**KW[5])
    c0, g0, *_ = oracle_mod.eval_batch_ext(T, Df, x, sdf, prm, mode=0)
    c1, g1, cm, gm, mg, cf, gf, _ = oracle_mod.eval_batch_ext(T, Df, x, sdf, prm, mode=1)
    assert np.array_equal(c0, c1) and not np.array_equal(g0, g1)
    n = x.shape[1] // 3
    assert np.all(g1[:, n:] == 1e-5) and np.all(gm[:, n:] == 1e-5) and np.all(gf[:, n:] == 0.0)
    assert np.all(g0[:, n:] != 1e-5)                      # (the reference's gradient does push an idle axis: gv |v|)


# name -> (the cases it applies to, what the suite holds that road to today, normwise; None: see the docstring)
WRONG = {
    "mode 1: field-gradient weight off by 2^-22": (lambda ev: ev["mode"] == 1, 1e-5),
    "moving: half extents off by 2^-36": (lambda ev: ev["boxes"] is not None and ev["mode"] == 0, None),
}


@pytest.mark.parametrize("mutation", list(WRONG))
def test_the_bound_catches_wrong_twins_of_the_later_semantics(evaluated, mutation):
    """Mode 1: a field-gradient weight gd*grad(k)*vn off by 2^-22 (2.4e-7) passes the 1e-5 normwise that
    tests/test_gpu_consistent_gradient.py holds the mode to, on every row, and fails the entrywise bound.  What the
    bound resolves is set by Gmag / |g|, the cancellation of A_s^-T and of the corner differences carried as products
    of magnitudes: some 5e4 on these rows even with the collision term alone and segments of a second, so 2^-30
    (the same twin: largest ratio 98 of 4096) stays below it.

    Moving: half extents off by 2^-36 fail the bound (largest ratios 5158 and 6600, on the cost of the rows with
    segments of a second on a constant field).  That twin does NOT pass the 1e-12 normwise of
    tests/test_gpu_moving_cost.py / tests/test_gpu_box_polynomials.py either — it is 3e-12 .. 1e-11 off in the cost and
    up to 1.7e-10 in the gradient — and none was found that does: Cmag >= (1 + (dist + d0) / r) * cost >= 2.6 cost, so
    on the cost the bound is never below 1.2e-12 relative, and a perturbed lookup moves every entry a sample feeds by
    the same relative amount, so an entry cannot leave its bound (4.5e-13 * Gmag_k, Gmag_k some 1e4 |g_k| here) before
    the row's largest leaves 1e-12.  For these bodies the entrywise check adds the small entries' own bound and the
    bodies no 1e-12 test launches, not resolution."""
    applies, today = WRONG[mutation]
    worst, rows = 0.0, 0
    for ev in evaluated:
        if not ev["new"] or not applies(ev):
            continue
        for b, e in enumerate(ev["exact"]):
            if _tie(ev["ref"], b):
                continue
            if mutation.startswith("mode 1"):
                look = _ScaledGradient(_lookup(ev, b), 2.0 ** -22)
            else:
                look = _lookup(ev, b, dict(ev["boxes"], scale=ev["boxes"]["scale"] * (1.0 + 2.0 ** -36)))
            c, g = _twin(ev, b, look)
            c_ok, g_ok = _twin(ev, b)
            rc, rg = _normwise(c, g, c_ok, g_ok)
            assert today is None or (rc <= today and rg <= today), (mutation, ev["case"], b, rc, rg)
            worst = max(worst, *_excess(c, g, e, ev["ref"], b))
            rows += 1
    assert rows >= 2
    assert worst > KAPPA64, (mutation, worst)


def test_horner_without_fma_stays_within_the_bound(evaluated):
    """The negative control: a separate multiply and add per Horner step changes the rounding of a box centre and
    nothing else, and must pass."""
    rows = 0
    for ev in evaluated:
        if not ev["new"] or ev["boxes"] is None or "coef" not in ev["boxes"]:
            continue
        for b, e in enumerate(ev["exact"]):
            if _tie(ev["ref"], b):
                continue
            c, g = _twin(ev, b, _lookup(ev, b, poly_lookup=_Unfused))
            c_ok, g_ok = _twin(ev, b)
            rows += not (c == c_ok and np.array_equal(g, g_ok))
            rc, rg = _excess(c, g, e, ev["ref"], b)
            assert rc <= KAPPA64 and rg <= KAPPA64, (ev["case"], b, rc, rg)
    assert rows >= 1          # (the control does round differently somewhere)
