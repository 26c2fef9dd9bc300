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
exact values, the trilinear lookup, exp and sqrt in 40 digits."""
import math

import mpmath
import numpy as np
import pytest

from oracle import np_twin

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


def exact_cost_grad(T, Df, x, sdf, p):
    """The callback in 40-digit arithmetic (see the module docstring).  sdf: np_twin.Sdf."""
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
                            h[k][i] += wc * (gd * g[k] * cd * vn * Tm[i] + cd * (vel[k] / vn) * TV[i]) * dt
                    if dyn:
                        acc = [fl(sum(c[a][i] * TVV[i] for i in range(6))) for a in range(3)]
                        av, rv, v0p = (mpmath.mpf(p[k]) for k in ("alpha_v", "r_v", "v0"))
                        aa, ra, a0p = (mpmath.mpf(p[k]) for k in ("alpha_a", "r_a", "a0"))
                        cv = ca = None
                        for k in range(3):
                            cv = av * mpmath.exp((abs(vel[k]) - v0p) / rv)
                            cv_tot += cv * vn * dt
                            ca = aa * mpmath.exp((abs(acc[k]) - a0p) / ra)
                            ca_tot += ca * vn * dt
                        for k in range(3):
                            gv = (av / rv) * mpmath.exp((abs(vel[k]) - v0p) / rv)
                            ga = (aa / ra) * mpmath.exp((abs(acc[k]) - a0p) / ra)
                            for i in range(6):
                                h[k][i] += (gv * vn * TV[i] + cv * (vel[k] / vn) * TV[i]) * dt
                                h[k][i] += (ga * vn * TVV[i] + ca * (vel[k] / vn) * TV[i]) * dt
                    t += dt_d
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


def _case(m, kind, origin, T_first, seed, rows=2):
    org, res, grid, dist = _map(kind, origin, seed=seed)
    rng = np.random.default_rng(seed)
    size = np.array(grid) * res
    lo, hi = org + 0.4, org + size - 0.4
    Ts, Dfs, xs = [], [], []
    for _ in range(rows):
        wp = lo + rng.random((m + 1, 3)) * (hi - lo)
        T = rng.uniform(0.3, 0.9, size=m)
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
      dict(enable_dyn=1, alpha_v=1.0, r_v=4.0, v0=2.5, alpha_a=1.0, r_a=15.0, a0=3.5)]
CASES = [(m, kind, origin, T0, kw_i)
         for i, (m, kind, origin, T0) in enumerate([
             (2, "random", (0.0, 0.0, 0.0), 2.0), (3, "constant", (-1.0, -1.5, 0.0), 0.0299),
             (4, "linear", (-500.0, 300.0, 0.0), 0.0301), (5, "signed", (0.0, 0.0, 0.0), 0.5),
             (6, "random", (-500.0, 300.0, 0.0), 0.0299), (7, "linear", (0.0, 0.0, 0.0), 2.0),
             (13, "random", (-1.0, -1.5, 0.0), 0.0301)])
         for kw_i in ([0, 4] if m in (3, 6) else [i % len(KW)])]


@pytest.fixture(scope="module")
def evaluated(oracle_mod):
    """Every case: the oracle with its magnitudes, the exact values, the inputs."""
    out = []
    for j, (m, kind, origin, T0, kw_i) in enumerate(CASES):
        (org, res, grid, dist), T, Df, x = _case(m, kind, origin, T0, seed=30 + j, rows=1 if m == 13 else 2)
        kw = dict(KW[kw_i])
        sdf = oracle_mod.Sdf(org, res, grid, dist.reshape(-1))
        twin_sdf = np_twin.Sdf(org, res, grid, dist)
        p = dict(oracle_mod.OPTI_NODE_PARAMS)
        p.update(kw)
        ref = oracle_mod.eval_batch_mag(T, Df, x, sdf, oracle_mod.make_params(**kw))
        exact = []
        for b in range(len(x)):
            c, g = exact_cost_grad(T[b], Df[b], x[b], twin_sdf, p)
            exact.append((float(c), np.array([float(v) for a in range(3) for v in g[a]])))
        out.append(dict(case=CASES[j], T=T, Df=Df, x=x, p=p, sdf=twin_sdf, ref=ref, exact=exact))
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


def _twin(ev, b):
    c, g, _ = np_twin.cost_grad(ev["T"][b], ev["Df"][b], ev["x"][b], ev["sdf"], ev["p"])
    return c, g


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
        for b, e in enumerate(ev["exact"]):
            if _tie(ev["ref"], b):
                continue
            c, g = _twin(ev, b)
            worst = max(worst, *_excess(c, g, e, ev["ref"], b))
    assert worst > KAPPA64, (mutation, worst)
