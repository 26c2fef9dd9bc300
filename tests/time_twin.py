"""The derivative of the cost with respect to the segment times, and the optimizer of the time allocation, restated in
numpy independently of the library (include/gtop_time.h): the cost is tests/consistent_twin.cost_grad's (src/
grad_traj_optimizer.cpp:281-432), formed segment by segment from the closed-form quintic of each segment — with the
waypoint values held in x and Df, segment s depends on T_s alone — and differentiated under the conventions of
GTOP_GRADIENT_CONSISTENT: the float round trips as the identity, the field as differentiable inside a cell,
d vel_norm / d v = v / vel_norm, sgn(+-0) = 0, the sample count held fixed and d t_i / d T_s = i / 30.

`sdf` is duck-typed as in consistent_twin: anything with query(pos) -> (dist, grad(3)), asked once per sample in
(segment, sample) order.  The float round trip and the 1e-5 of vel_norm are consistent_twin's module attributes
(to_float, VN_EPS), so a test that switches them there switches them here.  Pure-Python loops: small cases only.

`mutant` evaluates a deliberately wrong derivative (tests/test_time_twin.py): "no_i30" drops the i/30 terms, "no_vn30"
the cd vn / 30 term of the weight dt, "bad_cprime" gets c4' wrong, "no_jerk_explicit" drops the explicit d/dT of the
jerk integral."""
import math

import numpy as np

from tests import consistent_twin as ct

PARTS = 4
INFO = 8
FTOL, XTOL, MAXEVAL = 3, 4, 5
MUTANTS = ("no_i30", "no_vn30", "bad_cprime", "no_jerk_explicit")


def _sgn(v):
    return float(int(v > 0) - int(v < 0))


def waypoint_rows(Df, x, m):
    """(m + 1, 3 axes, 3) position, velocity, acceleration of every waypoint (src/qp_generator.cpp:363-387: Df holds
    start | end per axis, x the interior waypoints axis-major)."""
    Df = np.asarray(Df, dtype=np.float64).reshape(3, 6)
    dp = np.asarray(x, dtype=np.float64).reshape(3, 3 * m - 3)
    w = np.zeros((m + 1, 3, 3))
    w[0], w[m] = Df[:, :3], Df[:, 3:]
    for i in range(1, m):
        w[i] = dp[:, 3 * (i - 1):3 * i]
    return w


def segment_coefficients(T, w0, w1, mutant=None):
    """c (3, 6) = A^-1(T) d and dc (3, 6) = d c / d T of one segment (rows of A: src/qp_generator.cpp:185-195)."""
    c, dc = np.zeros((3, 6)), np.zeros((3, 6))
    for k in range(3):
        p0, v0, a0 = w0[k]
        pT, vT, aT = w1[k]
        P = pT - p0 - v0 * T - 0.5 * a0 * T * T
        V = (vT - v0 - a0 * T) * T
        A = (aT - a0) * T * T
        dP = -v0 - a0 * T
        dV = vT - v0 - 2.0 * a0 * T
        dA = 2.0 * (aT - a0) * T
        c[k, :3] = p0, v0, 0.5 * a0
        c[k, 3] = (10 * P - 4 * V + 0.5 * A) / T ** 3
        c[k, 4] = (7 * V - 15 * P - A) / T ** 4
        c[k, 5] = (6 * P - 3 * V + 0.5 * A) / T ** 5
        dc[k, 3] = (10 * dP - 4 * dV + 0.5 * dA) / T ** 3 - 3 * c[k, 3] / T
        dc[k, 4] = (7 * dV - 15 * dP - dA) / T ** 4 - (3 if mutant == "bad_cprime" else 4) * c[k, 4] / T
        dc[k, 5] = (6 * dP - 3 * dV + 0.5 * dA) / T ** 5 - 5 * c[k, 5] / T
    return c, dc


def jerk_term(T, c, dc, mutant=None):
    """c'Qc of one segment (Q: src/qp_generator.cpp:226-234) and its derivative with respect to T."""
    J = dJ = 0.0
    for k in range(3):
        c3, c4, c5 = c[k, 3:]
        q3 = 36 * T * c3 + 72 * T ** 2 * c4 + 120 * T ** 3 * c5
        q4 = 72 * T ** 2 * c3 + 192 * T ** 3 * c4 + 360 * T ** 4 * c5
        q5 = 120 * T ** 3 * c3 + 360 * T ** 4 * c4 + 720 * T ** 5 * c5
        J += c3 * q3 + c4 * q4 + c5 * q5
        if mutant != "no_jerk_explicit":
            dJ += (36 * c3 * c3 + 288 * T * c3 * c4 + 720 * T ** 2 * c3 * c5 + 576 * T ** 2 * c4 * c4
                   + 2880 * T ** 3 * c4 * c5 + 3600 * T ** 4 * c5 * c5)
        dJ += 2 * (q3 * dc[k, 3] + q4 * dc[k, 4] + q5 * dc[k, 5])
    return J, dJ


def cost_gradT(T, Df, x, sdf, p, mutant=None):
    """One pass.  p: np_twin's parameter dict.  Returns cost (the callback's, its 1e-3 included), gT (m,) and parts
    (m, 4): the segment's smoothness and collision + dyn cost, weighted as the callback adds them, and their two
    derivatives."""
    T = np.asarray(T, dtype=np.float64)
    m = len(T)
    w = waypoint_rows(Df, x, m)
    ws = 0.0 if p["step"] == 1 else p["ws"]                                 # :412-415
    dyn = bool(p.get("enable_dyn", 0)) and p["step"] == 2                   # :383
    colli = not abs(p["wc"]) < 1e-4                                         # :346
    i30 = 0.0 if mutant == "no_i30" else 1.0
    parts = np.zeros((m, PARTS))
    for s in range(m):
        Ts = float(T[s])
        c, dc = segment_coefficients(Ts, w[s], w[s + 1], mutant)
        J, dJ = jerk_term(Ts, c, dc, mutant)
        parts[s, 0], parts[s, 2] = ws * J, ws * dJ
        if not colli:
            continue
        dt = Ts / 30.0                                                      # :351
        t, i = 1e-3, 0
        cs = ds = 0.0
        while t < Ts:                                                       # :353
            fr = i30 * i / 30.0
            pw = [t ** j for j in range(6)]
            pos, vel, acc, pd, vd, ad = (np.zeros(3) for _ in range(6))
            for k in range(3):
                q, e = c[k], dc[k]
                pos[k] = ct.to_float(sum(q[j] * pw[j] for j in range(6)))
                vel[k] = ct.to_float(sum(j * q[j] * pw[j - 1] for j in range(1, 6)))
                acc[k] = ct.to_float(sum(j * (j - 1) * q[j] * pw[j - 2] for j in range(2, 6)))
                jerk = sum(j * (j - 1) * (j - 2) * q[j] * pw[j - 3] for j in range(3, 6))
                pd[k] = sum(e[j] * pw[j] for j in range(3, 6)) + vel[k] * fr
                vd[k] = sum(j * e[j] * pw[j - 1] for j in range(3, 6)) + acc[k] * fr
                ad[k] = sum(j * (j - 1) * e[j] * pw[j - 2] for j in range(3, 6)) + jerk * fr
            vn = math.sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) + ct.VN_EPS   # :358
            vdot = float(vel @ vd) / vn
            dist, g = sdf.query(pos)                                        # :363
            ex = math.exp(-(dist - p["d0"]) / p["r"])
            cd, gd = p["alpha"] * ex, -(p["alpha"] / p["r"]) * ex           # :509, :514
            w30 = 0.0 if mutant == "no_vn30" else 1.0 / 30.0
            cs += p["wc"] * cd * vn * dt                                    # :373
            ds += p["wc"] * (gd * float(np.asarray(g) @ pd) * vn * dt + cd * vdot * dt + cd * vn * w30)
            if dyn:                                                         # :383-407, formulas :517-535
                S = dS = 0.0
                for k in range(3):
                    cv = p["alpha_v"] * math.exp((abs(vel[k]) - p["v0"]) / p["r_v"])
                    ca = p["alpha_a"] * math.exp((abs(acc[k]) - p["a0"]) / p["r_a"])
                    S += cv + ca
                    dS += cv / p["r_v"] * _sgn(vel[k]) * vd[k] + ca / p["r_a"] * _sgn(acc[k]) * ad[k]
                cs += S * vn * dt
                ds += dS * vn * dt + S * vdot * dt + S * vn * w30
            t += dt
            i += 1
        parts[s, 1], parts[s, 3] = cs, ds
    cost = 0.0
    for s in range(m):
        cost += parts[s, 0] + parts[s, 1]
    return cost + 1e-3, parts[:, 2] + parts[:, 3], parts               # :417-418


def gradient_batch(T, Df, x, sdf, p):
    """Rows of a batch: T (B, m) or (m,), Df (B, 3, 6), x (B, n) -> cost (B,), gT (B, m), parts (B, m, 4)."""
    B = x.shape[0]
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (B, np.shape(T)[-1]))
    out = [cost_gradT(T[b], Df[b], x[b], sdf, p) for b in range(B)]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def optimize_times(T, Df, x, sdf, p, rho, t_min, t_max, first_move, ftol_rel, xtol_abs, max_evals, T_lo=None,
                   trace=None):
    """The optimizer's rule, step by step as include/gtop_time.h states it, on one row -> (T_out (m,), info (8,)).
    trace (a list): every accepted F is appended, the first one included."""
    T = np.asarray(T, dtype=np.float64)
    m = len(T)
    lo = np.full(m, float(t_min)) if T_lo is None else np.maximum(t_min, np.asarray(T_lo, dtype=np.float64))
    pinned = lo > t_max

    def clamp(v):
        return np.where(pinned, lo, np.minimum(np.maximum(v, lo), t_max))

    def ev(Tv):
        c, gT, _ = cost_gradT(Tv, Df, x, sdf, p)
        return c, c + rho * float(np.sum(Tv)), gT + rho

    Tc = clamp(T)
    cost, F, g = ev(Tc)
    F0, evals, accepted, code = F, 1, 0, XTOL
    if trace is not None:
        trace.append(F)
    gmax = float(np.max(np.abs(g)))
    if gmax > 0.0:
        a = first_move / gmax
        done = False
        while not done:
            backtracks = 0
            while True:
                Tp = clamp(Tc - a * g)
                if float(np.max(np.abs(Tp - Tc))) <= xtol_abs:
                    code, done = XTOL, True
                    break
                if evals >= max_evals:
                    code, done = MAXEVAL, True
                    break
                costp, Fp, gp = ev(Tp)
                evals += 1
                if Fp <= F + 1e-4 * float(np.sum(g * (Tp - Tc))):           # (a NaN F' is a rejection)
                    break
                a *= 0.5
                backtracks += 1
            if done:
                break
            decrease = F - Fp
            Tc, F, g, cost = Tp, Fp, gp, costp
            accepted += 1
            if trace is not None:
                trace.append(F)
            if decrease <= ftol_rel * abs(F):
                code = FTOL
                break
            if backtracks == 0:
                a *= 2.0
    held = pinned | ((Tc <= lo) & (g > 0.0)) | ((Tc >= t_max) & (g < 0.0))
    gfree = float(np.max(np.abs(g[~held]))) if np.any(~held) else 0.0
    return Tc, np.array([code, accepted, evals, F0, F, cost, gfree, float(np.sum(Tc))])
