"""The callback with a gradient MODE, restated in numpy independently of the library (include/gtop.h,
gtop_set_gradient_mode): src/grad_traj_optimizer.cpp:281-432 as oracle/np_twin.py's cost_grad has it, with

    mode 0 (GTOP_GRADIENT_REFERENCE)   the reference's gradient, line by line — the spurious factor cd on the
                                       collision gradient (:376-381), and in the enable_dyn block (:383-407) the last
                                       axis's cv, ca, no sign factors;
    mode 1 (GTOP_GRADIENT_CONSISTENT)  the derivative of the cost that is returned, with the float round trips taken
                                       as the identity, the field as differentiable inside a cell and
                                       d vel_norm / d v = v / vel_norm:
        g_colli.row(k) += ( gd*grad(k)*vel_norm * T*Ldp + cd*(vel(k)/vel_norm) * T*V*Ldp ) * dt
        S = sum_j (cv_j + ca_j)
        g_vel.row(k)   += ( gv_k*sgn(vel(k))*vel_norm + S*vel(k)/vel_norm ) * T*V*Ldp * dt
        g_acc.row(k)   += ( ga_k*sgn(acc(k))*vel_norm ) * T*V*V*Ldp * dt,          sgn(+-0) = 0.

The COST is computed by the same statements in both modes.  `sdf` is duck-typed — anything with query(pos) ->
(dist, grad(3)), asked once per sample in (segment, sample) order — so oracle.Sdf, np_twin.Sdf, a closed-form field
and tests/moving_twin.TimedLookup all plug in.  Pure-Python loops: small cases only."""
import math

import numpy as np

from oracle import np_twin

REFERENCE, CONSISTENT = 0, 1


# the reference's float locals (:457-465, :477-485) and its two "+1e-5" constants (:358, :425-432): module attributes, as
# in np_twin, so that a test can switch the round trips off (finite differences) or evaluate a deliberately wrong variant
def to_float(v):
    return np.float64(np.float32(v))


VN_EPS = 1e-5
GRAD_EPS = 1e-5


def _sgn(v):
    return float(int(v > 0) - int(v < 0))


def cost_grad(T, Df, x, sdf, p, mode=REFERENCE, gen=None):
    """One evaluation.  p: np_twin's parameter dict (ws, wc, alpha, r, d0, step, enable_dyn, alpha_v, r_v, v0, alpha_a,
    r_a, a0).  Returns cost, grad (9(m-1),), dict(g_colli, g_dyn (3, 3m-3) — the collision and the enable_dyn parts
    of the gradient, unweighted and weighted as the callback adds them —, cost_colli, cost_dyn)."""
    assert mode in (REFERENCE, CONSISTENT)
    T = np.asarray(T, dtype=np.float64)
    m = len(T)
    ndp = 3 * m - 3
    gen = gen or np_twin.generator(T)
    L, R = gen["L"], gen["R"]
    Rfp, Rpp = R[:6, 6:], R[6:, 6:]
    Df = np.asarray(Df, dtype=np.float64).reshape(3, 6)
    dp = np.asarray(x, dtype=np.float64).reshape(3, ndp)                    # axis-major (:182-187)
    d = np.hstack([Df, dp])
    cost_smooth = sum(float(d[a] @ R @ d[a]) for a in range(3))            # :326-327
    g_smooth = np.stack([2 * Rfp.T @ Df[a] + 2 * Rpp @ dp[a] for a in range(3)])  # :330-336
    coe = np.zeros((m, 18))                                                 # :253-279
    for a in range(3):
        coe[:, 6 * a:6 * a + 6] = (L @ d[a]).reshape(m, 6)
    V = np.zeros((6, 6))                                                    # :104-105
    for i in range(5):
        V[i, i + 1] = i + 1
    dyn = bool(p.get("enable_dyn", 0)) and p["step"] == 2                   # :383

    g_colli = np.zeros((3, ndp))
    g_dyn = np.zeros((3, ndp))
    cost_colli = cost_dyn = 0.0
    for s in range(m):
        if abs(p["wc"]) < 1e-4:                                             # :346
            break
        Ldp = L[6 * s:6 * s + 6, 6:]                                        # :348
        VL, VVL = V @ Ldp, V @ V @ Ldp
        dt = T[s] / 30.0                                                    # :351
        t = 1e-3
        while t < T[s]:                                                     # :353
            Tm = np.array([math.pow(t, i) for i in range(6)])               # :544-551
            pos, vel, acc = np.zeros(3), np.zeros(3), np.zeros(3)
            for a in range(3):
                c = coe[s, 6 * a:6 * a + 6]
                pos[a] = to_float(c[0] + c[1] * t + c[2] * t ** 2 + c[3] * t ** 3 + c[4] * t ** 4 + c[5] * t ** 5)
                vel[a] = to_float(c[1] + 2 * c[2] * t + 3 * c[3] * t ** 2 + 4 * c[4] * t ** 3 + 5 * c[5] * t ** 4)
                acc[a] = to_float(2 * c[2] + 6 * c[3] * t + 12 * c[4] * t ** 2 + 20 * c[5] * t ** 3)
            vn = math.sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) + VN_EPS   # :358
            dist, g = sdf.query(pos)                                        # :363
            e = math.exp(-(dist - p["d0"]) / p["r"])
            cd = p["alpha"] * e                                             # :509
            gd = -(p["alpha"] / p["r"]) * e                                 # :514
            cost_colli += cd * vn * dt                                      # :373
            for k in range(3):                                              # :376-381
                w1 = gd * g[k] * vn if mode == CONSISTENT else gd * g[k] * cd * vn
                g_colli[k] += (w1 * (Tm @ Ldp) + cd * (vel[k] / vn) * (Tm @ VL)) * dt
            if dyn:                                                         # :383-407, formulas :517-535
                cv = [p["alpha_v"] * math.exp((abs(vel[k]) - p["v0"]) / p["r_v"]) for k in range(3)]
                ca = [p["alpha_a"] * math.exp((abs(acc[k]) - p["a0"]) / p["r_a"]) for k in range(3)]
                for k in range(3):
                    cost_dyn += cv[k] * vn * dt
                    cost_dyn += ca[k] * vn * dt
                S = (cv[0] + cv[1] + cv[2]) + (ca[0] + ca[1] + ca[2])
                for k in range(3):
                    gv, ga = cv[k] / p["r_v"], ca[k] / p["r_a"]
                    if mode == CONSISTENT:
                        g_dyn[k] += ((gv * _sgn(vel[k]) * vn + S * (vel[k] / vn)) * (Tm @ VL)
                                     + ga * _sgn(acc[k]) * vn * (Tm @ VVL)) * dt
                    else:   # the values the cost loop left behind: the last axis's, on both rows; no sign factor
                        g_dyn[k] += ((gv * vn + cv[2] * (vel[k] / vn)) * (Tm @ VL)
                                     + ga * vn * (Tm @ VVL) + ca[2] * (vel[k] / vn) * (Tm @ VL)) * dt
            t += dt

    ws = 0.0 if p["step"] == 1 else p["ws"]                                 # :412-415
    cost = ws * cost_smooth + p["wc"] * cost_colli + cost_dyn + 1e-3        # :417-418
    grad = (ws * g_smooth + p["wc"] * g_colli + g_dyn) + GRAD_EPS           # :425-432
    return cost, grad.reshape(-1), dict(g_colli=g_colli, g_dyn=g_dyn, cost_colli=cost_colli, cost_dyn=cost_dyn)


def eval_batch(T, Df, x, sdf, p, mode=REFERENCE):
    """Rows of a batch: T (B, m), Df (B, 3, 6), x (B, n)."""
    B = x.shape[0]
    cost, grad = np.empty(B), np.empty_like(x, dtype=np.float64)
    for b in range(B):
        cost[b], grad[b], _ = cost_grad(T[b], Df[b], x[b], sdf, p, mode)
    return cost, grad
