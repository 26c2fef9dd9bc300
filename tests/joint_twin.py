"""The joint pass over waypoint values and segment times, and the optimizer of the stacked variable, restated in numpy
independently of the library (include/gtop_joint.h).  The cost, gT and parts ARE tests/time_twin.cost_gradT's (called,
not restated: the same bits); gx is formed here sample by sample in the header's h_j form — the polynomials
h_j(t) = d p(t) / d d_j of the table, evaluated per sample — where the kernel sums moments and applies the table once: two
routes to the same sums.  The optimizer is oracle/mma_twin.minimize on z = [x | T] with this twin's F and gradient.

`sdf` is duck-typed as in time_twin (query(pos) -> (dist, grad(3))); it is asked twice per sample (once by time_twin,
once here), so it must be stateless.  Pure-Python loops: small cases only.

`mutant` evaluates a deliberately wrong variant (tests/test_joint_twin.py): "no_start" drops the junction's start part,
"swapped" adds the start part of the segment before and the end part of the segment behind, "bad_table" gets
d c4 / d vT wrong, "no_jerk" leaves the jerk chain out of gx, "no_rho" leaves rho out of F (not out of its gradient)."""
import math

import numpy as np

from oracle import mma_twin
from tests import consistent_twin as ct
from tests import time_twin as tt

INFO = 8
MUTANTS = ("no_start", "swapped", "bad_table", "no_jerk", "no_rho")


def table(T, mutant=None):
    """H (6, 6): H[j, n] = d c_n / d d_j for d = (p0, v0, a0, pT, vT, aT) (include/gtop_joint.h)."""
    H = np.zeros((6, 6))
    H[0, 0], H[1, 1], H[2, 2] = 1.0, 1.0, 0.5
    H[:, 3] = [-10 / T ** 3, -6 / T ** 2, -3 / (2 * T), 10 / T ** 3, -4 / T ** 2, 1 / (2 * T)]
    H[:, 4] = [15 / T ** 4, 8 / T ** 3, 3 / (2 * T ** 2), -15 / T ** 4, (8 if mutant == "bad_table" else 7) / T ** 3,
               -1 / T ** 2]
    H[:, 5] = [-6 / T ** 5, -3 / T ** 4, -1 / (2 * T ** 3), 6 / T ** 5, -3 / T ** 4, 1 / (2 * T ** 3)]
    return H


def segment_gradient(Ts, w0, w1, sdf, p, mutant=None):
    """(3 axes, 6): d (the segment's weighted cost) / d (p0, v0, a0, pT, vT, aT) per axis."""
    ws = 0.0 if p["step"] == 1 else p["ws"]
    dyn = bool(p.get("enable_dyn", 0)) and p["step"] == 2
    colli = not abs(p["wc"]) < 1e-4
    c, _ = tt.segment_coefficients(Ts, w0, w1)
    H = table(Ts, mutant)
    g = np.zeros((3, 6))
    if mutant != "no_jerk":
        for k in range(3):
            c3, c4, c5 = c[k, 3:]
            q3 = 36 * Ts * c3 + 72 * Ts ** 2 * c4 + 120 * Ts ** 3 * c5
            q4 = 72 * Ts ** 2 * c3 + 192 * Ts ** 3 * c4 + 360 * Ts ** 4 * c5
            q5 = 120 * Ts ** 3 * c3 + 360 * Ts ** 4 * c4 + 720 * Ts ** 5 * c5
            g[k] += ws * 2.0 * (q3 * H[:, 3] + q4 * H[:, 4] + q5 * H[:, 5])
    if not colli:
        return g
    dt = Ts / 30.0
    t = 1e-3
    while t < Ts:
        pw = np.array([t ** j for j in range(6)])
        d1 = np.array([j * t ** (j - 1) if j >= 1 else 0.0 for j in range(6)])
        d2 = np.array([j * (j - 1) * t ** (j - 2) if j >= 2 else 0.0 for j in range(6)])
        h, h1, h2 = H @ pw, H @ d1, H @ d2                                      # h_j, h_j', h_j'' at t
        pos, vel, acc = np.zeros(3), np.zeros(3), np.zeros(3)
        for k in range(3):
            pos[k] = ct.to_float(float(c[k] @ pw))
            vel[k] = ct.to_float(float(c[k] @ d1))
            acc[k] = ct.to_float(float(c[k] @ d2))
        vn = math.sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) + ct.VN_EPS
        dist, grad = sdf.query(pos)
        ex = math.exp(-(dist - p["d0"]) / p["r"])
        cd, gd = p["alpha"] * ex, -(p["alpha"] / p["r"]) * ex
        if dyn:
            cv = [p["alpha_v"] * math.exp((abs(vel[k]) - p["v0"]) / p["r_v"]) for k in range(3)]
            ca = [p["alpha_a"] * math.exp((abs(acc[k]) - p["a0"]) / p["r_a"]) for k in range(3)]
            S = sum(cv) + sum(ca)
        for k in range(3):
            g[k] += p["wc"] * (gd * grad[k] * vn * dt * h + cd * (vel[k] / vn) * dt * h1)
            if dyn:
                g[k] += ((cv[k] / p["r_v"] * tt._sgn(vel[k]) * h1 + ca[k] / p["r_a"] * tt._sgn(acc[k]) * h2) * vn * dt
                         + S * (vel[k] / vn) * dt * h1)
        t += dt
    return g


def cost_grad(T, Df, x, sdf, p, mutant=None):
    """One pass -> cost, gx (9 (m - 1),) laid out as x, gT (m,), parts (m, 4)."""
    T = np.asarray(T, dtype=np.float64)
    m = len(T)
    cost, gT, parts = tt.cost_gradT(T, Df, x, sdf, p)
    w = tt.waypoint_rows(Df, x, m)
    seg = [segment_gradient(float(T[s]), w[s], w[s + 1], sdf, p, mutant) for s in range(m)]
    gx = np.zeros((3, 3 * m - 3))
    for wp in range(1, m):
        end, start = seg[wp - 1][:, 3:], seg[wp][:, :3]
        if mutant == "swapped":
            end, start = seg[wp - 1][:, :3], seg[wp][:, 3:]
        if mutant == "no_start":
            start = 0.0
        gx[:, 3 * (wp - 1):3 * wp] = end + start
    return cost, gx.reshape(-1), gT, parts


def gradient_batch(T, Df, x, sdf, p):
    """Rows of a batch: T (B, m) or (m,), Df (B, 3, 6), x (B, n) -> cost (B,), gx (B, n), gT (B, m), parts (B, m, 4)."""
    B = x.shape[0]
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (B, np.shape(T)[-1]))
    out = [cost_grad(T[b], Df[b], x[b], sdf, p) for b in range(B)]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def F_grad(z, m, Df, sdf, p, rho, mutant=None):
    """F = cost + rho sum(T) and its gradient [gx | gT + rho] at z = [x | T]."""
    n = 9 * (m - 1)
    cost, gx, gT, _ = cost_grad(z[n:], Df, z[:n], sdf, p, mutant)
    F = cost if mutant == "no_rho" else cost + rho * float(np.sum(z[n:]))
    return F, np.concatenate([gx, gT + rho]), cost


def bounds(m, lb, ub, rho, t_min, t_max, T_lo=None):
    """The packed bounds of z: [lb | lo], [ub | hi]; lo_s > t_max pins the segment (lo = hi)."""
    lo = np.full(m, float(t_min)) if T_lo is None else np.maximum(t_min, np.asarray(T_lo, dtype=np.float64))
    hi = np.where(lo > t_max, lo, float(t_max))
    return np.concatenate([lb, lo]), np.concatenate([ub, hi])


def optimize(T, Df, x, sdf, p, lb, ub, rho, t_min, t_max, max_evals, ftol_rel=0.0, xtol_rel=0.0, T_lo=None,
             observe=None, observe_outer=None):
    """oracle/mma_twin.minimize on z -> (x_out, T_out, info (8,), the minimiser's dict)."""
    T = np.asarray(T, dtype=np.float64)
    m, n = len(T), 9 * (len(T) - 1)
    zlb, zub = bounds(m, np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64), rho, t_min, t_max, T_lo)

    def f(z):
        F, g, _ = F_grad(z, m, Df, sdf, p, rho)
        return F, g

    res = mma_twin.minimize(f, np.concatenate([np.asarray(x, dtype=np.float64), T]), zlb, zub, max_evals, ftol_rel, xtol_rel,
                            observe=observe, observe_outer=observe_outer)
    z = res["x"]
    F, g, cost = F_grad(z, m, Df, sdf, p, rho)
    held = (zlb >= zub) | ((z <= zlb) & (g > 0.0)) | ((z >= zub) & (g < 0.0))
    a = np.where(held, 0.0, np.abs(g))
    info = np.array([res["code"], res["nevals"], res["fs"][0], res["minf"], cost, float(np.sum(z[n:])),
                     float(np.max(a[:n])), float(np.max(a[n:]))])
    return z[:n], z[n:], info, res
