#!/usr/bin/env python3
"""A known answer for the CONSISTENT gradient mode (include/gtop.h, gtop_set_gradient_mode) derived by hand from its
formulas (tests/golden/CONSISTENT_ANALYTIC.md has the derivation), independent of tests/consistent_twin.py, the oracle
and the HIP kernels: no matrix is built or inverted and no field is interpolated.

  D  constant ACCELERATION along x: p(tau) = p0 + v0 tau + a tau^2 / 2 on the global clock, y and z constant;
     alpha = 0 (no collision penalty), the enable_dyn block on
       every segment's polynomial is that parabola re-expanded (c3 = c4 = c5 = 0): jerk cost and gradient vanish;
       vel = (v0 + a tau, 0, 0) through `float`, acc = (a, 0, 0): cost and gradient are explicit finite sums over
       the 30 sample times of each segment,
       cost      = sum_s dt sum_i S_i vn_i + 1e-3,                  S_i = sum_k (cv_k + ca_k) at sample i
       grad_x,j  = sum_s dt sum_i [ (gv_x,i vn_i + S_i v_i / vn_i) phi'_{s,j}(t_i) + ga_x vn_i phi''_{s,j}(t_i) ] + 1e-5
       grad_y,j = grad_z,j = 1e-5 exactly: sgn(0) = 0 on the penalties' own terms, vel_k = 0 on the d|v|/dx term.

phi_{s,j}: the quintic Hermite basis of make_analytic.py, whose helpers this file reuses.

usage: python tests/golden/make_consistent_analytic.py   (writes tests/golden/consistent_analytic.npz)"""
import importlib.util
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_analytic", os.path.join(HERE, "make_analytic.py"))
ma = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ma)


def main():
    prm = dict(ws=1.0, wc=5.0, alpha=0.0, r=0.5, d0=0.8, alpha_v=2.0, r_v=0.5, v0=1.0, alpha_a=1.5, r_a=1.0, a0=1.0,
               step=2, enable_dyn=1)
    m, v0, a, T, p0 = 4, 1.0, 0.4, 1.0, (-3.5, 0.5, 1.5)    # 7.2 m along x inside the 12 x 6 x 6 m map
    n = 9 * (m - 1)

    def state(tau):                                         # (p, v, a) along x on the global clock
        return p0[0] + v0 * tau + 0.5 * a * tau * tau, v0 + a * tau, a

    Df = np.zeros((3, 6))
    x = np.zeros(n)
    Df[0] = list(state(0.0)) + list(state(m * T))
    Df[1] = [p0[1], 0, 0, p0[1], 0, 0]
    Df[2] = [p0[2], 0, 0, p0[2], 0, 0]
    for w in range(1, m):
        x[ma.free_index(m, 0, w, 0):ma.free_index(m, 0, w, 0) + 3] = state(w * T)
        x[ma.free_index(m, 1, w, 0)] = p0[1]
        x[ma.free_index(m, 2, w, 0)] = p0[2]
    ts, dt = ma.sample_times(T)
    assert len(ts) == 30
    cost = 0.0
    grad = np.zeros(n)
    cv_idle = prm["alpha_v"] * math.exp((0.0 - prm["v0"]) / prm["r_v"])            # the two axes at rest (:517-535)
    ca_idle = prm["alpha_a"] * math.exp((0.0 - prm["a0"]) / prm["r_a"])
    for s in range(m):
        for t in ts:
            v = ma.to_float32(state(s * T)[1] + a * t)      # c1 + 2 c2 t of the segment's own expansion, through `float`
            acc = ma.to_float32(a)
            vn = abs(v) + 1e-5                              # :358 (the other two components are 0)
            cv_x = prm["alpha_v"] * math.exp((abs(v) - prm["v0"]) / prm["r_v"])
            ca_x = prm["alpha_a"] * math.exp((abs(acc) - prm["a0"]) / prm["r_a"])
            S = (cv_x + 2 * cv_idle) + (ca_x + 2 * ca_idle)
            cost += S * vn * dt
            w_vel = (cv_x / prm["r_v"]) * 1.0 * vn + S * v / vn     # sgn(v) = 1
            w_acc = (ca_x / prm["r_a"]) * 1.0 * vn                  # sgn(a) = 1
            h1 = ma.hermite(t / T, T, 1)            # T*V*Ldp restricted to the segment's two waypoints
            h2 = ma.hermite(t / T, T, 2)            # T*V*V*Ldp
            for der in range(3):
                if 1 <= s + 1 <= m - 1:
                    grad[ma.free_index(m, 0, s + 1, der)] += (w_vel * h1[2 * der + 1] + w_acc * h2[2 * der + 1]) * dt
                if 1 <= s <= m - 1:
                    grad[ma.free_index(m, 0, s, der)] += (w_vel * h1[2 * der] + w_acc * h2[2 * der]) * dt
    cost += 1e-3
    grad += 1e-5
    keys = ["ws", "wc", "alpha", "r", "d0", "alpha_v", "r_v", "v0", "alpha_a", "r_a", "a0", "step", "enable_dyn"]
    np.savez(os.path.join(HERE, "consistent_analytic.npz"), grid=np.array((60, 30, 30)), resolution=0.2,
             origin=np.array((-6.0, -3.0, 0.0)), pkeys=np.array(keys), D_params=np.array([prm[k] for k in keys], dtype=float),
             D_T=np.full(m, T), D_Df=Df, D_x=x, D_cost=cost, D_grad=grad)
    print(cost, grad)


if __name__ == "__main__":
    main()
