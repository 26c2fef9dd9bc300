"""Moving obstacles on polynomial predictions (include/gtop.h, gtop_set_moving_box_polynomials) restated independently
of the library.

The centre of box b at time tau, axis k — the interface fixes the arithmetic:

    tc  = fmin(fmax(tau, t1[b]), t2[b])                       (no clamp without t_range)
    c_k = fma(fma(fma(fma(fma(c5, tc, c4), tc, c3), tc, c2), tc, c1), tc, c0)        fp64

Python 3.10 has no fma, so every step is formed in exact rational arithmetic and rounded once.  fma_fraction is that
sentence in fractions.Fraction, literally; fma is the same value from the operands' integer ratios (every finite double
is n / 2^k, and int / int is correctly rounded), some ten times faster — tests/test_box_polynomials.py holds the two
equal on every step of its random draws.

The lookup: tests/moving_twin.TimedLookup with, per query, every box parked at its centre at that query's tau — the C
oracle's evaluateEDTWithGrad(pos, tau, p0 = centre, vel = 0, scale); centre + 0 * tau is exact, so the already-tested
oracle does everything from the faces on."""
from fractions import Fraction

import numpy as np

from oracle import np_twin
from tests import moving_twin
from tests import validate_twin as vt


def fma_fraction(a, b, c):
    """round(a * b + c), the product and the sum exact: one correctly rounded float() of the rational result."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma(a, b, c):
    """fma_fraction's value from integer ratios (finite operands)."""
    an, ad = float(a).as_integer_ratio()
    bn, bd = float(b).as_integer_ratio()
    cn, cd = float(c).as_integer_ratio()
    pd = ad * bd                       # denominators are powers of two
    if pd >= cd:
        num, den = an * bn + cn * (pd // cd), pd
    else:
        num, den = an * bn * (cd // pd) + cn, cd
    return num / den                   # int / int: correctly rounded


def clamp_time(tau, t1=-np.inf, t2=np.inf):
    """fmin(fmax(tau, t1), t2) for a non-NaN tau."""
    tc = t1 if tau < t1 else tau
    return t2 if tc > t2 else tc


def centre_axis(c6, tc, fma_=fma):
    """Horner from the highest power down, one fma per step.  c6: ascending powers."""
    r = float(c6[5])
    for i in (4, 3, 2, 1, 0):
        r = fma_(r, tc, c6[i])
    return r


def centres(coef, tau, t_range=None, fma_=fma):
    """(nbox, 3) centres at the scalar time tau.  coef (nbox, 3, 6); t_range (nbox, 2) or None."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 3, 6)
    out = np.empty((coef.shape[0], 3))
    for b in range(coef.shape[0]):
        tc = float(tau) if t_range is None else clamp_time(float(tau), float(t_range[b][0]), float(t_range[b][1]))
        for k in range(3):
            out[b, k] = centre_axis(coef[b, k], tc, fma_)
    return out


def coefficients(w, v, a, when):
    """c(t) = w + v (t - when) + a (t - when)^2 / 2 expanded in powers of t: (nbox, 3, 6), c3 .. c5 = 0.  (The expansion
    is ordinary fp64 arithmetic: it DEFINES the list the tests use; nothing compares against the unexpanded form.)"""
    w, v, a = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (w, v, a))
    when = np.asarray(when, dtype=np.float64).reshape(-1, 1)
    coef = np.zeros((w.shape[0], 3, 6))
    coef[:, :, 0] = w - v * when + 0.5 * a * when * when
    coef[:, :, 1] = v - a * when
    coef[:, :, 2] = 0.5 * a
    return coef


def constant_velocity_part(coef):
    """(p0, vel) = (c0, c1) of every box: what a constant-velocity list can say about the same obstacles."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 3, 6)
    return coef[:, :, 0].copy(), coef[:, :, 1].copy()


class PolyLookup(moving_twin.TimedLookup):
    """sdf.query(pos) for np_twin.cost_grad / consistent_twin.cost_grad: evaluateEDTWithGrad(pos, tau_k) against the
    polynomial boxes, for the k-th call."""

    def __init__(self, osdf, taus, coef, scale, t_range=None):
        coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1, 3, 6)
        zero = np.zeros((coef.shape[0], 3))
        super().__init__(osdf, taus, zero, zero, scale)
        self.coef = coef
        self.t_range = None if t_range is None else np.asarray(t_range, dtype=np.float64).reshape(-1, 2)

    def query(self, pos):
        tau = self.taus[self.k]
        self.p0 = centres(self.coef, tau, self.t_range) if tau >= 0.0 else self.p0   # (tau < 0: static only)
        return super().query(pos)


def cost_grad(T, Df, x, osdf, p, coef, scale, t_range=None, t0=0.0, gen=None, callback=None):
    """One callback evaluation, as moving_twin.cost_grad returns it.  callback: np_twin.cost_grad's signature with the
    lookup in the sdf slot (consistent_twin.cost_grad with its mode bound, for instance)."""
    taus = moving_twin.sample_times(T, t0)
    look = PolyLookup(osdf, taus, coef, scale, t_range)
    cost, grad, _ = (callback or np_twin.cost_grad)(T, Df, x, look, p, gen=gen)
    assert look.k == len(taus)
    info = dict(base_idx=np.array(look.base_idx).reshape(-1, 3), lowered=np.array(look.lowered, dtype=bool), tau=taus,
                dist=np.array(look.dist))
    return cost, grad, info


def eval_batch(T, Df, x, osdf, p, coef, scale, t_range=None, t0=None, callback=None):
    B = x.shape[0]
    t0 = np.broadcast_to(0.0 if t0 is None else np.asarray(t0, dtype=np.float64), (B,))
    cost, grad, infos = np.empty(B), np.empty_like(x), []
    for b in range(B):
        cost[b], grad[b], info = cost_grad(T[b], Df[b], x[b], osdf, p, coef, scale, t_range, t0[b], callback=callback)
        infos.append(info)
    return cost, grad, infos


def edt_query(osdf, pos, tau, coef, scale, t_range=None):
    """evaluateEDTWithGrad for each (pos, tau) against the polynomial boxes: (dist (N,), grad (N, 3))."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (pos.shape[0],))
    scale = np.asarray(scale, dtype=np.float64).reshape(-1, 3)
    zero = np.zeros_like(scale)
    d, g = np.empty(pos.shape[0]), np.empty((pos.shape[0], 3))
    for i in range(pos.shape[0]):
        c = centres(coef, tau[i], t_range) if tau[i] >= 0.0 else zero
        di, gi = osdf.edt_query(pos[i], tau[i], c, zero, scale)
        d[i], g[i] = di[0], gi[0]
    return d, g


def report(oracle_mod, coeff, T, osdf, margin, coef, scale, t_range=None, t0=0.0, dt=0.01, max_samples=8192):
    """validate_twin.report with use_boxes against the polynomial boxes: (r (12,), dict(points, dist, tau, ...))."""
    kin = vt.kinematics(coeff, T, dt)
    n, pts = oracle_mod.traj_samples(coeff, T, dt, max_samples)
    assert n == len(kin["t"]) <= max_samples, (n, len(kin["t"]))
    tau = np.float64(t0) + kin["t"]
    dist, _ = edt_query(osdf, pts, tau, coef, scale, t_range)
    oom = vt.out_of_map(pts, np.array(osdf.c.min_range[:]), np.array(osdf.c.max_range[:]))
    assert np.all(dist[oom] == -1.0)
    return vt.reduce_report(kin["t"], dist, oom, kin, margin), dict(points=pts, dist=dist, tau=tau, out=oom, **kin)
