"""The derivative of the cost with respect to the segment times and the start time under the moving-obstacle cost, and
the time optimizer on it, restated in numpy independently of the library (include/gtop_time_moving.h).

The pass is tests/time_twin.cost_gradT's — the per-segment closed form, the conventions of GTOP_GRADIENT_CONSISTENT —
with every sample looked up at its absolute time

    tau = tau_s + t,     tau_s = ((t0 + T_0) + ... ) + T_{s-1}, fp64, summed left to right (tests/moving_twin.py),

over a duck-typed `lookup.query(pos, tau) -> (dist, grad(3), dtau)`, dtau = d dist / d tau at a fixed position.  T_s
then moves its own samples by i / 30 each and every sample of every later segment by 1:

    parts[s] = [0] [1] [2] as time_twin's; [3] time_twin's + sum_i wc gd_i dtau_i (i / 30) vn_i dt;
               [4] q_s = sum_i wc gd_i dtau_i vn_i dt;  [5] R_s, R_{m-1} = 0, R_s = R_{s+1} + q_{s+1}
    gT_s = ([2] + [3]) + [5]          gt0 = R_0 + q_0.

Lookups: BoxLookup / PolyBoxLookup take dist and grad from the C oracle's already-tested evaluateEDTWithGrad
(oracle.Sdf.edt_query, tests/box_poly_twin.edt_query) and restate the corner rule's time derivative themselves;
MovingPlane is a smooth analytic field.  TimedField turns any of them into the `query(pos)` of consistent_twin.cost_grad,
the evaluation twin whose cost is differentiated.  The float round trip and the 1e-5 of vel_norm are consistent_twin's
module attributes.  Pure-Python loops: small cases only.

`mutant` evaluates a deliberately wrong derivative (tests/test_time_moving_twin.py).  In the pass: "no_cross" drops
R_s, "cross_with_own" lets R_s include the segment's own q_s, "own_no_i30" adds the own term without its i / 30.  In the
box lookups: "bad_sign_above" takes +c'_k for a corner above the slab (pt > bmax), "no_interval_zero" does not zero a
polynomial's velocity outside its interval."""
import math

import numpy as np

from tests import box_poly_twin
from tests import consistent_twin as ct
from tests import moving_twin
from tests import time_twin as tt

PARTS = 6
INFO = tt.INFO
FTOL, XTOL, MAXEVAL = tt.FTOL, tt.XTOL, tt.MAXEVAL
PASS_MUTANTS = ("no_cross", "cross_with_own", "own_no_i30")
LOOKUP_MUTANTS = ("bad_sign_above", "no_interval_zero")
MUTANTS = PASS_MUTANTS + LOOKUP_MUTANTS


# ---- lookups --------------------------------------------------------------------------------------------------------
class MovingPlane:
    """dist = n . p - (c + u tau + a tau^2 / 2): a plane moving along its normal — smooth in position and in time, and
    what trilinear interpolation of such voxel values returns exactly."""

    def __init__(self, n=(0.05, -0.03, 0.04), c=-1.5, u=0.11, a=-0.07):
        self.n, self.c, self.u, self.a = np.asarray(n, dtype=np.float64), float(c), float(u), float(a)

    def query(self, pos, tau):
        d = float(self.n @ np.asarray(pos)) - (self.c + self.u * tau + 0.5 * self.a * tau * tau)
        return d, self.n.copy(), -(self.u + self.a * tau)


class StaticLookup:
    """A lookup that does not know the time: query(pos) -> (dist, grad) of any consistent_twin field, dtau = 0."""

    def __init__(self, sdf):
        self.sdf = sdf

    def query(self, pos, tau):
        d, g = self.sdf.query(pos)
        return float(d), np.asarray(g, dtype=np.float64), 0.0


class BoxLookup:
    """evaluateEDTWithGrad(pos, tau) against constant-velocity boxes {p0, vel, scale}: dist and grad are the C oracle's
    (osdf.edt_query); dtau is the corner rule restated here.  After a query: self.lowered (a box lowered one of the 8
    corners), self.dcorner (the 8 corner derivatives), self.margins (what the test's exclusions look at)."""

    def __init__(self, osdf, p0, vel, scale, mutant=None):
        self.osdf = osdf
        self.p0, self.vel, self.scale = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in (p0, vel, scale))
        self.mutant = mutant
        self.field = osdf.dist.reshape(osdf.grid)
        self.n = np.array(osdf.grid)
        self.map_min, self.map_max = np.array(osdf.c.min_range[:]), np.array(osdf.c.max_range[:])
        self.lowered, self.dcorner, self.margins = False, np.zeros(8), {}

    # the boxes at tau as (centre (nbox, 3), velocity (nbox, 3)); dist_grad: the oracle's answer
    def boxes_at(self, tau):
        return self.p0 + self.vel * tau, self.vel

    def dist_grad(self, pos, tau):
        d, g = self.osdf.edt_query(pos, tau, self.p0, self.vel, self.scale)
        return float(d[0]), g[0]

    def time_margin(self, tau):
        return np.inf

    def query(self, pos, tau):
        pos = np.asarray(pos, dtype=np.float64)
        dist, grad = self.dist_grad(pos, tau)
        res, org = self.osdf.resolution, self.osdf.origin
        self.lowered, self.dcorner = False, np.zeros(8)
        self.margins = dict(face=np.inf, tie=np.inf, time=self.time_margin(tau))
        in_map = not (np.any(pos < self.map_min + 1e-4) or np.any(pos > self.map_max - 1e-4))
        if not in_map or tau < 0.0 or not len(self.scale):
            return dist, grad, 0.0
        idx = np.floor((pos - 0.5 * res - org) * (1.0 / res)).astype(np.int64)   # sdf_map.cpp:201-204
        diff = (pos - ((idx + 0.5) * res + org)) * (1.0 / res)                    # :206-209
        centre, cvel = self.boxes_at(tau)
        val, der = np.empty((2, 2, 2)), np.zeros((2, 2, 2))
        for x in (0, 1):
            for y in (0, 1):
                for z in (0, 1):
                    cl = np.clip(idx + (x, y, z), 0, self.n - 1)
                    val[x, y, z] = self.field[cl[0], cl[1], cl[2]]
        low = np.zeros((2, 2, 2), dtype=bool)
        for b in range(len(self.scale)):
            bmin, bmax = centre[b] - 0.5 * self.scale[b], centre[b] + 0.5 * self.scale[b]
            d1, e1 = np.zeros((3, 2)), np.zeros((3, 2))
            for k in range(3):
                for o in (0, 1):
                    pt = (idx[k] + o + 0.5) * res + org[k]
                    self.margins["face"] = min(self.margins["face"], abs(pt - bmin[k]), abs(pt - bmax[k]))
                    if pt < bmin[k]:
                        d1[k, o], e1[k, o] = bmin[k] - pt, cvel[b, k]
                    elif pt > bmax[k]:
                        d1[k, o] = pt - bmax[k]
                        e1[k, o] = cvel[b, k] if self.mutant == "bad_sign_above" else -cvel[b, k]
            for x in (0, 1):
                for y in (0, 1):
                    for z in (0, 1):
                        d2 = math.sqrt(d1[0, x] ** 2 + d1[1, y] ** 2 + d1[2, z] ** 2)
                        if not low[x, y, z]:   # (against a value a box has set, the earlier box wins a tie the same way)
                            self.margins["tie"] = min(self.margins["tie"], abs(d2 - val[x, y, z]))
                        if d2 < val[x, y, z]:                                  # strictly: the static value wins a tie
                            val[x, y, z], low[x, y, z] = d2, True
                            num = d1[0, x] * e1[0, x] + d1[1, y] * e1[1, y] + d1[2, z] * e1[2, z]
                            der[x, y, z] = num / d2 if d2 > 0.0 else 0.0
        self.lowered, self.dcorner = bool(low.any()), der.reshape(-1)
        # the trilinear blend with the value's own weights (edt_environment.cpp:104-112)
        wx, wy, wz = ((1 - diff[k], diff[k]) for k in range(3))
        dtau = sum(wx[x] * wy[y] * wz[z] * der[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1))
        return dist, grad, float(dtau)


class PolyBoxLookup(BoxLookup):
    """The same against polynomial boxes (coef (nbox, 3, 6), scale, t_range or None): the centre is
    box_poly_twin.centres', its velocity the derivative of the quintic at the clamped time inside the open interval
    and 0 outside it and at its ends."""

    def __init__(self, osdf, coef, scale, t_range=None, mutant=None):
        coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1, 3, 6)
        zero = np.zeros((coef.shape[0], 3))
        super().__init__(osdf, zero, zero, scale, mutant)
        self.coef = coef
        self.t_range = None if t_range is None else np.asarray(t_range, dtype=np.float64).reshape(-1, 2)

    def boxes_at(self, tau):
        centre = box_poly_twin.centres(self.coef, tau, self.t_range)
        vel = np.zeros_like(centre)
        for b in range(len(centre)):
            t1, t2 = (-np.inf, np.inf) if self.t_range is None else self.t_range[b]
            tc = box_poly_twin.clamp_time(float(tau), t1, t2)
            if t1 < tau < t2 or self.mutant == "no_interval_zero":
                for k in range(3):
                    c = self.coef[b, k]
                    vel[b, k] = c[1] + tc * (2 * c[2] + tc * (3 * c[3] + tc * (4 * c[4] + tc * 5 * c[5])))
        return centre, vel

    def dist_grad(self, pos, tau):
        d, g = box_poly_twin.edt_query(self.osdf, pos, tau, self.coef, self.scale, self.t_range)
        return float(d[0]), g[0]

    def time_margin(self, tau):
        return np.inf if self.t_range is None else float(np.min(np.abs(self.t_range - tau)))


class TimedField:
    """query(pos) for consistent_twin.cost_grad / np_twin.cost_grad: lookup.query(pos, taus[k]) for the k-th call."""

    def __init__(self, lookup, taus):
        self.lookup, self.taus, self.k = lookup, taus, 0

    def query(self, pos):
        d, g, _ = self.lookup.query(pos, self.taus[self.k])
        self.k += 1
        return d, g


def eval_cost(T, Df, x, lookup, p, t0=0.0):
    """The evaluation twin's cost at (T, t0): consistent_twin.cost_grad over the lookup at moving_twin's sample times."""
    field = TimedField(lookup, moving_twin.sample_times(T, t0))
    return ct.cost_grad(T, Df, x, field, p, ct.CONSISTENT)[0]


# ---- the pass ---------------------------------------------------------------------------------------------------------
def cost_gradT(T, Df, x, lookup, p, t0=0.0, mutant=None):
    """One pass.  p: np_twin's parameter dict.  Returns cost (the callback's, its 1e-3 included), gT (m,), gt0, parts
    (m, 6) and lowered (m,) — whether a box lowered a corner of any of the segment's samples (False for a lookup that
    does not say)."""
    T = np.asarray(T, dtype=np.float64)
    m = len(T)
    w = tt.waypoint_rows(Df, x, m)
    ws = 0.0 if p["step"] == 1 else p["ws"]                                 # :412-415
    dyn = bool(p.get("enable_dyn", 0)) and p["step"] == 2                   # :383
    colli = not abs(p["wc"]) < 1e-4                                         # :346
    parts = np.zeros((m, PARTS))
    lowered = np.zeros(m, dtype=bool)
    start = np.float64(t0)
    for s in range(m):
        Ts = float(T[s])
        c, dc = tt.segment_coefficients(Ts, w[s], w[s + 1])
        J, dJ = tt.jerk_term(Ts, c, dc)
        parts[s, 0], parts[s, 2] = ws * J, ws * dJ
        if colli:
            dt = Ts / 30.0                                                  # :351
            t, i = 1e-3, 0
            cs = ds = qs = 0.0
            while t < Ts:                                                   # :353
                fr = i / 30.0
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
                dist, g, dtau = lookup.query(pos, start + t)                # :363 at the sample's absolute time
                lowered[s] |= bool(getattr(lookup, "lowered", False))
                ex = math.exp(-(dist - p["d0"]) / p["r"])
                cd, gd = p["alpha"] * ex, -(p["alpha"] / p["r"]) * ex       # :509, :514
                cs += p["wc"] * cd * vn * dt                                # :373
                ds += p["wc"] * (gd * float(np.asarray(g) @ pd) * vn * dt + cd * vdot * dt + cd * vn * (1.0 / 30.0))
                moved = p["wc"] * gd * dtau * vn * dt                       # per second of delay of this sample
                ds += moved * (1.0 if mutant == "own_no_i30" else fr)
                qs += moved
                if dyn:                                                     # :383-407, formulas :517-535
                    S = dS = 0.0
                    for k in range(3):
                        cv = p["alpha_v"] * math.exp((abs(vel[k]) - p["v0"]) / p["r_v"])
                        ca = p["alpha_a"] * math.exp((abs(acc[k]) - p["a0"]) / p["r_a"])
                        S += cv + ca
                        dS += cv / p["r_v"] * tt._sgn(vel[k]) * vd[k] + ca / p["r_a"] * tt._sgn(acc[k]) * ad[k]
                    cs += S * vn * dt
                    ds += dS * vn * dt + S * vdot * dt + S * vn * (1.0 / 30.0)
                t += dt
                i += 1
            parts[s, 1], parts[s, 3], parts[s, 4] = cs, ds, qs
        start = start + T[s]
    R = 0.0
    for s in range(m - 1, -1, -1):                                          # from the last segment to the first
        parts[s, 5] = 0.0 if mutant == "no_cross" else (R + parts[s, 4] if mutant == "cross_with_own" else R)
        R += parts[s, 4]
    cost = 0.0
    for s in range(m):
        cost += parts[s, 0] + parts[s, 1]
    return cost + 1e-3, (parts[:, 2] + parts[:, 3]) + parts[:, 5], R, parts, lowered   # :417-418


def gradient_batch(T, Df, x, lookup, p, t0=None):
    """Rows of a batch: T (B, m) or (m,), Df (B, 3, 6), x (B, n), t0 None / scalar / (B,) -> cost (B,), gT (B, m), gt0
    (B,), parts (B, m, 6), lowered (B, m)."""
    B = x.shape[0]
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (B, np.shape(T)[-1]))
    t0 = np.broadcast_to(0.0 if t0 is None else np.asarray(t0, dtype=np.float64), (B,))
    out = [cost_gradT(T[b], Df[b], x[b], lookup, p, t0[b]) for b in range(B)]
    return (np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out]),
            np.stack([o[3] for o in out]), np.stack([o[4] for o in out]))


def optimize_times(T, Df, x, lookup, p, rho, t_min, t_max, first_move, ftol_rel, xtol_abs, max_evals, T_lo=None, t0=0.0,
                   trace=None):
    """time_twin.optimize_times, step for step, with the pass above as its evaluation -> (T_out (m,), info (8,))."""
    T = np.asarray(T, dtype=np.float64)
    m = len(T)
    lo = np.full(m, float(t_min)) if T_lo is None else np.maximum(t_min, np.asarray(T_lo, dtype=np.float64))
    pinned = lo > t_max

    def clamp(v):
        return np.where(pinned, lo, np.minimum(np.maximum(v, lo), t_max))

    def ev(Tv):
        c, gT = cost_gradT(Tv, Df, x, lookup, p, t0)[:2]
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
