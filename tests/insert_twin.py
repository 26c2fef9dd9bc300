"""Waypoint insertion (include/gtop.h: gtop_insert_waypoints_device) restated in numpy, independently of the library:
the rule per row in plain float64 operations, one rounded IEEE operation per step in the order the header writes them
and nothing fused, so that the device kernel (csrc/gtop_insert.hip, compiled unfused) reproduces the bits.

insert_row serves one trajectory; insert_batch loops it.  The static field enters through `lookup`, a function
p (3,) -> (d, g (3,), out): the distance and gradient gtop_edt_query_device returns for (p, -1) and whether p is out of
the map — the oracle's query on the CPU, the device's own on the GPU.

`mutant` switches on ONE deliberate mistake; tests/test_insert_twin.py shows that its checks catch each of them.

The second half is exact: the curve's position, velocity and acceleration at the cut, the Taylor shift of a quintic and
the Hermite coefficients of a segment from its six end conditions, in rational arithmetic (fractions)."""
from fractions import Fraction

import numpy as np

from tests import post_twin as pt

AT_TIME, LONGEST = 0, 1
N_INFO = 6
MUTANTS = ("junction_shift", "times_swapped", "last_on_tie", "no_clamp", "old_axis_stride")
F = np.float64


def walk(T, t):
    """(segment, local time) of trajectory time t: segment_of of csrc/gtop_report_common.h, the last segment extended."""
    idx, m = 0, len(T)
    while idx < m - 1 and T[idx] <= t:
        t = t - T[idx]
        idx += 1
    return idx, t


def longest(T, mutant=None):
    """The first index of the largest time: a later segment replaces the current one only on strict > (mutant
    last_on_tie: on >=)."""
    s = 0
    for i in range(1, len(T)):
        if (T[i] >= T[s]) if mutant == "last_on_tie" else (T[i] > T[s]):
            s = i
    return s


def poly_eval(c, t):
    """poly_eval of csrc/gtop_device_common.h: the dot over descending powers, powers by multiplication."""
    t2 = t * t
    t3 = t2 * t
    t4 = t2 * t2
    t5 = t4 * t
    s = F(0.0)
    s = s + t5 * c[5]
    s = s + t4 * c[4]
    s = s + t3 * c[3]
    s = s + t2 * c[2]
    s = s + t * c[1]
    s = s + c[0]
    return s


def horner_vel(c, t):
    return ((((F(5.0) * c[5]) * t + F(4.0) * c[4]) * t + F(3.0) * c[3]) * t + F(2.0) * c[2]) * t + c[1]


def horner_acc(c, t):
    return (((F(20.0) * c[5]) * t + F(12.0) * c[4]) * t + F(6.0) * c[3]) * t + F(2.0) * c[2]


def grow(old, m, s, fresh, mutant=None):
    """A row of 9 (m - 1) entries (x, lb or ub) -> the row of 9 m: junction k' = 1 .. m of the output is old junction
    k' for k' <= s, the new one (fresh (3 components, 3 axes)) for k' == s + 1, old junction k' - 1 behind it."""
    old = np.asarray(old, dtype=F).reshape(3, 3 * m - 3)
    stride = 3 * m - 3 if mutant == "old_axis_stride" else 3 * m
    flat = np.zeros(9 * m)
    new_at = s + 1
    if mutant == "junction_shift":       # one place too far (one too near at the end of the row)
        new_at = s + 2 if s + 2 <= m else s
    k = np.arange(1, m + 1)
    source = np.where(k < new_at, k, k - 1)[k != new_at] - 1        # the old junction (from 0) behind each copied one
    for axis in range(3):
        block = np.empty((m, 3))
        block[k != new_at] = old[axis].reshape(m - 1, 3)[source]
        block[new_at - 1] = fresh[:, axis]
        flat[axis * stride:axis * stride + 3 * m] = block.reshape(-1)
    return flat


def insert_row(m, x, coeff, T, mode=LONGEST, when=None, min_fraction=0.1, push=0.0, push_below=0.0, bos=3.0, vos=8.0,
               aos=10.0, lb=None, ub=None, lookup=None, mutant=None):
    """One row: dict(x_out (9m,), T_out (m+1,), lb_out, ub_out (9m,) or None, info (6,))."""
    T = np.asarray(T, dtype=F)
    coeff = np.asarray(coeff, dtype=F).reshape(m, 3, 6)
    info = np.zeros(N_INFO)
    at_time = mode == AT_TIME
    if at_time:
        t = F(when)
        if not (t >= 0.0 and t < np.inf):
            at_time = False
            info[2] = 1.0
    if at_time:
        s, tl = walk(T, t)
        Ts = T[s]
    else:
        s = longest(T, mutant)
        Ts = T[s]
        tl = F(0.5) * Ts
    lo = F(min_fraction) * Ts
    hi = Ts - lo
    tc = tl if mutant == "no_clamp" else np.fmin(np.fmax(tl, lo), hi)
    info[3] = 1.0 if tc != tl else 0.0
    tl = tc
    T_out = np.empty(m + 1)
    T_out[:s] = T[:s]
    T_out[s], T_out[s + 1] = (Ts - tl, tl) if mutant == "times_swapped" else (tl, Ts - tl)
    T_out[s + 2:] = T[s + 1:]
    fresh = np.empty((3, 3))             # [p | v | a][axis]
    for k in range(3):
        c = coeff[s, k]
        fresh[0, k], fresh[1, k], fresh[2, k] = poly_eval(c, tl), horner_vel(c, tl), horner_acc(c, tl)
    if push > 0.0:
        d, g, out = lookup(fresh[0].copy())
        g = np.asarray(g, dtype=F)
        n = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        info[4] = d
        if not out and not (d >= push_below) and not (n == 0.0):
            for k in range(3):
                fresh[0, k] = fresh[0, k] + (F(push) * g[k]) / n
            info[5] = 1.0
    info[0], info[1] = s, tl
    res = dict(x_out=grow(x, m, s, fresh, mutant), T_out=T_out, lb_out=None, ub_out=None, info=info)
    if lb is not None:
        p = fresh[0]
        below = np.array([p - F(bos), np.full(3, -F(vos)), np.full(3, -F(aos))])
        above = np.array([p + F(bos), np.full(3, F(vos)), np.full(3, F(aos))])
        res["lb_out"], res["ub_out"] = grow(lb, m, s, below, mutant), grow(ub, m, s, above, mutant)
    return res


def insert_batch(m, x, coeff, T, when=None, lb=None, ub=None, **kw):
    """Rows of a batch: T (B, m) or shared (m,); when, lb, ub per row or None.  -> dict of stacked arrays."""
    B = len(x)
    T = np.asarray(T, dtype=F)
    rows = [insert_row(m, x[i], coeff[i], T[i] if T.ndim == 2 else T, when=None if when is None else when[i],
                       lb=None if lb is None else lb[i], ub=None if ub is None else ub[i], **kw) for i in range(B)]
    return {k: (None if rows[0][k] is None else np.array([r[k] for r in rows])) for k in rows[0]}


# ---- exact arithmetic ----------------------------------------------------------------------------------------------
def exact_pva(c6, t):
    """((p, v, a), (|p|-, |v|-, |a|-magnitudes)) of sum_j c_j t^j at t, exact: the magnitudes are sum |c_j| t^j,
    sum j |c_j| t^(j-1) and sum j (j-1) |c_j| t^(j-2)."""
    c, t = [Fraction(float(v)) for v in c6], Fraction(t)
    val, mag = [], []
    for der in range(3):
        f = [Fraction(1)] * 6
        for j in range(6):
            for i in range(der):
                f[j] *= (j - i)
        val.append(sum(f[j] * c[j] * t ** (j - der) for j in range(der, 6)))
        mag.append(sum(f[j] * abs(c[j]) * abs(t) ** (j - der) for j in range(der, 6)))
    return val, mag


def taylor_shift(c6, t):
    """The coefficients of q(u) = p(t + u), exact."""
    c, t = [Fraction(v) for v in c6], Fraction(t)
    out = []
    for i in range(6):
        acc = Fraction(0)
        for j in range(i, 6):
            binom = Fraction(1)
            for r in range(i):
                binom = binom * (j - r) / (r + 1)
            acc += binom * c[j] * t ** (j - i)
        out.append(acc)
    return out


def hermite_exact(d6, Ts):
    """c = A^-1 d for d = [p0, v0, a0, pT, vT, aT] of Fractions and a Fraction time, exact."""
    inv = pt.invert(pt.hermite_matrix(Fraction(Ts)))
    return [sum(inv[r][k] * Fraction(d6[k]) for k in range(6)) for r in range(6)]


def segment_rows_exact(m, Df, x, T):
    """The coefficient rows {(s, axis): c[6]} of a problem of m segments whose Df (18,), x (9 (m - 1),) and T (m,) are
    Fractions, each formed exactly from its six end conditions: the layout x[i + axis * (3m - 3)] is applied HERE."""
    out = {}
    for axis in range(3):
        def wp(j):
            if j == 0:
                return list(Df[6 * axis:6 * axis + 3])
            if j == m:
                return list(Df[6 * axis + 3:6 * axis + 6])
            at = axis * (3 * m - 3) + 3 * (j - 1)
            return list(x[at:at + 3])
        for s in range(m):
            out[(s, axis)] = hermite_exact(wp(s) + wp(s + 1), T[s])
    return out
