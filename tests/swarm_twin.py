"""The twin of include/gtop_swarm.h: the swarm separation cost and its gradient, operation by operation, generic over
the number type.  With FLOAT every product, quotient and sum below is one numpy float64 operation (one rounding each),
in the order the header writes them — so the device's outputs are these bits.  With EXACT the same lines run on
fractions.Fraction: only + - * / and comparisons occur, so that run is exact.

Arrays are numpy arrays of float64 or of Fractions (dtype object); rows are vectorised, the sums whose order the header
fixes (partners j, samples k, powers n) are Python loops.

`mag=True` returns the rounding-error MAGNITUDES of the same figures: the same decisions (flown, segment, active) taken
from the true values, then every input by its absolute value, additions for subtractions.

A `mutant` names one deliberate mistake (tests/test_swarm_twin.py kills each of them):
  "inclusive"      active iff e >= 0
  "self_pair"      j == i is not left out
  "junction"       a waypoint takes the END part of the segment behind it and the START part of the one before
  "wrong_D"        d c4 / d v0 = 7 / T^3 in place of 8 / T^3
  "no_dt"          dt left out of S and of the gradient"""
from fractions import Fraction

import numpy as np

MUTANTS = ("inclusive", "self_pair", "junction", "wrong_D", "no_dt")


class FLOAT:
    @staticmethod
    def num(v):
        return np.float64(v)

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape)


class EXACT:
    @staticmethod
    def num(v):
        return v if isinstance(v, Fraction) else Fraction(float(v))

    @staticmethod
    def arr(a):
        a = np.asarray(a, dtype=object)
        out = np.empty(a.shape, dtype=object)
        for i, v in np.ndenumerate(a):
            out[i] = EXACT.num(v)
        return out

    @staticmethod
    def zeros(shape):
        out = np.empty(shape, dtype=object)
        out.fill(Fraction(0))
        return out


def _b(x):
    return np.asarray(x, dtype=bool)


def start_times(t0, B, N):
    """The rules of gtop_set_start_times: None -> 0, one value -> shared, else one per row."""
    if t0 is None:
        return N.zeros((B,))
    t0 = N.arr(np.atleast_1d(np.asarray(t0, dtype=object)).reshape(-1))
    if t0.shape[0] == 1:
        return N.arr([t0[0]] * B)
    assert t0.shape[0] == B, "a start-time count that is not 0, 1 or B"
    return t0


def sample_rows(coeff, T, t0, t_lo, dt, n, hold_ends, N=FLOAT):
    """(pos (B, n, 3), flown (B, n) bool, u (B, n), seg (B, n) int) of rows coeff (B, m, 18), T (B, m) or (m,): the
    grid, the flown samples, the segment walk and the positions of include/gtop_separation.h.  A sample at which a row is
    not flown has position 0 here (the device stores NaN; both are left out by `flown`)."""
    coeff = N.arr(coeff)
    B, m = coeff.shape[:2]
    T = np.broadcast_to(N.arr(T), (B, m))
    start = start_times(t0, B, N)
    tau = N.num(t_lo) + N.arr(list(range(n))) * N.num(dt)                  # the product rounded, then the sum
    zero = N.num(0)
    pos, uu = N.zeros((B, n, 3)), N.zeros((B, n))
    flown, seg = np.zeros((B, n), dtype=bool), np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        time_sum = zero
        for s in range(m):
            time_sum = time_sum + T[b, s]
        u = tau - start[b]
        fl = _b(u >= zero) & _b(u <= time_sum)
        if hold_ends:
            u = np.where(_b(u < zero), zero, np.where(_b(u > time_sum), time_sum, u))
            fl = np.ones(n, dtype=bool)
        idx = np.zeros(n, dtype=np.int64)
        t = u.copy()
        for s in range(m - 1):                                             # while s < m - 1 and T_s <= t: t -= T_s, ++s
            go = (idx == s) & _b(T[b, s] <= t)
            t = np.where(go, t - T[b, s], t)
            idx = idx + go
        c = coeff[b, idx].reshape(n, 3, 6)
        tt = t[:, None]
        t2 = tt * tt
        t3 = t2 * tt
        t4 = t2 * t2
        t5 = t4 * tt
        p = zero + t5 * c[..., 5]
        p = p + t4 * c[..., 4]
        p = p + t3 * c[..., 3]
        p = p + t2 * c[..., 2]
        p = p + tt * c[..., 1]
        p = p + c[..., 0]
        pos[b] = np.where(fl[:, None], p, zero)
        uu[b] = np.where(fl, t, zero)
        flown[b], seg[b] = fl, idx
    return pos, flown, uu, seg


def swarm_terms(coeff, T, t0, t_lo, dt, n, hold_ends, w, radius, frozen=None, N=FLOAT, mutant=None, mag=False,
                want_grad=True):
    """(S (B,), grad (B, 9 (m - 1)), active (B,) int, least |e| over the tested terms) of the rows coeff against
    themselves (frozen None) or against the rows `frozen` (B, m, 18), as include/gtop_swarm.h states them."""
    coeff = N.arr(coeff)
    B, m = coeff.shape[:2]
    Tb = np.broadcast_to(N.arr(T), (B, m))
    zero = N.num(0)
    pos, flown, u, seg = sample_rows(coeff, T, t0, t_lo, dt, n, hold_ends, N)
    if frozen is None:
        posj, flownj = pos, flown
    else:
        posj, flownj = sample_rows(frozen, T, t0, t_lo, dt, n, hold_ends, N)[:2]
    if mag:
        pm = sample_rows(np.abs(coeff), T, t0, t_lo, dt, n, hold_ends, N)[0]
        pmj = pm if frozen is None else sample_rows(np.abs(N.arr(frozen)), T, t0, t_lo, dt, n, hold_ends, N)[0]
    R2 = N.num(radius) * N.num(radius)
    C, F = N.zeros((B, n)), N.zeros((B, n, 3))
    active = np.zeros(B, dtype=np.int64)
    rows = np.arange(B)
    least = None
    for j in range(B):                                                     # the partners, ascending
        d = pos - posj[j][None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        e = R2 - d2
        both = flown & flownj[j][None]
        if mutant != "self_pair":
            both = both & (rows != j)[:, None]
        act = both & (_b(e >= zero) if mutant == "inclusive" else _b(e > zero))
        if both.any():
            near = np.abs(e[both]).min()
            least = near if least is None or near < least else least
        if mag:
            d = pm + pmj[j][None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            e = R2 + d2
        ea = np.where(act, e, zero)
        e2 = ea * ea
        C = C + e2 * ea
        F = F + e2[..., None] * np.where(act[..., None], d, zero)
        active += act.sum(axis=1)
    wdt = N.num(w) if mutant == "no_dt" else N.num(w) * N.num(dt)
    total = N.zeros((B,))
    for k in range(n):                                                     # the samples, ascending
        total = total + C[:, k]
    S = wdt * total
    if not want_grad:
        return S, None, active, least
    # the moments of the forces per segment and axis
    G = N.zeros((B, m, 3, 6))
    u2 = u * u
    u3 = u2 * u
    u4 = u2 * u2
    u5 = u4 * u
    powers = (None, u, u2, u3, u4, u5)
    for k in range(n):
        fl, s = flown[:, k], seg[:, k]
        for a in range(3):
            for p in range(6):
                term = F[:, k, a] if p == 0 else F[:, k, a] * powers[p][:, k]
                G[rows, s, a, p] = G[rows, s, a, p] + np.where(fl, term, zero)
    Ts = Tb[:, :, None]                                                    # (B, m, 1) against G (B, m, 3)
    T2 = Ts * Ts
    T3 = T2 * Ts
    T4 = T2 * T2
    T5 = T4 * Ts
    G0, G1, G2, G3, G4, G5 = (G[..., p] for p in range(6))

    def q(v):
        return N.num(abs(v) if mag else v)
    c4v0 = 7.0 if mutant == "wrong_D" else 8.0
    h0 = [(((G0 + (q(-10.0) / T3) * G3) + (q(15.0) / T4) * G4) + (q(-6.0) / T5) * G5),
          (((G1 + (q(-6.0) / T2) * G3) + (q(c4v0) / T3) * G4) + (q(-3.0) / T4) * G5),
          (((q(0.5) * G2 + (q(-1.5) / Ts) * G3) + (q(1.5) / T2) * G4) + (q(-0.5) / T3) * G5)]
    hT = [(((q(10.0) / T3) * G3 + (q(-15.0) / T4) * G4) + (q(6.0) / T5) * G5),
          (((q(-4.0) / T2) * G3 + (q(7.0) / T3) * G4) + (q(-3.0) / T4) * G5),
          (((q(0.5) / Ts) * G3 + (q(-1.0) / T2) * G4) + (q(0.5) / T3) * G5)]
    K = q(-6.0) * N.num(w)
    if mutant != "no_dt":
        K = K * N.num(dt)
    ndp = 3 * m - 3
    grad = N.zeros((B, 3 * ndp))
    for j in range(1, m):
        for c in range(3):
            for a in range(3):
                if mutant == "junction":
                    v = K * hT[c][:, j, a] + K * h0[c][:, j - 1, a]
                else:
                    v = K * hT[c][:, j - 1, a] + K * h0[c][:, j, a]
                grad[:, 3 * (j - 1) + c + a * ndp] = v
    return S, grad, active, least


def coefficients(x, Df, T, N=FLOAT):
    """coeff (B, m, 18) of free variables x (B, 9 (m - 1)), Df (B, 18) and T (B, m) or (m,) by the closed form
    include/gtop_time.h states: P, V, A, N3 .. N5.  (In FLOAT the roundings are this function's own: the device's
    coefficients come from gtop_coefficients_device.)"""
    x, Df = N.arr(x), N.arr(Df).reshape(len(x), 3, 6)
    B = x.shape[0]
    m = x.shape[1] // 9 + 1
    ndp = 3 * m - 3
    T = np.broadcast_to(N.arr(T), (B, m))
    coeff = N.zeros((B, m, 18))
    half = N.num(0.5)
    for b in range(B):
        for a in range(3):
            way = [Df[b, a, 0:3]] + [x[b, a * ndp + 3 * j:a * ndp + 3 * j + 3] for j in range(m - 1)] + [Df[b, a, 3:6]]
            for s in range(m):
                (p0, v0, a0), (pT, vT, aT), t = way[s], way[s + 1], T[b, s]
                P = pT - p0 - v0 * t - a0 * t * t * half
                V = (vT - v0 - a0 * t) * t
                A = (aT - a0) * t * t
                t3 = t * t * t
                coeff[b, s, 6 * a:6 * a + 6] = [p0, v0, a0 * half, (10 * P - 4 * V + A * half) / t3,
                                                (7 * V - 15 * P - A) / (t3 * t), (6 * P - 3 * V + A * half) / (t3 * t * t)]
    return coeff


D_TABLE = {   # d c_n / d q as (constant, power of T in the denominator), n = 0 .. 5 (include/gtop_swarm.h)
    "p0": ((1, 0), (0, 0), (0, 0), (-10, 3), (15, 4), (-6, 5)),
    "v0": ((0, 0), (1, 0), (0, 0), (-6, 2), (8, 3), (-3, 4)),
    "a0": ((0, 0), (0, 0), (Fraction(1, 2), 0), (Fraction(-3, 2), 1), (Fraction(3, 2), 2), (Fraction(-1, 2), 3)),
    "pT": ((0, 0), (0, 0), (0, 0), (10, 3), (-15, 4), (6, 5)),
    "vT": ((0, 0), (0, 0), (0, 0), (-4, 2), (7, 3), (-3, 4)),
    "aT": ((0, 0), (0, 0), (0, 0), (Fraction(1, 2), 1), (-1, 2), (Fraction(1, 2), 3)),
}


# ---- inputs ----
def crossing_rows(B, m, seed, spread=1.0, shared_T=False, dyadic=False):
    """(x (B, 9 (m - 1)), Df (B, 18), T (B, m) or (m,)): B robots that cross a ball of radius `spread` around the origin
    on straight lines with random lateral offsets, velocities and accelerations at the waypoints random — so many pairs
    come close.  dyadic: every number a multiple of 2^-6 (exact in both number types, and exact sample times)."""
    rng = np.random.default_rng(seed)

    def r(v):
        return np.round(v * 64.0) / 64.0 if dyadic else v
    ndp = 3 * m - 3
    x, Df = np.zeros((B, 3 * ndp)), np.zeros((B, 3, 6))
    T = r(rng.uniform(0.5, 1.0, (m,) if shared_T else (B, m)))
    for b in range(B):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        off = rng.uniform(-0.3, 0.3, 3) * spread
        a, e = r(-2.0 * spread * d + off), r(2.0 * spread * d + off)
        Df[b, :, 0], Df[b, :, 3] = a, e
        for j in range(1, m):
            p = a + (e - a) * (j / m) + rng.uniform(-0.2, 0.2, 3) * spread
            for ax in range(3):
                x[b, ax * ndp + 3 * (j - 1):ax * ndp + 3 * j] = r(np.array([p[ax], rng.uniform(-1, 1), rng.uniform(-1, 1)]))
    return x, Df.reshape(B, 18), T
