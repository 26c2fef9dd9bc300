"""An exact twin of the set-up and post-processing kernels (gtop_setup.hip: setup_paths_kernel, coefficients_kernel,
eval_trajectories_kernel), for tests/test_post_twin.py (CPU) and tests/test_gpu_post.py (GPU).  Standard library and
numpy only; it neither imports oracle/ nor calls the product.

Two kinds of quantity, kept apart:

  * DECISIONS are replayed in Python float (IEEE double) with the additions of
    include/grad_traj_optimization/polynomial_traj.hpp: time_sum as the serial sum (:37-43), the accumulated
    eval_t += dt while eval_t <= time_sum (:69-78), the segment walk t -= T[idx] while T[idx] <= t (:48-51; the last
    segment is extended where the reference walks off the end) and per segment the number of eval_t < T_s steps
    (:155-167).  A correct implementation performs the same additions, so these are compared with ==.
  * VALUES are computed in exact rational arithmetic from the doubles (Fraction(float) is exact), square roots in
    decimal at SQRT_DIGITS digits.  Beside every value stands its MAGNITUDE: the same expression with absolute values
    and sums for differences (sum |c_i| |t|^i for a point, |A^-1| |d| for a coefficient), the scale a rounding-error
    bound K * u * magnitude is written against.

segment_time / initial_d restate setPath in plain floats: that arithmetic is unfused and sqrt is correctly rounded,
so the comparison with the kernel is bit for bit.

Two MUTATION SWITCHES exist for the sensitivity test only: strict_boundary (the walk compares with <) and
product_times (sample k at k * dt in place of the accumulated time)."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)          # unit roundoff of IEEE double
SQRT_DIGITS = 80
STATS = ("time_sum", "length", "jerk", "mean_v", "max_v", "mean_a", "max_a", "acc_cost", "n_samples")


def _floats(a):
    return [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def fsqrt(q):
    """sqrt of a non-negative Fraction, as a Fraction, to SQRT_DIGITS significant digits."""
    q = Fraction(q)
    if q == 0:
        return Fraction(0)
    with localcontext() as ctx:
        ctx.prec = SQRT_DIGITS
        return Fraction((Decimal(q.numerator) / Decimal(q.denominator)).sqrt())


# ---------------------------------------------------------------------------------------------------------------------
# set-up (src/grad_traj_optimizer.cpp:67-110, src/qp_generator.cpp:199-221, :407-451) in plain floats
# ---------------------------------------------------------------------------------------------------------------------
def segment_time(path, mean_v=1.8, init_time=0.3):
    """(m,) segment times of one waypoint list (m + 1, 3).  `i == segment_time.size()` never holds inside the
    reference's loop (:73-81): only segment 0 gets init_time."""
    p = np.asarray(path, dtype=np.float64)
    m = p.shape[0] - 1
    T = np.empty(m)
    for i in range(m):
        dx, dy, dz = (float(p[i, a]) - float(p[i + 1, a]) for a in range(3))
        ln = math.sqrt(dx * dx + dy * dy + dz * dz)          # math.sqrt is correctly rounded
        T[i] = ln / mean_v + init_time if i == 0 else ln / mean_v
    return T


def initial_d(path):
    """(Df (3, 6), x0 (3, 3m - 3)) of one waypoint list: [p_start, 0, 0, p_end, 0, 0] per axis and the interior
    waypoints' positions with zero velocity / acceleration."""
    p = np.asarray(path, dtype=np.float64)
    m = p.shape[0] - 1
    Df = np.zeros((3, 6))
    x0 = np.zeros((3, 3 * m - 3))
    for a in range(3):
        Df[a, 0], Df[a, 3] = p[0, a], p[m, a]
        for w in range(1, m):
            x0[a, 3 * (w - 1)] = p[w, a]
    return Df, x0


# ---------------------------------------------------------------------------------------------------------------------
# decisions, in float
# ---------------------------------------------------------------------------------------------------------------------
def time_sum(T):
    s = 0.0
    for t in _floats(T):
        s += t
    return s


def sample_times(T, dt, product_times=False):
    """The getTraj sample times: eval_t accumulated by += dt while eval_t <= time_sum."""
    ts, dt = time_sum(T), float(dt)
    out, t, k = [], 0.0, 0
    while t <= ts:
        out.append(t)
        k += 1
        t = k * dt if product_times else t + dt
    return out


def walk(T, t, strict_boundary=False):
    """(segment index, local time) of trajectory time t."""
    T = T if isinstance(T, list) else _floats(T)
    idx, m = 0, len(T)
    while idx < m - 1 and (T[idx] < t if strict_boundary else T[idx] <= t):
        t -= T[idx]
        idx += 1
    return idx, t


def segment_counts(T, dt):
    """Per segment, the number of accumulated eval_t < T_s steps (getMeanAndMaxVel / Acc, :155-167)."""
    out, dt = [], float(dt)
    for Ts in _floats(T):
        c, e = 0, 0.0
        while e < Ts:
            c += 1
            e += dt
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# values, exact
# ---------------------------------------------------------------------------------------------------------------------
def point(c6, t):
    """(value, magnitude) of sum_i c_i t^i, exact."""
    t = Fraction(t)
    v = m = Fraction(0)
    p = Fraction(1)
    for c in c6:
        c = Fraction(c)
        v += c * p
        m += abs(c) * abs(p)
        p *= t
    return v, m


def samples(coeff, T, dt, strict_boundary=False, product_times=False):
    """The getTraj points of one trajectory: dict(n, time_sum, idx[n], tloc[n], pts[n][3], mag[n][3])."""
    T = _floats(T)
    cf = np.asarray(coeff, dtype=np.float64).reshape(len(T), 18)
    times = sample_times(T, dt, product_times)
    idx, tloc, pts, mag = [], [], [], []
    for t in times:
        i, tl = walk(T, t, strict_boundary)
        pv = [point(_floats(cf[i, 6 * a:6 * a + 6]), tl) for a in range(3)]
        idx.append(i)
        tloc.append(tl)
        pts.append([p[0] for p in pv])
        mag.append([p[1] for p in pv])
    return dict(n=len(times), time_sum=time_sum(T), idx=idx, tloc=tloc, pts=pts, mag=mag)


def length(smp):
    """(value, magnitude) of getLength over the points of samples(): sum of point-to-point norms; the magnitude is the
    same sum over the norms of (mag_k + mag_{k-1}) per axis."""
    v = m = Fraction(0)
    for k in range(1, smp["n"]):
        v += fsqrt(sum((smp["pts"][k][a] - smp["pts"][k - 1][a]) ** 2 for a in range(3)))
        m += fsqrt(sum((smp["mag"][k][a] + smp["mag"][k - 1][a]) ** 2 for a in range(3)))
    return v, m


def jerk_matrix(Ts):
    """M(i, j) = i(i-1)(i-2) j(j-1)(j-2) T^(i+j-5) / (i+j-5), i, j = 3..5 (:126-130), exact."""
    Ts = Fraction(Ts)
    return {(i, j): Fraction(i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2), i + j - 5) * Ts ** (i + j - 5)
            for i in range(3, 6) for j in range(3, 6)}


def segment_terms(c18, Ts):
    """One segment's exact terms: dict(jerk, jerk_mag, acc_cost, vn, vn_mag, an, an_mag) — the end-time velocity and
    acceleration norms are the reference's (tv(i) = pow(ts, i): the segment DURATION, :158, :191)."""
    Ts = Fraction(Ts)
    c = [Fraction(float(v)) for v in c18]
    M = jerk_matrix(Ts)
    jk = jm = Fraction(0)
    vel, velm, acc, accm = [], [], [], []
    for a in range(3):
        cc = c[6 * a:6 * a + 6]
        for (i, j), mij in M.items():
            jk += cc[i] * mij * cc[j]
            jm += abs(cc[i]) * abs(mij) * abs(cc[j])
        vel.append(sum(Ts ** i * (i + 1) * cc[i + 1] for i in range(5)))
        velm.append(sum(abs(Ts) ** i * (i + 1) * abs(cc[i + 1]) for i in range(5)))
        acc.append(sum(Ts ** i * (i + 2) * (i + 1) * cc[i + 2] for i in range(4)))
        accm.append(sum(abs(Ts) ** i * (i + 2) * (i + 1) * abs(cc[i + 2]) for i in range(4)))
    ac = sum((2 * c[6 * a + 2]) ** 2 for a in range(3)) * Ts
    return dict(jerk=jk, jerk_mag=jm, acc_cost=ac, vn=fsqrt(sum(v * v for v in vel)),
                vn_mag=fsqrt(sum(v * v for v in velm)), an=fsqrt(sum(v * v for v in acc)),
                an_mag=fsqrt(sum(v * v for v in accm)))


def stats(coeff, T, dt, smp=None, strict_boundary=False, product_times=False):
    """(value[9], magnitude[9], info) of one trajectory, in the order of STATS.  time_sum and n_samples are decisions
    (floats, magnitude 0); the rest are Fractions.  info: counts per segment, the segments holding the maxima."""
    Tl = _floats(T)
    cf = np.asarray(coeff, dtype=np.float64).reshape(len(Tl), 18)
    if smp is None:
        smp = samples(cf, Tl, dt, strict_boundary, product_times)
    ln, ln_mag = length(smp)
    cnt = segment_counts(Tl, dt)
    num = sum(cnt)
    seg = [segment_terms(cf[s], Tl[s]) for s in range(len(Tl))]
    jerk, jerk_mag = sum(g["jerk"] for g in seg), sum(g["jerk_mag"] for g in seg)
    acc_cost = sum(g["acc_cost"] for g in seg)
    counted = [s for s in range(len(Tl)) if cnt[s] > 0]
    arg_v = max(counted, key=lambda s: seg[s]["vn"]) if counted else -1
    arg_a = max(counted, key=lambda s: seg[s]["an"]) if counted else -1
    if num:
        mean_v = sum(cnt[s] * seg[s]["vn"] for s in counted) / num
        mean_v_mag = sum(cnt[s] * seg[s]["vn_mag"] for s in counted) / num
        mean_a = sum(cnt[s] * seg[s]["an"] for s in counted) / num
        mean_a_mag = sum(cnt[s] * seg[s]["an_mag"] for s in counted) / num
        max_v, max_a = seg[arg_v]["vn"], seg[arg_a]["an"]
        max_v_mag = max(seg[s]["vn_mag"] for s in counted)
        max_a_mag = max(seg[s]["an_mag"] for s in counted)
    else:   # no counted sample: 0 / 0 and the -1 the maxima start from
        mean_v = mean_a = None
        mean_v_mag = mean_a_mag = max_v_mag = max_a_mag = Fraction(0)
        max_v = max_a = Fraction(-1)
    val = [smp["time_sum"], ln, jerk, mean_v, max_v, mean_a, max_a, acc_cost, float(smp["n"])]
    mag = [0, ln_mag, jerk_mag, mean_v_mag, max_v_mag, mean_a_mag, max_a_mag, acc_cost, 0]
    return val, mag, dict(counts=cnt, num=num, arg_v=arg_v, arg_a=arg_a, seg=seg)


# ---------------------------------------------------------------------------------------------------------------------
# coefficients: the 6 x 6 Hermite system from its definition, rational elimination
# ---------------------------------------------------------------------------------------------------------------------
def hermite_matrix(Ts):
    """Rows p(0), p'(0), p''(0), p(T), p'(T), p''(T) of p(t) = sum_j c_j t^j, exact."""
    Ts = Fraction(Ts)
    A = [[Fraction(0)] * 6 for _ in range(6)]
    for der in range(3):
        for j in range(der, 6):
            f = Fraction(math.factorial(j), math.factorial(j - der))
            A[der][j] = f if j == der else Fraction(0)          # t = 0: only the t^0 term of the derivative
            A[3 + der][j] = f * Ts ** (j - der)
    return A


def invert(A):
    """Inverse of a small rational matrix by Gauss-Jordan elimination with exact pivots."""
    n = len(A)
    W = [list(map(Fraction, A[r])) + [Fraction(int(r == c)) for c in range(n)] for r in range(n)]
    for col in range(n):
        piv = next(r for r in range(col, n) if W[r][col] != 0)
        W[col], W[piv] = W[piv], W[col]
        d = W[col][col]
        W[col] = [v / d for v in W[col]]
        for r in range(n):
            if r != col and W[r][col] != 0:
                f = W[r][col]
                W[r] = [v - f * w for v, w in zip(W[r], W[col])]
    return [row[n:] for row in W]


_HERMITE_INV = {}


def hermite_inverse(Ts):
    """A^-1 of a segment time, solved once per time; row by row as (common denominator D, [(column, integer n)]) of
    its non-zeros n / D — integer arithmetic keeps the many solves of a large batch cheap."""
    Ts = float(Ts)
    if Ts not in _HERMITE_INV:
        rows = []
        for row in invert(hermite_matrix(Ts)):
            D = math.lcm(*(v.denominator for v in row))
            rows.append((D, [(k, int(v * D)) for k, v in enumerate(row) if v != 0]))
        _HERMITE_INV[Ts] = rows
    return _HERMITE_INV[Ts]


def hermite_coefficients(d6, Ts):
    """(c[6], mag[6]): c = A^-1 d for d = [p0, v0, a0, pT, vT, aT], mag = |A^-1| |d| entrywise."""
    ratios = [float(v).as_integer_ratio() for v in d6]           # doubles: the denominators are powers of two
    E = max(den for _, den in ratios)
    d = [num * (E // den) for num, den in ratios]
    c, mag = [], []
    for D, row in hermite_inverse(Ts):
        c.append(Fraction(sum(n * d[k] for k, n in row), D * E))
        mag.append(Fraction(sum(abs(n * d[k]) for k, n in row), D * E))
    return c, mag


def derivatives(m, Df, x):
    """d(s, axis) -> [p0, v0, a0, pT, vT, aT] of a segment as floats: Df (3, 6) = [start p v a | end p v a] per axis
    and the free variables x laid out axis-major, (p, v, a) per interior waypoint
    (src/grad_traj_optimizer.cpp:182-187)."""
    Dfl = np.asarray(Df, dtype=np.float64).reshape(3, 6).tolist()
    xl = np.asarray(x, dtype=np.float64).reshape(3, 3 * m - 3).tolist()

    def wp(j, a):   # (p, v, a) of waypoint j: the boundary ones from Df, the interior ones from x
        return Dfl[a][0:3] if j == 0 else Dfl[a][3:6] if j == m else xl[a][3 * (j - 1):3 * j]
    return lambda s, a: wp(s, a) + wp(s + 1, a)


def coefficients(T, Df, x, only=None):
    """{(s, axis): (c[6], mag[6])} of one trajectory (getCoefficientFromDerivative, :253-279), for every (segment,
    axis) or those listed in `only`."""
    Tl = _floats(T)
    m = len(Tl)
    keys = only if only is not None else [(s, a) for s in range(m) for a in range(3)]
    d = derivatives(m, Df, x)
    return {(s, a): hermite_coefficients(d(s, a), Tl[s]) for (s, a) in keys}


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def ratio(got, exact, mag):
    """|got - exact| / (u * mag) as a float: what K bounds.  got is a double; a zero magnitude admits no error."""
    err = abs(Fraction(float(got)) - Fraction(exact))
    if err == 0:
        return 0.0
    if mag == 0:
        return math.inf
    return float(err / (U * Fraction(mag)))
