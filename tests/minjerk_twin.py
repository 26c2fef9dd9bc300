"""An exact twin of the minimum-jerk start point (csrc/gtop_minjerk.hip, gtop_min_jerk_start of include/gtop.h), for
tests/test_minjerk_twin.py (CPU) and tests/test_gpu_minjerk.py (GPU).  Standard library and numpy only; it neither
imports oracle/ nor calls the product.

With the waypoint positions fixed, the interior (v_k, a_k), k = 1 .. m-1, minimise sum over the axes of d' R d.  Per
axis the stationarity condition is K u + c = 0: K the block tridiagonal matrix of include/gtop.h (blocks D_k, U_k),
u = (v_1, a_1, ..., v_{m-1}, a_{m-1}) and c = g plus the boundary pairs' terms.  Everything here is exact rational
arithmetic on the doubles taken as rationals (Fraction(float) is exact):

  * segment_matrix(T): M(T) from the table M(1); segment_matrix_derived(T): the same from its definition
    (A^-T Q A^-1 with tests/post_twin.py's hermite_matrix, invert and jerk_matrix), which the CPU test holds equal;
  * rows(T, Df_axis, p_axis): every unknown row as its list of (column, K_ij) and its KNOWN terms, each known term with
    the magnitude the value criterion counts for it — a position term on the exact waypoint difference, e.g.
    360 |p_{k-1} - p_k| / Ta^4, so absolute coordinates do not loosen the bound;
  * ratios(T, Df, x_in, x_out): |r_i| / (u * mag_i) of every unknown row and axis of one trajectory, r = K u + c at the
    doubles x_out holds, mag_i = sum_j |K_ij u_j| + the known terms' magnitudes.  The VALUE CRITERION is
    ratio <= BOUND_K = 2^12, this project's entrywise standard (tests/test_gpu_entrywise.py);
  * solve(T, Df, x_in): the exact minimiser, by rational block elimination.

eliminate(T, Df, x_in, mutant=None) is a plain fp64 restatement of the kernel's elimination (numpy over the three
axes), with MUTATION SWITCHES for the sensitivity test only.  cases() lists the inputs the GPU test uses, so the CPU
test can show that a correct fp64 elimination meets the criterion on every one of them."""
import functools
from fractions import Fraction

import numpy as np

from tests import post_twin

U = post_twin.U
BOUND_K = 2 ** 12

M1 = ((720, -720, 360, 360, 60, -60),
      (-720, 720, -360, -360, -60, 60),
      (360, -360, 192, 168, 36, -24),
      (360, -360, 168, 192, 24, -36),
      (60, -60, 36, 24, 9, -3),
      (-60, 60, -24, -36, -3, 9))
ORDER = (0, 0, 1, 1, 2, 2)      # derivative order of [p(0), p(T), v(0), v(T), a(0), a(T)]


def segment_matrix(T):
    """M(T) as Fractions, rows / columns [p(0), p(T), v(0), v(T), a(0), a(T)]."""
    it = 1 / Fraction(T)
    return [[M1[i][j] * it ** (5 - ORDER[i] - ORDER[j]) for j in range(6)] for i in range(6)]


def segment_matrix_derived(T):
    """The same from the definition: d = A c (post_twin.hermite_matrix, rows p, v, a at 0 then at T), the jerk
    integral c' Q c (post_twin.jerk_matrix), so M = A^-T Q A^-1 in the twin's order of d."""
    Ai = post_twin.invert(post_twin.hermite_matrix(T))
    Q = post_twin.jerk_matrix(T)
    perm = (0, 3, 1, 4, 2, 5)   # [p(0), p(T), v(0), v(T), a(0), a(T)] in hermite_matrix's rows
    return [[sum(Ai[i][perm[r]] * q * Ai[j][perm[c]] for (i, j), q in Q.items()) for c in range(6)] for r in range(6)]


def _inv_powers(T):
    out = []
    for t in T:
        i1 = 1 / Fraction(float(t))
        out.append((None, i1, i1 * i1, i1 ** 3, i1 ** 4))
    return out


def rows(T, Df_axis, p_axis):
    """The 2 (m - 1) unknown rows of one axis.  T (m,), Df_axis [p0, v0, a0, pm, vm, am], p_axis the m - 1 interior
    positions.  Row 2 (k - 1) + c (c = 0: v_k, 1: a_k) is (entries, known): entries [(column, K_ij)], known
    [(value, magnitude)]."""
    T = [float(t) for t in T]
    m = len(T)
    ip = _inv_powers(T)
    df = [Fraction(float(v)) for v in Df_axis]
    p = [df[0]] + [Fraction(float(v)) for v in p_axis] + [df[3]]
    assert len(p) == m + 1
    out = []
    for k in range(1, m):
        a, b = ip[k - 1], ip[k]
        da, db = p[k - 1] - p[k], p[k] - p[k + 1]
        # (coefficient of v_{k-1}, a_{k-1}), (v_k, a_k), (v_{k+1}, a_{k+1}) and the position terms, per row
        prev = ((168 * a[3], 24 * a[2]), (-24 * a[2], -3 * a[1]))                    # U_{k-1}'
        diag = ((192 * a[3] + 192 * b[3], 36 * b[2] - 36 * a[2]), (36 * b[2] - 36 * a[2], 9 * a[1] + 9 * b[1]))
        nxt = ((168 * b[3], -24 * b[2]), (24 * b[2], -3 * b[1]))                     # U_k
        pos = ((360 * a[4] * da, 360 * b[4] * db), (-60 * a[3] * da, 60 * b[3] * db))
        for c in range(2):
            entries, known = [], [(v, abs(v)) for v in pos[c]]
            for (blk, wp, pair) in ((prev[c], k - 1, df[1:3]), (diag[c], k, None), (nxt[c], k + 1, df[4:6])):
                if 1 <= wp <= m - 1:
                    entries += [(2 * (wp - 1), blk[0]), (2 * (wp - 1) + 1, blk[1])]
                else:   # a boundary pair: known
                    known += [(blk[0] * pair[0], abs(blk[0] * pair[0])), (blk[1] * pair[1], abs(blk[1] * pair[1]))]
            out.append((entries, known))
    return out


def dense(T):
    """K as a dense list of lists of Fractions, 2 (m - 1) square."""
    m = len(T)
    K = [[Fraction(0)] * (2 * m - 2) for _ in range(2 * m - 2)]
    for i, (entries, _) in enumerate(rows(T, [0] * 6, [0] * (m - 1))):
        for j, v in entries:
            K[i][j] = v
    return K


def known_vector(T, Df_axis, p_axis):
    """c of K u + c = 0: the position terms g and the boundary pairs' terms, per unknown row."""
    return [sum(v for v, _ in known) for _, known in rows(T, Df_axis, p_axis)]


def split(m, x):
    """(positions (3, m - 1), u (3, 2 (m - 1))) of free variables x (9 (m - 1),) in the layout x[i + axis (3m - 3)],
    i = 3 (k - 1) + {0: p, 1: v, 2: a}."""
    x3 = np.asarray(x, dtype=np.float64).reshape(3, m - 1, 3)
    return x3[:, :, 0].copy(), x3[:, :, 1:].reshape(3, 2 * (m - 1)).copy()


def join(pos, u):
    m1 = pos.shape[1]
    x3 = np.empty((3, m1, 3))
    x3[:, :, 0] = pos
    x3[:, :, 1:] = np.asarray(u, dtype=np.float64).reshape(3, m1, 2)
    return x3.reshape(-1)


def ratios(T, Df, x_in, x_out):
    """(3, 2 (m - 1)) floats: |r_i| / (u mag_i) per axis and unknown row (0 where the residual is exactly 0, inf for a
    non-zero residual on a zero magnitude)."""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    m = T.shape[0]
    pos, _ = split(m, x_in)
    _, u_out = split(m, x_out)
    Df = np.asarray(Df, dtype=np.float64).reshape(3, 6)
    out = np.zeros((3, 2 * (m - 1)))
    for a in range(3):
        u = [Fraction(float(v)) for v in u_out[a]]
        for i, (entries, known) in enumerate(rows(T, Df[a], pos[a])):
            terms = [kij * u[j] for j, kij in entries]
            r = sum(terms) + sum(v for v, _ in known)
            mag = sum(abs(t) for t in terms) + sum(mg for _, mg in known)
            out[a, i] = 0.0 if r == 0 else (float("inf") if mag == 0 else float(abs(r) / (U * mag)))
    return out


@functools.lru_cache(maxsize=None)
def _worst_ratio_cached(T, Df, x_in, x_out, m):
    f = lambda b: np.frombuffer(b, dtype=np.float64)
    return float(np.max(ratios(f(T), f(Df), f(x_in), f(x_out))))


def worst_ratio(T, Df, x_in, x_out):
    """max of ratios(); cached on the bits of its arguments (rows of a batch that repeat another row's inputs and
    outputs cost nothing)."""
    c = lambda v: np.ascontiguousarray(v, dtype=np.float64).tobytes()
    return _worst_ratio_cached(c(T), c(Df), c(x_in), c(x_out), len(np.reshape(T, -1)))


def solve(T, Df, x_in):
    """The exact minimiser: u (3 lists of 2 (m - 1) Fractions), by block elimination in rationals."""
    T = [float(t) for t in np.reshape(T, -1)]
    m = len(T)
    pos, _ = split(m, x_in)
    Df = np.asarray(Df, dtype=np.float64).reshape(3, 6)
    K = dense(T)
    n = 2 * (m - 1)
    out = []
    for a in range(3):
        A = [K[i][:] + [-c] for i, c in enumerate(known_vector(T, Df[a], pos[a]))]
        for col in range(n):          # K is positive definite: no pivoting; the band keeps this O(m)
            d = A[col][col]
            for r in range(col + 1, min(col + 4, n)):
                if A[r][col] != 0:
                    f = A[r][col] / d
                    for cc in list(range(col, min(col + 4, n))) + [n]:
                        A[r][cc] -= f * A[col][cc]
        u = [Fraction(0)] * n
        for r in range(n - 1, -1, -1):
            u[r] = (A[r][n] - sum(A[r][cc] * u[cc] for cc in range(r + 1, min(r + 4, n)))) / A[r][r]
        out.append(u)
    return out


MUTANTS = ("u168", "sign24", "swap_g", "drop_end", "drop_start")


def eliminate(T, Df, x_in, mutant=None):
    """The kernel's block elimination in plain fp64, the three axes as numpy vectors: x_out (9 (m - 1),).
    mutant: None, or one of MUTANTS — 168 -> 192 in U, the sign of -24, Ta and Tb swapped in g, the end pair dropped
    from the last right-hand side, the start pair dropped from the first."""
    assert mutant is None or mutant in MUTANTS
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    m = T.shape[0]
    pos, _ = split(m, x_in)
    Df = np.asarray(Df, dtype=np.float64).reshape(3, 6)
    p = np.concatenate([Df[:, 0:1], pos, Df[:, 3:4]], axis=1)      # (3, m + 1)
    c168 = 192.0 if mutant == "u168" else 168.0
    c24 = 24.0 if mutant == "sign24" else -24.0

    def ublock(i1):
        return c168 * i1 ** 3, c24 * i1 * i1, 24.0 * i1 * i1, -3.0 * i1

    yv = np.zeros(3) if mutant == "drop_start" else Df[:, 1].copy()
    ya = np.zeros(3) if mutant == "drop_start" else Df[:, 2].copy()
    j11 = j12 = j22 = 0.0
    J, Y = [None] * m, [None] * m
    for k in range(1, m):
        ia, ib = 1.0 / T[k - 1], 1.0 / T[k]
        a11, a12, a21, a22 = ublock(ia)
        b11, b12, b21, b22 = ublock(ib)
        w11, w12 = j11 * a11 + j12 * a21, j11 * a12 + j12 * a22
        w21, w22 = j12 * a11 + j22 * a21, j12 * a12 + j22 * a22
        s11 = (192.0 * ia ** 3 + 192.0 * ib ** 3) - (a11 * w11 + a21 * w21)
        s12 = (36.0 * ib * ib - 36.0 * ia * ia) - (a11 * w12 + a21 * w22)
        s22 = (9.0 * ia + 9.0 * ib) - (a12 * w12 + a22 * w22)
        idet = 1.0 / (s11 * s22 - s12 * s12)
        j11, j12, j22 = s22 * idet, -s12 * idet, s11 * idet
        da, db = p[:, k - 1] - p[:, k], p[:, k] - p[:, k + 1]
        ga, gb = (ib, ia) if mutant == "swap_g" else (ia, ib)
        rv = -(360.0 * da * ga ** 4 + 360.0 * db * gb ** 4) - (a11 * yv + a21 * ya)
        ra = -(60.0 * db * gb ** 3 - 60.0 * da * ga ** 3) - (a12 * yv + a22 * ya)
        if k == m - 1 and mutant != "drop_end":
            rv = rv - (b11 * Df[:, 4] + b12 * Df[:, 5])
            ra = ra - (b21 * Df[:, 4] + b22 * Df[:, 5])
        yv, ya = j11 * rv + j12 * ra, j12 * rv + j22 * ra
        J[k], Y[k] = (j11, j12, j22), (yv, ya)
    u = np.zeros((3, m - 1, 2))
    uv, ua = Y[m - 1]
    u[:, m - 2, 0], u[:, m - 2, 1] = uv, ua
    for k in range(m - 2, 0, -1):
        b11, b12, b21, b22 = ublock(1.0 / T[k])
        k11, k12, k22 = J[k]
        tv, ta = b11 * uv + b12 * ua, b21 * uv + b22 * ua
        uv, ua = Y[k][0] - (k11 * tv + k12 * ta), Y[k][1] - (k12 * tv + k22 * ta)
        u[:, k - 1, 0], u[:, k - 1, 1] = uv, ua
    return join(pos, u.reshape(3, -1))


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
# 43 | 44, 86 | 87 and 171 | 172 are where the launch plan (csrc/gtop_minjerk_plan.h) halves its lanes per workgroup
SEGMENTS = (2, 3, 6, 7, 13, 43, 44, 64, 86, 87, 171, 172, 227)
BATCHES = (1, 3, 65, 130)
BASE_ROWS = 4
T_RANGES = {"narrow": (0.3, 3.0), "wide": (0.05, 8.0)}


def base_rows(m, t_range, shared):
    """The four distinct rows every batch of a case is made of (row b of a batch = base row b mod 4): T (4, m) — one
    vector repeated when `shared` —, Df (4, 18) with non-zero velocity and acceleration at both ends, x (4, 9 (m - 1))
    with random positions and, in the v, a entries, junk the call must overwrite."""
    lo, hi = T_RANGES[t_range]
    rng = np.random.default_rng([m, int(shared), int(t_range == "wide")])
    T = rng.uniform(lo, hi, size=(1 if shared else BASE_ROWS, m))
    T = np.repeat(T, BASE_ROWS, axis=0) if shared else T
    steps = rng.normal(0.0, 1.5, size=(BASE_ROWS, 3, m + 1))
    way = np.cumsum(steps, axis=2) + rng.uniform(-20.0, 20.0, size=(BASE_ROWS, 3, 1))
    Df = np.zeros((BASE_ROWS, 3, 6))
    Df[:, :, 0], Df[:, :, 3] = way[:, :, 0], way[:, :, m]
    Df[:, :, (1, 4)] = rng.uniform(-3.0, 3.0, size=(BASE_ROWS, 3, 2))
    Df[:, :, (2, 5)] = rng.uniform(-4.0, 4.0, size=(BASE_ROWS, 3, 2))
    x = rng.uniform(-7.0, 7.0, size=(BASE_ROWS, 3, m - 1, 3))
    x[:, :, :, 0] = way[:, :, 1:m]
    return T, Df.reshape(BASE_ROWS, 18), x.reshape(BASE_ROWS, 9 * (m - 1))


def cases():
    """(m, t_range, shared) of every GPU case."""
    return [(m, r, s) for m in SEGMENTS for r in ("narrow", "wide") for s in (False, True)]


def analytic(m):
    """Collinear waypoints 1.5 apart along x, every T = 0.5, boundary velocity 3 along x, boundary acceleration 0:
    constant velocity has zero jerk, so the unique minimiser is v_k = (3, 0, 0), a_k = 0.  Returns T (m,), Df (18,),
    x_in (n,) with junk in v, a, and the expected x (n,)."""
    T = np.full(m, 0.5)
    Df = np.zeros((3, 6))
    Df[0] = [-2.0, 3.0, 0.0, -2.0 + 1.5 * m, 3.0, 0.0]
    Df[1, 0] = Df[1, 3] = 2.0
    Df[2, 0] = Df[2, 3] = -1.0
    pos = np.empty((3, m - 1))
    pos[0] = -2.0 + 1.5 * np.arange(1, m)
    pos[1], pos[2] = 2.0, -1.0
    u = np.zeros((3, m - 1, 2))
    u[0, :, 0] = 3.0
    junk = np.full((3, 2 * (m - 1)), 7.25)
    return T, Df.reshape(18), join(pos, junk), join(pos, u.reshape(3, -1))
