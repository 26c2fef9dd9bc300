"""The prediction fit of include/gtop_prediction.h (gtop_fit_predictions[_device], gtop_refresh_box_predictions_device)
restated in Python scalars, operation by operation: every `+ - * /` below is one rounded fp64 operation on Python
floats, math.sqrt is correctly rounded, and the one fused step (the centre's Horner) is tests/box_poly_twin.fma.  The
host entry and the kernel reproduce these bits.

`mutant` switches on ONE deliberate error, for tests/test_predict_twin.py's check that its checks can fail:
    "reg_sign"     the regulariser enters with the wrong sign
    "sigma_sq"     lambda / sigma^2 for lambda / sigma^3
    "shift_sign"   the Taylor shift by +t_last
    "no_horizon"   the interval ends at t_last
    "serial_sum"   the chunk's pair tree replaced by a left-to-right sum
    "back_order"   the back substitution subtracts from the far end first
"""
import math

import numpy as np

from tests.box_poly_twin import fma

POLYFIT, CONST_VEL = 0, 1
OK, LOWERED, EMPTY, BAD = 0, 1, 2, 3
INFO = 12
LOCAL = 20
CHUNK = 64
PIVOT_FLOOR = 2.0 ** -40


def tree_sum(v, mutant=None):
    """One chunk of up to 64 values: missing lanes are +0.0, then the balanced pair tree, six levels."""
    lane = [float(x) for x in v] + [0.0] * (CHUNK - len(v))
    if mutant == "serial_sum":
        acc = 0.0
        for x in lane:
            acc = acc + x
        return acc
    while len(lane) > 1:
        lane = [lane[2 * k] + lane[2 * k + 1] for k in range(len(lane) // 2)]
    return lane[0]


def chunked_sum(v, mutant=None):
    """Chunk sums added in chunk order, from +0.0."""
    acc = 0.0
    for lo in range(0, len(v), CHUNK):
        acc = acc + tree_sum(v[lo:lo + CHUNK], mutant)
    return acc


def history(hist_n, count, head, H):
    """The `count` samples of one object, oldest first: slot (head + i) mod H."""
    hm = int(head) % H
    return [[float(x) for x in hist_n[(hm + i) % H]] for i in range(count)]


def system(s, q, lam_e, e, mutant=None):
    """(A 6 x 6, b 6 x 3) of the local system from the scaled times s and the positions q."""
    pw = []
    for si in s:
        p = [1.0]
        for _ in range(10):
            p.append(p[-1] * si)
        pw.append(p)
    S = [chunked_sum([p[j] for p in pw], mutant) for j in range(11)]
    M = [[chunked_sum([pw[i][j] * q[i][k] for i in range(len(s))], mutant) for k in range(3)] for j in range(6)]
    ep = [1.0, e]
    for _ in range(6):
        ep.append(ep[-1] * e)
    A = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        for k in range(6):
            A[j][k] = S[j + k]
            if j >= 2 and k >= 2:
                p = j + k - 3
                w = float(j * (j - 1) * k * (k - 1)) / float(p)
                d = ep[p] - (-1.0 if p % 2 else 1.0)
                term = (lam_e * w) * d
                A[j][k] = S[j + k] - term if mutant == "reg_sign" else S[j + k] + term
    return A, M


def cholesky(A, deg):
    """Row by row, left-to-right subtractions.  Returns (L, deg): deg lowered to below the first row whose pivot d is
    not > 2^-40 A_jj (the leading rows of the factor do not depend on deg, so factoring again is stopping there)."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(deg + 1):
        for k in range(j + 1):
            acc = A[j][k]
            for p in range(k):
                acc = acc - L[j][p] * L[k][p]
            if k < j:
                L[j][k] = acc / L[k][k]
            else:
                if not acc > PIVOT_FLOOR * A[j][j]:
                    return L, j - 1
                L[j][j] = math.sqrt(acc)
    return L, deg


def substitute(L, deg, b, mutant=None):
    """g_0 .. g_deg of one axis (higher entries 0): forward, then back; sums left to right in ascending index."""
    y = [0.0] * 6
    for j in range(deg + 1):
        acc = b[j]
        for p in range(j):
            acc = acc - L[j][p] * y[p]
        y[j] = acc / L[j][j]
    g = [0.0] * 6
    for j in range(deg, -1, -1):
        acc = y[j]
        order = range(deg, j, -1) if mutant == "back_order" else range(j + 1, deg + 1)
        for p in order:
            acc = acc - L[p][j] * g[p]
        g[j] = acc / L[j][j]
    return g


def to_row(g, sigma, t_last, mutant=None):
    """a_j = g_j / sigma^j, then the Taylor shift to absolute time."""
    sp = [1.0]
    for _ in range(5):
        sp.append(sp[-1] * sigma)
    c = [g[j] / sp[j] for j in range(6)]
    x0 = t_last if mutant == "shift_sign" else -t_last
    for i in range(6):
        for j in range(4, i - 1, -1):
            c[j] = c[j] + c[j + 1] * x0
    return c


def centre(c6, t):
    """gtop_box_poly_centre: Horner in explicit fmas."""
    r = float(c6[5])
    for i in (4, 3, 2, 1, 0):
        r = fma(r, t, c6[i])
    return r


def finite(x):
    return not (math.isinf(x) or math.isnan(x))


def fit_one(samples, mode=POLYFIT, degree=5, lam=1.0, horizon=0.0, regularise_horizon=0, mutant=None, detail=None):
    """One object.  Returns (info (12,), coef (18,) or None, t_range (2,) or None, local (20,) or None); the last three
    are None exactly when the status is EMPTY or BAD (the outputs stay untouched).  detail: a dict that receives the
    local system's data (s, lam_e, e, A, b, L, deg) for the exact-arithmetic tests."""
    count = len(samples)
    info = [0.0] * INFO
    info[1] = float(count)

    def bad():
        info[0] = float(BAD)
        return np.array(info), None, None, None

    if count == 0:
        info[0] = float(EMPTY)
        return np.array(info), None, None, None
    if not all(finite(x) for smp in samples for x in smp):
        return bad()
    t_first, t_last = samples[0][3], samples[-1][3]
    if count >= 2 and not t_last - t_first > 0.0:
        return bad()
    q = [smp[:3] for smp in samples]
    status = OK
    g = [[0.0] * 6 for _ in range(3)]
    if count == 1:
        status, deg, sigma, t_start = LOWERED, 0, 0.0, t_last
        coef = [[q[0][k], 0.0, 0.0, 0.0, 0.0, 0.0] for k in range(3)]
        for k in range(3):
            g[k][0] = q[0][k]
    elif mode == CONST_VEL:
        t1, t2 = samples[-2][3], t_last
        if not t1 < t2:
            return bad()
        deg, sigma, t_start = 1, t2 - t1, t1
        coef = []
        for k in range(3):
            d = q[-1][k] - q[-2][k]
            c1 = d / sigma
            c0 = q[-1][k] - c1 * t2
            coef.append([c0, c1, 0.0, 0.0, 0.0, 0.0])
            g[k][0], g[k][1] = q[-1][k], d
    else:
        sigma, t_start = t_last - t_first, t_first
        s = [(smp[3] - t_last) / sigma for smp in samples]
        e = horizon / sigma if regularise_horizon else 0.0
        lam_e = lam / (sigma * sigma) if mutant == "sigma_sq" else lam / ((sigma * sigma) * sigma)
        A, M = system(s, q, lam_e, e, mutant)
        deg0 = min(degree, count - 1)
        L, deg = cholesky(A, deg0)
        if deg < degree:
            status = LOWERED
        coef = []
        for k in range(3):
            g[k] = substitute(L, deg, [M[j][k] for j in range(6)], mutant)
            if not all(finite(x) for x in g[k]):
                return bad()
            coef.append(to_row(g[k], sigma, t_last, mutant))
        if detail is not None:
            detail.update(s=s, lam_e=lam_e, e=e, A=A, b=M, L=L, deg=deg, sigma=sigma, t_last=t_last)
    if not all(finite(x) for ck in coef for x in ck):
        return bad()
    t_end = t_last if mutant == "no_horizon" else t_last + horizon
    # the residuals, at the consumers' own centre
    resmax = [0.0, 0.0, 0.0]
    sq = []
    for smp in samples:
        r = [centre(coef[k], smp[3]) - smp[k] for k in range(3)]
        for k in range(3):
            resmax[k] = max(resmax[k], abs(r[k]))
        sq.append((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    rms = math.sqrt(chunked_sum(sq, mutant) / float(3 * count))
    info[0], info[2] = float(status), float(deg)
    info[3], info[4], info[5] = t_start, t_last, t_end
    info[6:9] = resmax
    info[9] = rms
    local = [x for gk in g for x in gk] + [t_last, sigma]
    return np.array(info), np.array([x for ck in coef for x in ck]), np.array([t_start, t_end]), np.array(local)


def fit(hist, count, head=None, sentinel=None, **opts):
    """The batch: hist (N, H, 4), count (N,), head (N,) or None -> (coef (N, 18), t_range (N, 2), info (N, 12), local
    (N, 20)); rows of an EMPTY or BAD object hold `sentinel` (NaN when None) in coef, t_range and local.  A count
    outside 0 .. H is clamped and the object is BAD."""
    hist = np.asarray(hist, dtype=np.float64)
    N, H = hist.shape[0], hist.shape[1]
    fill = np.nan if sentinel is None else sentinel
    coef, t_range = np.full((N, 18), fill), np.full((N, 2), fill)
    info, local = np.zeros((N, INFO)), np.full((N, LOCAL), fill)
    for n in range(N):
        raw = int(count[n])
        cnt = min(max(raw, 0), H)
        smp = history(hist[n], cnt, 0 if head is None else head[n], H)
        if cnt != raw:
            info[n, 0], info[n, 1] = BAD, cnt
            continue
        info[n], c, tr, loc = fit_one(smp, **opts)
        if c is not None:
            coef[n], t_range[n], local[n] = c, tr, loc
    return coef, t_range, info, local


def half_extents(scale, inflate, info):
    """What the refresh writes beside the fit: 0.5 scale_k + inflate resmax_k, one rounded operation each."""
    scale = np.asarray(scale, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(scale)
    for n in range(scale.shape[0]):
        for k in range(3):
            out[n, k] = 0.5 * float(scale[n, k]) + float(inflate) * float(info[n, 6 + k])
    return out


# ---- the committed draws: shared by the CPU and the GPU tests ----
KINDS = ("full", "nan", "empty", "one", "two", "five", "six", "flat", "over", "negative", "dup", "inf_time")
_batches = {}


def make_batch(N, H, seed=0):
    """(hist (N, H, 4), count (N,) int32, head (N,) int32): object n is of kind KINDS[n] while they last, then of a
    random count in 2 .. H.  Counts are cut to H.  Slots outside an object's samples hold NaN (nothing may read them);
    heads wrap, and a few lie outside 0 .. H-1 (the ring takes the non-negative remainder).  Positions follow a cubic
    with noise of 1 cm; times start up to 100 s from 0 and span 0.2 .. 4 s."""
    key = (N, H, seed)
    if key in _batches:
        return _batches[key]
    rng = np.random.default_rng(1000 * H + 10 * N + seed)
    hist = np.full((N, H, 4), np.nan)
    count = np.zeros(N, dtype=np.int32)
    head = rng.integers(0, H, N).astype(np.int32)
    head[::5] += H * rng.integers(-2, 3, len(head[::5])).astype(np.int32)
    for n in range(N):
        kind = KINDS[n] if n < len(KINDS) else "random"
        want = dict(full=H, nan=min(4, H), empty=0, one=1, two=2, five=5, six=6, flat=min(3, H), over=H, negative=0,
                    dup=6, inf_time=min(3, H)).get(kind)
        c = int(rng.integers(2, H + 1)) if want is None else min(want, H)
        t_start, span = rng.uniform(0.0, 100.0), rng.uniform(0.2, 4.0)
        t = np.sort(rng.uniform(t_start, t_start + span, c))
        if kind == "dup" and c >= 3:
            t[2] = t[1]
        if kind == "flat":
            t[:] = t[0]
        a = rng.normal(size=(3, 4)) * np.array([1.0, 1.0, 0.5, 0.1])
        hm = int(head[n]) % H
        for i in range(c):
            u = t[i] - t_start
            hist[n, (hm + i) % H, :3] = a[:, 0] + a[:, 1] * u + a[:, 2] * u * u + a[:, 3] * u ** 3 + 0.01 * rng.normal(size=3)
            hist[n, (hm + i) % H, 3] = t[i]
        if kind == "nan" and c:
            hist[n, (hm + c - 1) % H, 1] = np.nan
        if kind == "inf_time" and c:
            hist[n, (hm + c - 1) % H, 3] = np.inf
        count[n] = c + 2 if kind == "over" else (-1 if kind == "negative" else c)
    _batches[key] = (hist, count, head)
    return _batches[key]


_fits = {}


def fit_batch(N, H, mode, seed=0, sentinel=7.0, **opts):
    """fit() of make_batch(N, H, seed), computed once per option set and left unchanged."""
    key = (N, H, mode, seed, sentinel, tuple(sorted(opts.items())))
    if key not in _fits:
        hist, count, head = make_batch(N, H, seed)
        _fits[key] = fit(hist, count, head, sentinel=sentinel, mode=mode, **opts)
    return _fits[key]
