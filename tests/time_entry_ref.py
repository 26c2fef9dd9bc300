"""The time pass of csrc/gtop_time_pass.h — cost, gT, the six parts columns, gt0 and gx — restated in vectorised numpy
with the rounding-error MAGNITUDE of every entry beside it, for tests/test_time_entrywise_bound.py (which holds this
module against 40-digit arithmetic) and tests/test_gpu_time_entrywise.py (which holds the kernels to it on every row).

Why numpy and not the C oracle: every array here is (rows, segments, 30 samples), so the largest GPU case (130 x 6,
65 x 7 with 32 boxes, 2 x 227) is evaluated in well under a second, and the magnitudes stand beside the values line by
line, where they can be read.  Nothing is shared with the three pure-Python twins (tests/time_twin.py,
tests/time_moving_twin.py, tests/joint_twin.py) but the semantics they state: float round trips as the identity in the
derivative, the field differentiable inside a cell, sgn(+-0) = 0, the sample count held fixed, d t_i / d T = i / 30, the
lookup static for tau < 0 and out of the map.

Magnitudes follow the rule of oracle_cost_grad_mag (oracle/gtop_oracle.h): absolute values of the inputs, additions for
subtractions, products of magnitudes.  The two cancellations of the pass are therefore carried as the sum of their
terms: the closed-form P / V / A with the coefficients formed from them, and c' = (...) T^-n - n c_n / T.  exp carries
1 + (|argument's terms|) / r for its argument's error.  A float-rounded velocity or acceleration enters by the magnitude
of its pre-rounding polynomial (it may have cancelled), the corner values of a box-lowered corner by the magnitude of
the box's faces.

Decisions a correct kernel may take either way get an ABSOLUTE allowance, they do not drop the row:
  * the float rounding of a position / velocity / acceleration whose pre-rounding double is within TIE (2^9 u64 of its
    magnitude) of a rounding boundary, and the sign of a velocity / acceleration within TIE of 0: the sample's terms are
    evaluated again with that one coordinate at its other value, and twice the change of every entry is allowed;
  * the corner-or-box argmin and the inside / outside face of a box within TIE of a tie: the corner's time derivative
    jumps there (the value does not), so twice the largest box speed times the sample's weight is allowed on [3], q and
    what is summed from them.
A velocity whose float spacing is below 2^-42 of its magnitude is noise, not a decision (oracle float_margin): it is
carried by its magnitude, vel_norm included.

`variant`: a set of names, for tests/test_time_entrywise_bound.py — deliberately wrong lines (WRONG) and pure changes
of rounding (ROUNDING)."""
import numpy as np

U64 = 2.0 ** -53
TIE = 2.0 ** 9 * U64
NOISE = 2.0 ** -42

# variant names: family -> wrong lines; and the changes of rounding only
WRONG = {
    "gT": ("c4_factor", "fr_float", "w30_float", "jerk_576"),
    "MOV": ("box_vel_1e-8", "tau_float", "R_float"),
    "GX": ("table_s4_1e-8", "table_e5_1e-8", "wv_no_eps"),
}
# wrong lines the 1e-5 checks see too, or that the bound does not resolve (tests/test_time_entrywise_bound.py says which)
OTHER = ("R_drops_last_q", "q_past_bound", "swap_acc_jerk", "own_fr_float")
ROUNDING = ("horner", "mul_iT")


class Field:
    """The distance field a lookup reads: origin, res, grid, dist (nx, ny, nz), min_range, max_range."""

    def __init__(self, origin, res, grid, dist, min_range=None, max_range=None):
        self.origin = np.asarray(origin, dtype=np.float64)
        self.res = float(res)
        self.res_inv = 1.0 / self.res
        self.grid = np.asarray(grid, dtype=np.int64)
        self.dist = np.asarray(dist, dtype=np.float64).reshape(tuple(self.grid))
        self.min_range = self.origin.copy() if min_range is None else np.asarray(min_range, dtype=np.float64)
        self.max_range = (self.origin + self.grid * self.res) if max_range is None else np.asarray(max_range, dtype=np.float64)

    @classmethod
    def from_oracle(cls, osdf):
        """oracle.Sdf -> Field (the same buffer, the descriptor's ranges)."""
        return cls(osdf.origin, osdf.resolution, osdf.grid, osdf.dist, np.array(osdf.c.min_range[:]),
                   np.array(osdf.c.max_range[:]))


def waypoint_rows(Df, x, m):
    """(B, m + 1, 3 axes, 3): position, velocity, acceleration of every waypoint (Df: start | end per axis)."""
    B = x.shape[0]
    Df = np.asarray(Df, dtype=np.float64).reshape(B, 3, 6)
    dp = np.asarray(x, dtype=np.float64).reshape(B, 3, 3 * m - 3)
    w = np.zeros((B, m + 1, 3, 3))
    w[:, 0], w[:, m] = Df[:, :, :3], Df[:, :, 3:]
    for i in range(1, m):
        w[:, i] = dp[:, :, 3 * (i - 1):3 * i]
    return w


def table(T):
    """H (..., 6, 6): H[e, n] = d c_n / d (p0, v0, a0, pT, vT, aT)[e] (include/gtop_joint.h)."""
    H = np.zeros(T.shape + (6, 6))
    H[..., 0, 0], H[..., 1, 1], H[..., 2, 2] = 1.0, 1.0, 0.5
    for n, col in ((3, (-10, -6, -1.5, 10, -4, 0.5)), (4, (15, 8, 1.5, -15, 7, -1.0)), (5, (-6, -3, -0.5, 6, -3, 0.5))):
        for e, v in enumerate(col):
            H[..., e, n] = v / T ** (n - (e % 3))
    return H


def _float_alt(pre, mag, noise):
    """(rounded, flagged, other value, is noise, margin): the float rounding of `pre`, whether it is within TIE * mag of
    a rounding boundary (then: the float on the other side), whether it is noise, and the margin relative to mag."""
    f = pre.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    is_noise = (up - f <= NOISE * mag) if noise else np.zeros(pre.shape, dtype=bool)
    hi, lo = 0.5 * (f + up), 0.5 * (f + dn)
    with np.errstate(divide="ignore", invalid="ignore"):
        marg = np.where((mag > 0) & ~is_noise, np.minimum(np.abs(pre - hi), np.abs(pre - lo)) / mag, np.inf)
    flagged = marg < TIE
    alt = np.where(np.abs(pre - hi) < np.abs(pre - lo), up, dn)
    return f, flagged, alt, is_noise, marg


def _trilinear(diff, wm, V, Vm):
    """sum_c w_c V_c and its magnitude: sum_c w_c Vm_c + sum_k wm_k |d value / d w_k| (oracle sdf_query_mag_v)."""
    w = [(np.abs(1 - diff[..., k]), np.abs(diff[..., k])) for k in range(3)]
    d = diff
    v00 = (1 - d[..., 0]) * V[..., 0, 0, 0] + d[..., 0] * V[..., 1, 0, 0]
    v01 = (1 - d[..., 0]) * V[..., 0, 0, 1] + d[..., 0] * V[..., 1, 0, 1]
    v10 = (1 - d[..., 0]) * V[..., 0, 1, 0] + d[..., 0] * V[..., 1, 1, 0]
    v11 = (1 - d[..., 0]) * V[..., 0, 1, 1] + d[..., 0] * V[..., 1, 1, 1]
    v0 = (1 - d[..., 1]) * v00 + d[..., 1] * v10
    v1 = (1 - d[..., 1]) * v01 + d[..., 1] * v11
    val = (1 - d[..., 2]) * v0 + d[..., 2] * v1
    mag = 0.0
    for x in (0, 1):
        for y in (0, 1):
            for z in (0, 1):
                mag = mag + w[0][x] * w[1][y] * w[2][z] * Vm[..., x, y, z]
    sens = [0.0, 0.0, 0.0]
    for a in (0, 1):
        for b in (0, 1):
            sens[0] = sens[0] + w[1][a] * w[2][b] * np.abs(V[..., 1, a, b] - V[..., 0, a, b])
            sens[1] = sens[1] + w[0][a] * w[2][b] * np.abs(V[..., a, 1, b] - V[..., a, 0, b])
            sens[2] = sens[2] + w[0][a] * w[1][b] * np.abs(V[..., a, b, 1] - V[..., a, b, 0])
    mag = mag + wm[..., 0] * sens[0] + wm[..., 1] * sens[1] + wm[..., 2] * sens[2]
    return val, mag, (v00, v01, v10, v11, v0, v1)


def _gradient(diff, wm, V, Vm, res_inv, inter):
    """The trilinear value's gradient (sdf_map.cpp:231-239) and its magnitude: every corner difference as the sum of the
    two corners' magnitudes, plus the other two weights' error times the gradient's sensitivity to them."""
    d = diff
    v00, v01, v10, v11, v0, v1 = inter
    gx = (1 - d[..., 2]) * (1 - d[..., 1]) * (V[..., 1, 0, 0] - V[..., 0, 0, 0])
    gx = gx + (1 - d[..., 2]) * d[..., 1] * (V[..., 1, 1, 0] - V[..., 0, 1, 0])
    gx = gx + d[..., 2] * (1 - d[..., 1]) * (V[..., 1, 0, 1] - V[..., 0, 0, 1])
    gx = gx + d[..., 2] * d[..., 1] * (V[..., 1, 1, 1] - V[..., 0, 1, 1])
    g = np.stack([gx * res_inv, ((1 - d[..., 2]) * (v10 - v00) + d[..., 2] * (v11 - v01)) * res_inv, (v1 - v0) * res_inv], axis=-1)
    w = [(np.abs(1 - d[..., k]), np.abs(d[..., k])) for k in range(3)]
    gm = []
    for k in range(3):
        o1, o2 = (k + 1) % 3, (k + 2) % 3
        e = 0.0
        for a in (0, 1):          # offset along o1
            for b in (0, 1):      # offset along o2
                i0, i1 = [0, 0, 0], [0, 0, 0]
                i0[o1] = i1[o1] = a
                i0[o2] = i1[o2] = b
                i1[k] = 1
                e = e + w[o1][a] * w[o2][b] * (Vm[(Ellipsis, *i1)] + Vm[(Ellipsis, *i0)])
        for j, l in ((o1, o2), (o2, o1)):      # the k-gradient's sensitivity to weight j, blended along l
            for b in (0, 1):
                c = lambda ok, oj: V[(Ellipsis, *[ok if a == k else (oj if a == j else b) for a in range(3)])]
                e = e + wm[..., j] * w[l][b] * np.abs((c(1, 1) - c(0, 1)) - (c(1, 0) - c(0, 0)))
        gm.append(e * res_inv)
    return g, np.stack(gm, axis=-1)


def _boxes_at(boxes, tau, variant):
    """Per box: centre, its magnitude, half extent, velocity and its magnitude at the times tau (...,) -> lists of
    (..., 3) arrays."""
    scale = np.asarray(boxes["scale"], dtype=np.float64).reshape(-1, 3)
    out = []
    for b in range(len(scale)):
        if boxes.get("coef") is not None:
            cf = np.asarray(boxes["coef"], dtype=np.float64).reshape(-1, 3, 6)[b]
            tr = boxes.get("t_range")
            t1, t2 = (-np.inf, np.inf) if tr is None else np.asarray(tr, dtype=np.float64).reshape(-1, 2)[b]
            tc = np.minimum(np.maximum(tau, t1), t2)[..., None]
            moves = ((tau > t1) & (tau < t2))[..., None]
            c = cf[:, 5]
            for j in (4, 3, 2, 1, 0):
                c = c * tc + cf[:, j]
            cm = sum(np.abs(cf[:, j]) * np.abs(tc) ** j for j in range(6))
            v = 5.0 * cf[:, 5]
            for j in (4, 3, 2, 1):
                v = v * tc + j * cf[:, j]
            vm = sum(j * np.abs(cf[:, j]) * np.abs(tc) ** (j - 1) for j in range(1, 6))
            v, vm = np.where(moves, v, 0.0), np.where(moves, vm, 0.0)
            tmarg = np.minimum(np.abs(tau - t1), np.abs(tau - t2)) / (np.abs(tau) + 1e-300)
        else:
            p0, vel = (np.asarray(boxes[k], dtype=np.float64).reshape(-1, 3)[b] for k in ("p0", "vel"))
            t = tau[..., None]
            c, cm = p0 + vel * t, np.abs(p0) + np.abs(vel) * np.abs(t)
            v, vm = np.broadcast_to(vel, c.shape), np.broadcast_to(np.abs(vel), c.shape)
            tmarg = np.full(tau.shape, np.inf)
        if "box_vel_1e-8" in variant:
            v = v * (1.0 + 1e-8)
        out.append((c, cm, 0.5 * scale[b], v, vm, tmarg))
    return out


def _lookup(F, pos, tau, boxes, variant):
    """evaluateEDTWithGrad(pos, tau) and d dist / d tau with their magnitudes -> dict."""
    out = np.any((pos < F.min_range + 1e-4) | (pos > F.max_range - 1e-4), axis=-1)
    with np.errstate(invalid="ignore", over="ignore"):
        idx = np.floor(((pos - 0.5 * F.res) - F.origin) * F.res_inv)
    idx = np.where(out[..., None], 0, np.nan_to_num(idx)).astype(np.int64)
    ip = (idx + 0.5) * F.res + F.origin
    diff = (pos - ip) * F.res_inv
    wm = (np.abs(pos) + np.abs(ip)) * F.res_inv + 1.0
    shape = pos.shape[:-1]
    V = np.empty(shape + (2, 2, 2))
    for x in (0, 1):
        for y in (0, 1):
            for z in (0, 1):
                ii = [np.clip(idx[..., k] + o, 0, F.grid[k] - 1) for k, o in enumerate((x, y, z))]
                V[..., x, y, z] = F.dist[ii[0], ii[1], ii[2]]
    Vm = np.abs(V)
    D, Dm = np.zeros_like(V), np.zeros_like(V)
    lowered = np.zeros(shape, dtype=bool)
    tie = np.zeros(shape, dtype=bool)
    speed = np.zeros(shape)
    marg_face = np.full(shape, np.inf)
    marg_min = np.full(shape, np.inf)
    if boxes is not None and len(np.asarray(boxes["scale"]).reshape(-1, 3)):
        on = ~out & (tau >= 0.0)
        low = np.zeros(V.shape, dtype=bool)
        for c, cm, h, cv, cvm, tmarg in _boxes_at(boxes, tau, variant):
            bmin, bmax, fm = c - h, c + h, cm + h
            speed = np.maximum(speed, cvm.sum(axis=-1))
            tie |= on & (tmarg < TIE)
            d1, e1, d1m, e1m = (np.zeros(shape + (3, 2)) for _ in range(4))
            for o in (0, 1):
                pt = (idx + o + 0.5) * F.res + F.origin
                below, above = pt < bmin, pt > bmax
                d1[..., o] = np.where(below, bmin - pt, np.where(above, pt - bmax, 0.0))
                e1[..., o] = np.where(below, cv, np.where(above, -cv, 0.0))
                d1m[..., o] = np.where(below | above, np.abs(pt) + fm, 0.0)
                e1m[..., o] = np.where(below | above, cvm, 0.0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    mf = np.minimum(np.abs(pt - bmin), np.abs(pt - bmax)) / (np.abs(pt) + fm)
                marg_face = np.where(on, np.minimum(marg_face, mf.min(axis=-1)), marg_face)
                tie |= on & (mf.min(axis=-1) < TIE)
            for x in (0, 1):
                for y in (0, 1):
                    for z in (0, 1):
                        d2 = np.sqrt(d1[..., 0, x] ** 2 + d1[..., 1, y] ** 2 + d1[..., 2, z] ** 2)
                        d2m = np.sqrt(d1m[..., 0, x] ** 2 + d1m[..., 1, y] ** 2 + d1m[..., 2, z] ** 2)
                        num = d1[..., 0, x] * e1[..., 0, x] + d1[..., 1, y] * e1[..., 1, y] + d1[..., 2, z] * e1[..., 2, z]
                        numm = (d1m[..., 0, x] * e1m[..., 0, x] + d1m[..., 1, y] * e1m[..., 1, y]
                                + d1m[..., 2, z] * e1m[..., 2, z])
                        with np.errstate(divide="ignore", invalid="ignore"):
                            der = np.where(d2 > 0.0, num / d2, 0.0)
                            derm = np.where(d2 > 0.0, numm / d2 + np.abs(num) * d2m / (d2 * d2), 0.0)
                            mm = np.abs(d2 - V[..., x, y, z]) / (d2m + Vm[..., x, y, z])
                        # (against a value an earlier box has set the earlier box wins a tie the same way)
                        marg_min = np.where(on, np.minimum(marg_min, np.nan_to_num(mm, nan=np.inf)), marg_min)
                        tie |= on & (mm < TIE)
                        lower = on & (d2 < V[..., x, y, z])
                        V[..., x, y, z] = np.where(lower, d2, V[..., x, y, z])
                        Vm[..., x, y, z] = np.where(lower, d2m, Vm[..., x, y, z])
                        D[..., x, y, z] = np.where(lower, der, D[..., x, y, z])
                        Dm[..., x, y, z] = np.where(lower, derm, Dm[..., x, y, z])
                        low[..., x, y, z] |= lower
        lowered = low.any(axis=(-1, -2, -3))
    dist, dm, inter = _trilinear(diff, wm, V, Vm)
    grad, gm = _gradient(diff, wm, V, Vm, F.res_inv, inter)
    dtau, dtm, _ = _trilinear(diff, wm, D, Dm)
    o3 = out[..., None]
    with np.errstate(invalid="ignore"):
        u = ((pos - 0.5 * F.res) - F.origin) * F.res_inv
        marg_cell = np.where(out, np.inf, np.min(np.abs(u - np.rint(u)) / ((np.abs(pos) + np.abs(F.origin) + F.res) * F.res_inv), axis=-1))
    lo, hi = F.min_range + 1e-4, F.max_range - 1e-4
    marg_map = np.min(np.minimum(np.abs(pos - lo), np.abs(pos - hi)) / (np.abs(pos) + np.abs(F.min_range) + np.abs(F.max_range) + 1e-4), axis=-1)
    return dict(dist=np.where(out, -1.0, dist), dm=np.where(out, 1.0, dm), grad=np.where(o3, 0.0, grad),
                gm=np.where(o3, 0.0, gm), dtau=np.where(out, 0.0, dtau), dtm=np.where(out, 0.0, dtm),
                lowered=lowered & ~out, tie=tie & ~out, speed=speed, marg_face=marg_face, marg_min=marg_min,
                marg_cell=marg_cell, marg_map=marg_map)


def reference(T, Df, x, field, p, t0=None, boxes=None, variant=()):
    """The pass on every row.  T (B, m) or (m,), Df (B, 3, 6) or (B, 18), x (B, 9 (m - 1)); p: the parameter dict of the
    twins (oracle.OPTI_NODE_PARAMS with changes); t0 None / scalar / (B,); boxes None or dict(p0, vel, scale) /
    dict(coef, scale, t_range), the dict of oracle.eval_batch_ext.

    Returns dict(val, mag, allow: dicts with cost (B,), gT (B, m), parts (B, m, 6), gt0 (B,), gx (B, 9 (m - 1));
    margins: dict name -> (B,) smallest relative margin of a row's decisions; lowered (B, m); counts (B, m))."""
    variant = set(variant)
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    m = x.shape[1] // 9 + 1
    T = np.ascontiguousarray(np.broadcast_to(np.asarray(T, dtype=np.float64), (B, m)))
    t0 = np.broadcast_to(0.0 if t0 is None else np.asarray(t0, dtype=np.float64), (B,))
    w = waypoint_rows(Df, x, m)
    ws = 0.0 if p["step"] == 1 else p["ws"]
    dyn = bool(p.get("enable_dyn", 0)) and p["step"] == 2
    colli = not abs(p["wc"]) < 1e-4
    wc = p["wc"]

    # ---- coefficients and c' (B, m, 3 axes[, 6]) ----
    Tk = T[:, :, None]
    p0, v0, a0 = (w[:, :-1, :, j] for j in range(3))
    pT, vT, aT = (w[:, 1:, :, j] for j in range(3))
    ab = np.abs
    P, Pm = pT - p0 - v0 * Tk - 0.5 * a0 * Tk * Tk, ab(pT) + ab(p0) + ab(v0) * Tk + 0.5 * ab(a0) * Tk * Tk
    V, Vm = (vT - v0 - a0 * Tk) * Tk, (ab(vT) + ab(v0) + ab(a0) * Tk) * Tk
    A, Am = (aT - a0) * Tk * Tk, (ab(aT) + ab(a0)) * Tk * Tk
    dP, dPm = -v0 - a0 * Tk, ab(v0) + ab(a0) * Tk
    dV, dVm = vT - v0 - 2.0 * a0 * Tk, ab(vT) + ab(v0) + 2.0 * ab(a0) * Tk
    dA, dAm = 2.0 * (aT - a0) * Tk, 2.0 * (ab(aT) + ab(a0)) * Tk
    if "mul_iT" in variant:
        iT = 1.0 / Tk
        iT3 = iT * iT * iT
        inv = {3: iT3, 4: iT3 * iT, 5: iT3 * iT * iT}
        div = lambda v, n: v * inv[n]
        divT = lambda v: v * iT
    else:
        div = lambda v, n: v / Tk ** n
        divT = lambda v: v / Tk
    c, cm = np.zeros((B, m, 3, 6)), np.zeros((B, m, 3, 6))
    c[..., 0], c[..., 1], c[..., 2] = p0, v0, 0.5 * a0
    cm[..., :3] = ab(c[..., :3])
    c[..., 3], cm[..., 3] = div(10 * P - 4 * V + 0.5 * A, 3), div(10 * Pm + 4 * Vm + 0.5 * Am, 3)
    c[..., 4], cm[..., 4] = div(7 * V - 15 * P - A, 4), div(7 * Vm + 15 * Pm + Am, 4)
    c[..., 5], cm[..., 5] = div(6 * P - 3 * V + 0.5 * A, 5), div(6 * Pm + 3 * Vm + 0.5 * Am, 5)
    four = 4.0 * (1.0 + 1e-9) if "c4_factor" in variant else 4.0
    dc, dcm = np.zeros((B, m, 3, 6)), np.zeros((B, m, 3, 6))
    dc[..., 3] = div(10 * dP - 4 * dV + 0.5 * dA, 3) - divT(3 * c[..., 3])
    dc[..., 4] = div(7 * dV - 15 * dP - dA, 4) - divT(four * c[..., 4])
    dc[..., 5] = div(6 * dP - 3 * dV + 0.5 * dA, 5) - divT(5 * c[..., 5])
    dcm[..., 3] = div(10 * dPm + 4 * dVm + 0.5 * dAm, 3) + divT(3 * cm[..., 3])
    dcm[..., 4] = div(7 * dVm + 15 * dPm + dAm, 4) + divT(4 * cm[..., 4])
    dcm[..., 5] = div(6 * dPm + 3 * dVm + 0.5 * dAm, 5) + divT(5 * cm[..., 5])

    # ---- the jerk term c'Qc, its derivative, and the chain 2 ws (Qc) for gx ----
    def jerk(c3, c4, c5, e3, e4, e5, k576):
        q3 = 36 * Tk * c3 + 72 * Tk ** 2 * c4 + 120 * Tk ** 3 * c5
        q4 = 72 * Tk ** 2 * c3 + 192 * Tk ** 3 * c4 + 360 * Tk ** 4 * c5
        q5 = 120 * Tk ** 3 * c3 + 360 * Tk ** 4 * c4 + 720 * Tk ** 5 * c5
        J = c3 * q3 + c4 * q4 + c5 * q5
        dJ = (36 * c3 * c3 + 288 * Tk * c3 * c4 + 720 * Tk ** 2 * c3 * c5 + k576 * Tk ** 2 * c4 * c4
              + 2880 * Tk ** 3 * c4 * c5 + 3600 * Tk ** 4 * c5 * c5) + 2 * (q3 * e3 + q4 * e4 + q5 * e5)
        return J.sum(axis=-1), dJ.sum(axis=-1), np.stack([q3, q4, q5], axis=-1)
    k576 = 576.0 * (1.0 + 1e-8) if "jerk_576" in variant else 576.0
    J, dJ, Q = jerk(c[..., 3], c[..., 4], c[..., 5], dc[..., 3], dc[..., 4], dc[..., 5], k576)
    Jm, dJm, Qm = jerk(cm[..., 3], cm[..., 4], cm[..., 5], dcm[..., 3], dcm[..., 4], dcm[..., 5], 576.0)
    H = table(T)                                               # (B, m, 6 entries, 6 powers)
    if "table_s4_1e-8" in variant:
        H[..., 1, 4] *= 1.0 + 1e-8
    if "table_e5_1e-8" in variant:
        H[..., 4, 5] *= 1.0 + 1e-8
    Hm = ab(table(T))
    Hj = H.copy()
    if "swap_acc_jerk" in variant and m > 2:                   # waypoint 1's acceleration entry, in the jerk term only:
        Hj[:, 0, 5, 3:], Hj[:, 1, 2, 3:] = H[:, 1, 2, 3:], H[:, 0, 5, 3:]      # end part of segment 0 <-> start part of 1
    seg_gx = 2.0 * ws * np.einsum("bskn,bsen->bske", Q, Hj[..., 3:])          # (B, m, 3 axes, 6 entries)
    seg_gxm = 2.0 * ab(ws) * np.einsum("bskn,bsen->bske", Qm, Hm[..., 3:])
    seg_gxa = np.zeros_like(seg_gx)

    val = dict(parts=np.zeros((B, m, 6)))
    mag = dict(parts=np.zeros((B, m, 6)))
    allow = dict(parts=np.zeros((B, m, 6)))
    val["parts"][..., 0], val["parts"][..., 2] = ws * J, ws * dJ
    mag["parts"][..., 0], mag["parts"][..., 2] = ab(ws) * Jm, ab(ws) * dJm
    margins = {k: np.full(B, np.inf) for k in ("float rounding", "sign", "sample count", "cell choice", "in-map test",
                                               "box face", "box argmin")}
    lowered = np.zeros((B, m), dtype=bool)
    counts = np.zeros((B, m), dtype=np.int64)

    if colli:
        # ---- sample times: the reference's chain t += dt from 1e-3, the count t < T held fixed ----
        dt = T / 30.0
        t = np.empty((B, m, 30))
        t[..., 0] = 1e-3
        for i in range(1, 30):
            t[..., i] = t[..., i - 1] + dt
        live = t < T[..., None]
        counts = live.sum(axis=-1)
        margins["sample count"] = np.min(np.abs(t - T[..., None]) / T[..., None], axis=(1, 2))
        i30 = np.arange(30, dtype=np.float64)
        fr = np.broadcast_to(i30 / 30.0, t.shape)
        fr_f = np.broadcast_to((i30.astype(np.float32) / np.float32(30.0)).astype(np.float64), t.shape)
        te = np.where(live, t, 1e-3)[..., None]                 # (B, m, 30, 1): a sample past the bound has weight 0
        dt3 = dt[..., None]
        start = np.empty((B, m))
        acc_t = t0.copy()
        for s in range(m):                                      # ((t0 + T_0) + ...) + T_{s-1}
            start[:, s] = acc_t
            acc_t = acc_t + T[:, s]
        tau = start[..., None] + te[..., 0]
        if "tau_float" in variant:
            tau = tau.astype(np.float32).astype(np.float64)
        cc, ccm, dd, ddm = (a[:, :, None, :, :] for a in (c, cm, dc, dcm))     # (B, m, 1, 3, 6)

        def poly(q, der):
            f = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0] if der == 0 else ([0, 1, 2, 3, 4, 5] if der == 1 else
                                                                 ([0, 0, 2, 6, 12, 20] if der == 2 else [0, 0, 0, 6, 24, 60]))
            if "horner" in variant:
                r = f[5] * q[..., 5]
                for j in range(4, der - 1, -1):
                    r = r * te + f[j] * q[..., j]
                return r
            return sum(f[j] * q[..., j] * te ** (j - der) for j in range(der, 6))
        pre = [poly(cc, d) for d in (0, 1, 2)]
        prem = [sum(f * ccm[..., j] * te ** (j - d) for j, f in zip(range(d, 6), fs))
                for d, fs in ((0, [1] * 6), (1, [1, 2, 3, 4, 5]), (2, [2, 6, 12, 20]))]
        jerk_t, jerk_m = poly(cc, 3), sum(f * ccm[..., j] * te ** (j - 3) for j, f in ((3, 6), (4, 24), (5, 60)))
        pdc = [sum(f * q[..., j] * te ** (j - d) for j, f in zip((3, 4, 5), fs))
               for q in (dd, ddm) for d, fs in ((0, (1, 1, 1)), (1, (3, 4, 5)), (2, (6, 12, 20)))]
        rounded = [_float_alt(pre[d], prem[d], noise=d > 0) for d in (0, 1, 2)]
        for d in range(3):
            used = live[..., None] & ((d < 2) | dyn)
            margins["float rounding"] = np.minimum(margins["float rounding"], np.min(np.where(used, rounded[d][4], np.inf), axis=(1, 2, 3)))
        h = [np.einsum("bsen,bsin->bsie", Hd, np.stack([f * te[..., 0] ** max(j - d, 0) for j, f in enumerate(fs)], axis=-1))
             for Hd in (H, Hm) for d, fs in ((0, [1] * 6), (1, [0, 1, 2, 3, 4, 5]), (2, [0, 0, 2, 6, 12, 20]))]
        Pw = p

        def terms(pos, vel, acc):
            """Every sample's contributions from its float position / velocity / acceleration on: (values, magnitudes),
            each dict(cs, ds, q (B, m, 30), g (B, m, 30, 3 axes, 6 entries)), and the lookup's dict."""
            velm = np.where(rounded[1][3], prem[1], ab(vel))     # noise: by its magnitude
            accm = np.where(rounded[2][3], prem[2], ab(acc))
            fri = fr_f if "fr_float" in variant else fr
            pd, vd, ad = pdc[0] + vel * fri[..., None], pdc[1] + acc * fri[..., None], pdc[2] + jerk_t * fri[..., None]
            pdm, vdm, adm = pdc[3] + velm * fr[..., None], pdc[4] + accm * fr[..., None], pdc[5] + jerk_m * fr[..., None]
            vn = np.sqrt(vel[..., 0] ** 2 + vel[..., 1] ** 2 + vel[..., 2] ** 2) + 1e-5
            vnm = vn + np.where(rounded[1][3], prem[1], 0.0).sum(axis=-1)
            vdot, vdotm = (vel * vd).sum(axis=-1) / vn, (velm * vdm).sum(axis=-1) / vn
            L = _lookup(field, pos, tau, boxes, variant)
            with np.errstate(over="ignore"):
                e = np.exp(-(L["dist"] - Pw["d0"]) / Pw["r"])
            ec = 1.0 + (L["dm"] + abs(Pw["d0"])) / abs(Pw["r"])
            cd, gd = Pw["alpha"] * e, -(Pw["alpha"] / Pw["r"]) * e
            cdm, gdm = ab(cd) * ec, ab(gd) * ec
            gp, gpm = (L["grad"] * pd).sum(axis=-1), (L["gm"] * pdm).sum(axis=-1)
            w30 = float(np.float32(1.0 / 30.0)) if "w30_float" in variant else 1.0 / 30.0
            cs = wc * cd * vn * dt3
            csm = ab(wc) * cdm * vnm * dt3
            ds = wc * (gd * gp * vn * dt3 + cd * vdot * dt3 + cd * vn * w30)
            dsm = ab(wc) * (gdm * gpm * vnm * dt3 + cdm * vdotm * dt3 + cdm * vnm / 30.0)
            vk = vel / vn[..., None]
            vkm = velm / vn[..., None]
            if "wv_no_eps" in variant:
                vk = vel / (vn - 1e-5 + 1e-300)[..., None]
            wp, wpm = (wc * gd * vn * dt3)[..., None] * L["grad"], (ab(wc) * gdm * vnm * dt3)[..., None] * L["gm"]
            wv, wvm = (wc * cd * dt3)[..., None] * vk, (ab(wc) * cdm * dt3)[..., None] * vkm
            wa, wam = np.zeros_like(wp), np.zeros_like(wp)
            if dyn:
                with np.errstate(over="ignore"):
                    cv = Pw["alpha_v"] * np.exp((ab(vel) - Pw["v0"]) / Pw["r_v"])
                    ca = Pw["alpha_a"] * np.exp((ab(acc) - Pw["a0"]) / Pw["r_a"])
                cvm = ab(cv) * (1.0 + (velm + abs(Pw["v0"])) / abs(Pw["r_v"]))
                cam = ab(ca) * (1.0 + (accm + abs(Pw["a0"])) / abs(Pw["r_a"]))
                sv, sa = np.sign(vel), np.sign(acc)
                S, Sm = (cv + ca).sum(axis=-1), (cvm + cam).sum(axis=-1)
                dS = (cv / Pw["r_v"] * sv * vd + ca / Pw["r_a"] * sa * ad).sum(axis=-1)
                dSm = (cvm / abs(Pw["r_v"]) * ab(sv) * vdm + cam / abs(Pw["r_a"]) * ab(sa) * adm).sum(axis=-1)
                cs = cs + S * vn * dt3
                csm = csm + Sm * vnm * dt3
                ds = ds + (dS * vn * dt3 + S * vdot * dt3 + S * vn * (1.0 / 30.0))
                dsm = dsm + (dSm * vnm * dt3 + Sm * vdotm * dt3 + Sm * vnm / 30.0)
                wv = wv + cv / Pw["r_v"] * sv * (vn * dt3)[..., None] + (S * dt3)[..., None] * vk
                wvm = wvm + cvm / abs(Pw["r_v"]) * ab(sv) * (vnm * dt3)[..., None] + (Sm * dt3)[..., None] * vkm
                wa = ca / Pw["r_a"] * sa * (vn * dt3)[..., None]
                wam = cam / abs(Pw["r_a"]) * ab(sa) * (vnm * dt3)[..., None]
            q = wc * gd * L["dtau"] * vn * dt3
            qm = ab(wc) * gdm * L["dtm"] * vnm * dt3
            ds = ds + q * (fr_f if "own_fr_float" in variant else fr)
            dsm = dsm + qm * fr
            g = wp[..., None] * h[0][..., None, :] + wv[..., None] * h[1][..., None, :] + wa[..., None] * h[2][..., None, :]
            gm = wpm[..., None] * h[3][..., None, :] + wvm[..., None] * h[4][..., None, :] + wam[..., None] * h[5][..., None, :]
            return dict(cs=cs, ds=ds, q=q, g=g), dict(cs=csm, ds=dsm, q=qm, g=gm), L

        base = [r[0] for r in rounded]
        V0, M0, L0 = terms(*base)
        A0 = {k: np.zeros_like(v) for k, v in V0.items()}
        # the float roundings and signs that may go either way: each coordinate's other value on its own
        for d in range(3):
            if d == 2 and not dyn:
                continue
            f, flagged, alt, _, _ = rounded[d]
            flips = [(flagged, alt)]
            if d > 0 and dyn:
                with np.errstate(divide="ignore", invalid="ignore"):
                    sm = np.where((prem[d] > 0) & (pre[d] != 0), ab(pre[d]) / prem[d], np.inf)
                margins["sign"] = np.minimum(margins["sign"], np.min(np.where(live[..., None], sm, np.inf), axis=(1, 2, 3)))
                flips.append((sm < TIE, np.where(f != 0.0, -f, TIE * prem[d])))
            for flag, other in flips:
                flag = flag & live[..., None]
                for k in range(3):
                    if not flag[..., k].any():
                        continue
                    trial = [a.copy() for a in base]
                    trial[d][..., k] = np.where(flag[..., k], other[..., k], base[d][..., k])
                    with np.errstate(all="ignore"):
                        V1, _, _ = terms(*trial)
                    for name in A0:
                        sel = flag[..., k].reshape(flag.shape[:3] + (1,) * (V0[name].ndim - 3))
                        A0[name] = A0[name] + np.where(sel, 2.0 * ab(np.nan_to_num(V1[name] - V0[name])), 0.0)
        # a box decision within TIE of a tie: the corner's time derivative may be either box's, or none
        jump = np.where(L0["tie"], ab(wc * (-(Pw["alpha"] / Pw["r"])) * np.exp(-(L0["dist"] - Pw["d0"]) / Pw["r"]))
                        * 2.0 * L0["speed"] * dt3 * (np.sqrt((base[1] ** 2).sum(axis=-1)) + 1e-5), 0.0)
        A0["q"] = A0["q"] + jump
        A0["ds"] = A0["ds"] + jump * fr
        for name in ("marg_face", "marg_min", "marg_cell", "marg_map"):
            key = {"marg_face": "box face", "marg_min": "box argmin", "marg_cell": "cell choice", "marg_map": "in-map test"}[name]
            margins[key] = np.min(np.where(live, L0[name], np.inf), axis=(1, 2))
        lowered = (L0["lowered"] & live).any(axis=-1)
        lv = live.astype(np.float64)
        qlive = np.ones_like(lv) if "q_past_bound" in variant else lv
        for D, S_ in ((val, V0), (mag, M0), (allow, A0)):
            D["parts"][..., 1] = (S_["cs"] * lv).sum(axis=-1)
            D["parts"][..., 3] = (S_["ds"] * lv).sum(axis=-1)
            D["parts"][..., 4] = (S_["q"] * qlive).sum(axis=-1)
        seg_gx = seg_gx + (V0["g"] * lv[..., None, None]).sum(axis=2)
        seg_gxm = seg_gxm + (M0["g"] * lv[..., None, None]).sum(axis=2)
        seg_gxa = seg_gxa + (A0["g"] * lv[..., None, None]).sum(axis=2)

    for D in (val, mag, allow):
        pr = D["parts"]
        R = np.zeros(B)
        for s in range(m - 1, -1, -1):
            pr[:, s, 5] = R
            if not ("R_drops_last_q" in variant and D is val and s == m - 1):
                R = R + pr[:, s, 4]
            if "R_float" in variant and D is val:
                R = R.astype(np.float32).astype(np.float64)
        D["gt0"] = R
        D["gT"] = (pr[..., 2] + pr[..., 3]) + pr[..., 5]
        cost = np.zeros(B)
        for s in range(m):
            cost = cost + (pr[:, s, 0] + pr[:, s, 1])
        D["cost"] = cost + (1e-3 if D is not allow else 0.0)
    for D, S_ in ((val, seg_gx), (mag, seg_gxm), (allow, seg_gxa)):
        gx = np.zeros((B, 3, 3 * m - 3))
        for wp_ in range(1, m):
            gx[:, :, 3 * (wp_ - 1):3 * wp_] = S_[:, wp_ - 1, :, 3:] + S_[:, wp_, :, :3]
        D["gx"] = gx.reshape(B, -1)
    return dict(val=val, mag=mag, allow=allow, margins=margins, lowered=lowered, counts=counts)


ENTRIES = ("cost", "gT", "parts", "gt0", "gx")


def ratios(got, ref, kappa_u=U64):
    """Per entry kind: max over the finite entries of max(|got - ref| - allowance, 0) / (u * magnitude) as an array of
    the entry's shape (inf where the reference is finite and `got` is not; 0 where the magnitude is 0 and the values
    agree).  got: dict with any of ENTRIES."""
    out = {}
    for k in ENTRIES:
        if got.get(k) is None:
            continue
        g = np.asarray(got[k], dtype=np.float64)
        v, mg, al = ref["val"][k], ref["mag"][k], ref["allow"][k]
        if k == "parts" and g.shape[-1] < 6:
            v, mg, al = v[..., :g.shape[-1]], mg[..., :g.shape[-1]], al[..., :g.shape[-1]]
        fin = np.isfinite(v) & np.isfinite(mg) & np.isfinite(al)
        with np.errstate(divide="ignore", invalid="ignore"):
            ex = np.maximum(np.abs(g - v) - al, 0.0)
            r = np.where(ex == 0.0, 0.0, ex / (kappa_u * mg))
        r = np.where(fin, np.where(np.isfinite(g), r, np.inf), np.nan)
        out[k] = r
    return out


def allowance_share(ref, kappa, entries=ENTRIES):
    """Share of the (row, entry) pairs whose allowance is larger than kappa * u * magnitude."""
    big = tot = 0
    for k in entries:
        mg, al = ref["mag"][k], ref["allow"][k]
        fin = np.isfinite(mg) & np.isfinite(al)
        big += int(np.sum(al[fin] > kappa * U64 * mg[fin]))
        tot += int(fin.sum())
    return big / max(tot, 1)
