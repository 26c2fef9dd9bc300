"""tests/time_entry_ref.py — the time pass with rounding-error magnitudes, what tests/test_gpu_time_entrywise.py holds
the kernels of csrc/gtop_time_pass.h to on every row — is sound and sharp, on the CPU, against the pass restated in
40-digit arithmetic (mpmath).

    |entry - exact| <= KAPPA * u64 * magnitude + allowance        for the cost, every gT_s, every parts column, gt0,
                                                                  every gx entry

Sound: the reference itself and the three numpy twins (tests/time_twin.py, tests/time_moving_twin.py,
tests/joint_twin.py) are within the bound of the exact values on every case.  Sharp: deliberately wrong variants of the
reference (time_entry_ref.WRONG, at least three per family gT / MOV / GX) and the twins' own MUTANTS leave it, while each
variant stays within the 1e-5 of the max-norm that the suite's twin comparisons ask (shown per variant); a pure change of
rounding (Horner for powers, * 1 / T^3 for / T^3) stays inside.

The exact evaluation shares no formula with the closed forms: c = A_s^-1 d from the exact inverse of the segment's
Hermite matrix, c' = -A_s^-1 A_s' c from A c = d, the table d c / d d as the columns of A_s^-1, the jerk term c'Qc with
Q' entry by entry.  Sample times are the reference's doubles (t += dt; the count held fixed), d t_i / d T = i / 30,
tau = t0 + T_0 + ... + t summed exactly; positions, velocities and accelerations are rounded to float from their exact
values; the lookup, the boxes (faces, distances, their time derivatives), exp and sqrt are in 40 digits.

KAPPA, counted along the longest chain as tests/test_gpu_entrywise.py counts the evaluation's 620 u (not from a run):
  * the evaluation's chain is all here: closed-form coefficients (1 / T, its powers as products, P / V / A), the sample
    polynomial, the lookup, penalty_exp (240 u, the largest single term), sqrt, the sample times (150 u) — 620 u for two
    implementations together;
  * c' adds to a coefficient's ~12 roundings the three of (...) * iT^n, the product n c_n iT and the subtraction: +5 per
    coefficient, carried by the magnitude (...) T^-n + n |c_n| / T; pd / vd / ad are three-term polynomials in c' plus
    vel * fr: 8 roundings, and fr = i / 30 itself (1 u);
  * the per-sample products of ds (gd gp vn dt + cd vdot dt + cd vn / 30, the dyn block, w * fri): ~15 roundings on top
    of the exp's;
  * the 32-lane butterfly: 5 additions per value where the twins add 30 in sequence: <= 30 u deterministic, sqrt(30)
    in practice;
  * q_s and R_s: R_0 sums up to 226 q's, each a sum of 30: 226 + 30 roundings at worst for same-signed terms, sqrt of
    that (16) in practice — the sums' magnitudes are sums of the terms' magnitudes, so the worst case stays 256 u;
  * the 18-way spread: the same five additions per value as the butterfly, then the jerk chain (2 ws q_n times three
    table values: 8 roundings) and the two parts of a waypoint: +2.
  Together 620 + 5 + 9 + 15 + 30 + 256 + 10 ~ 945 u worst case for two implementations: KAPPA64 = 2^12 still leaves a
  factor of four, so KAPPA stays 2^12 for these tests.

Output (pytest -s): per family the largest ratio of the reference and of each twin against 40 digits, every variant's
ratio, every GPU case's allowance share."""
import math

import mpmath
import numpy as np
import pytest

from tests import joint_twin as jt
from tests import test_entrywise_bound as eb
from tests import time_entry_cases as cases
from tests import time_entry_ref as ref
from tests import time_moving_twin as tm
from tests import time_twin as tt

U64 = ref.U64
KAPPA = 2 ** 12
ALLOWANCE_CAP = 0.05
TOL_TODAY = 1e-5
M = mpmath.mpf


def _fl(v):
    return M(float(np.float32(float(v))))


def _exact_lookup(F, pos, tau, boxes):
    """evaluateEDTWithGrad(pos, tau) and d dist / d tau in the working precision -> (dist, grad[3], dtau, lowered)."""
    lo = [float(v) + 1e-4 for v in F.min_range]          # (the reference's doubles)
    hi = [float(v) - 1e-4 for v in F.max_range]
    if any(pos[a] < lo[a] or pos[a] > hi[a] for a in range(3)):
        return M(-1), [M(0)] * 3, M(0), False
    res, org = M(F.res), [M(float(v)) for v in F.origin]
    idx = [int(mpmath.floor((pos[a] - res / 2 - org[a]) / res)) for a in range(3)]
    df = [(pos[a] - ((idx[a] + M(0.5)) * res + org[a])) / res for a in range(3)]
    v, d, lowered = {}, {}, False
    for c in [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]:
        ii = [min(max(idx[a] + c[a], 0), int(F.grid[a]) - 1) for a in range(3)]
        v[c], d[c] = M(float(F.dist[ii[0], ii[1], ii[2]])), M(0)
    if boxes is not None and tau >= 0:
        scale = np.asarray(boxes["scale"], float).reshape(-1, 3)
        for b in range(len(scale)):
            cen, cv = [], []
            for a in range(3):
                if boxes.get("coef") is not None:
                    cf = [M(float(q)) for q in np.asarray(boxes["coef"], float).reshape(-1, 3, 6)[b, a]]
                    t1, t2 = M("-inf"), M("inf")
                    if boxes.get("t_range") is not None:
                        t1, t2 = (M(float(q)) for q in np.asarray(boxes["t_range"], float).reshape(-1, 2)[b])
                    tc = min(max(tau, t1), t2)
                    cen.append(sum(cf[j] * tc ** j for j in range(6)))
                    cv.append(sum(j * cf[j] * tc ** (j - 1) for j in range(1, 6)) if t1 < tau < t2 else M(0))
                else:
                    cen.append(M(float(boxes["p0"][b][a])) + M(float(boxes["vel"][b][a])) * tau)
                    cv.append(M(float(boxes["vel"][b][a])))
            d1, e1 = {}, {}
            for a in range(3):
                h = M(float(scale[b, a])) / 2
                bmin, bmax = cen[a] - h, cen[a] + h
                for o in (0, 1):
                    pt = (idx[a] + o + M(0.5)) * res + org[a]
                    if pt < bmin:
                        d1[a, o], e1[a, o] = bmin - pt, cv[a]
                    elif pt > bmax:
                        d1[a, o], e1[a, o] = pt - bmax, -cv[a]
                    else:
                        d1[a, o], e1[a, o] = M(0), M(0)
            for c in v:
                d2 = mpmath.sqrt(sum(d1[a, c[a]] ** 2 for a in range(3)))
                if d2 < v[c]:
                    v[c], lowered = d2, True
                    d[c] = sum(d1[a, c[a]] * e1[a, c[a]] for a in range(3)) / d2 if d2 > 0 else M(0)
    w = [(1 - df[a], df[a]) for a in range(3)]
    dist = sum(w[0][c[0]] * w[1][c[1]] * w[2][c[2]] * v[c] for c in v)
    dtau = sum(w[0][c[0]] * w[1][c[1]] * w[2][c[2]] * d[c] for c in v)
    grad = []
    for a in range(3):
        o1, o2 = (a + 1) % 3, (a + 2) % 3
        g = M(0)
        for c in v:
            if c[a] == 0:
                c1 = tuple(1 if k == a else c[k] for k in range(3))
                g += w[o1][c[o1]] * w[o2][c[o2]] * (v[c1] - v[c])
        grad.append(g / res)
    return dist, grad, dtau, lowered


def exact_pass(T, Df, x, F, p, t0=0.0, boxes=None):
    """The pass on one row in 40-digit arithmetic (see the module docstring) -> dict of float arrays."""
    with mpmath.workdps(40):
        m = len(T)
        w = tt.waypoint_rows(Df, x, m)
        ws = M(0.0 if p["step"] == 1 else p["ws"])
        wc = M(p["wc"])
        dyn = bool(p.get("enable_dyn", 0)) and p["step"] == 2
        colli = not abs(p["wc"]) < 1e-4
        parts = [[M(0)] * 6 for _ in range(m)]
        seg = [[[M(0)] * 6 for _ in range(3)] for _ in range(m)]       # [s][axis][entry p0 v0 a0 pT vT aT]
        start = M(float(t0))
        lowered = [False] * m
        for s in range(m):
            Ts = M(float(T[s]))
            A, dA = mpmath.zeros(6, 6), mpmath.zeros(6, 6)
            for i in range(3):
                A[2 * i, i] = math.factorial(i)
                for j in range(i, 6):
                    f = math.factorial(j) // math.factorial(j - i)
                    A[2 * i + 1, j] = f * Ts ** (j - i)
                    dA[2 * i + 1, j] = f * (j - i) * Ts ** (j - i - 1) if j > i else 0
            Ai = mpmath.inverse(A)
            Q = [[(i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2) // (i + j - 5)) * Ts ** (i + j - 5) if i >= 3 and j >= 3
                  else M(0) for j in range(6)] for i in range(6)]
            dQ = [[(i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2)) * Ts ** (i + j - 6) if i >= 3 and j >= 3 else M(0)
                   for j in range(6)] for i in range(6)]
            # local rows of A: p(0), p(T), v(0), v(T), a(0), a(T); entry e = (p0, v0, a0, pT, vT, aT) -> row
            row_of = [0, 2, 4, 1, 3, 5]
            c, dc = [], []
            for a in range(3):
                d = [M(0)] * 6
                for e in range(6):
                    d[row_of[e]] = M(float(w[s + e // 3][a][e % 3]))
                ca = [sum(Ai[i, r] * d[r] for r in range(6)) for i in range(6)]
                Ac = [sum(dA[r, j] * ca[j] for j in range(6)) for r in range(6)]
                c.append(ca)
                dc.append([-sum(Ai[i, r] * Ac[r] for r in range(6)) for i in range(6)])
            H = [[Ai[n, row_of[e]] for n in range(6)] for e in range(6)]      # H[e][n] = d c_n / d entry e
            J = dJ = M(0)
            for a in range(3):
                qc = [sum(Q[i][j] * c[a][j] for j in range(6)) for i in range(6)]
                J += sum(c[a][i] * qc[i] for i in range(6))
                dJ += sum(c[a][i] * dQ[i][j] * c[a][j] for i in range(6) for j in range(6))
                dJ += 2 * sum(qc[i] * dc[a][i] for i in range(6))
                for e in range(6):
                    seg[s][a][e] += ws * 2 * sum(qc[n] * H[e][n] for n in range(6))
            parts[s][0], parts[s][2] = ws * J, ws * dJ
            if colli:
                dt_d, dt = float(T[s]) / 30.0, Ts / 30
                t, i = 1e-3, 0
                while t < float(T[s]):
                    tm_ = M(t)
                    fr = M(i) / 30
                    P0 = [tm_ ** j for j in range(6)]
                    P1 = [j * tm_ ** (j - 1) if j else M(0) for j in range(6)]
                    P2 = [j * (j - 1) * tm_ ** (j - 2) if j >= 2 else M(0) for j in range(6)]
                    P3 = [j * (j - 1) * (j - 2) * tm_ ** (j - 3) if j >= 3 else M(0) for j in range(6)]
                    dot = lambda q, Pw: sum(q[j] * Pw[j] for j in range(6))
                    pos = [_fl(dot(c[a], P0)) for a in range(3)]
                    vel = [_fl(dot(c[a], P1)) for a in range(3)]
                    acc = [_fl(dot(c[a], P2)) for a in range(3)]
                    pd = [dot(dc[a], P0) + vel[a] * fr for a in range(3)]
                    vd = [dot(dc[a], P1) + acc[a] * fr for a in range(3)]
                    ad = [dot(dc[a], P2) + dot(c[a], P3) * fr for a in range(3)]
                    vn = mpmath.sqrt(sum(v * v for v in vel)) + M(1e-5)
                    vdot = sum(vel[a] * vd[a] for a in range(3)) / vn
                    dist, g, dtau, low = _exact_lookup(F, pos, start + tm_, boxes)
                    lowered[s] |= low
                    e_ = mpmath.exp(-(dist - M(p["d0"])) / M(p["r"]))
                    cd, gd = M(p["alpha"]) * e_, -(M(p["alpha"]) / M(p["r"])) * e_
                    gp = sum(g[a] * pd[a] for a in range(3))
                    parts[s][1] += wc * cd * vn * dt
                    parts[s][3] += wc * (gd * gp * vn * dt + cd * vdot * dt + cd * vn / 30)
                    q = wc * gd * dtau * vn * dt
                    parts[s][3] += q * fr
                    parts[s][4] += q
                    wp = [wc * gd * vn * dt * g[a] for a in range(3)]
                    wv = [wc * cd * dt * vel[a] / vn for a in range(3)]
                    wa = [M(0)] * 3
                    if dyn:
                        cv = [M(p["alpha_v"]) * mpmath.exp((abs(vel[a]) - M(p["v0"])) / M(p["r_v"])) for a in range(3)]
                        ca_ = [M(p["alpha_a"]) * mpmath.exp((abs(acc[a]) - M(p["a0"])) / M(p["r_a"])) for a in range(3)]
                        S = sum(cv) + sum(ca_)
                        dS = sum(cv[a] / M(p["r_v"]) * mpmath.sign(vel[a]) * vd[a]
                                 + ca_[a] / M(p["r_a"]) * mpmath.sign(acc[a]) * ad[a] for a in range(3))
                        parts[s][1] += S * vn * dt
                        parts[s][3] += dS * vn * dt + S * vdot * dt + S * vn / 30
                        for a in range(3):
                            wv[a] += cv[a] / M(p["r_v"]) * mpmath.sign(vel[a]) * vn * dt + S * vel[a] / vn * dt
                            wa[a] = ca_[a] / M(p["r_a"]) * mpmath.sign(acc[a]) * vn * dt
                    for e in range(6):
                        h0, h1, h2 = dot(H[e], P0), dot(H[e], P1), dot(H[e], P2)
                        for a in range(3):
                            seg[s][a][e] += wp[a] * h0 + wv[a] * h1 + wa[a] * h2
                    t += dt_d
                    i += 1
            start += Ts
        R = M(0)
        for s in range(m - 1, -1, -1):
            parts[s][5] = R
            R += parts[s][4]
        cost = sum(parts[s][0] + parts[s][1] for s in range(m)) + M(1e-3)
        gx = np.zeros((3, 3 * m - 3))
        for wp_ in range(1, m):
            for a in range(3):
                for j in range(3):
                    gx[a, 3 * (wp_ - 1) + j] = float(seg[wp_ - 1][a][3 + j] + seg[wp_][a][j])
        pr = np.array([[float(v) for v in row] for row in parts])
        gT = np.array([float(parts[s][2] + parts[s][3] + parts[s][5]) for s in range(m)])
        return dict(cost=np.array(float(cost)), gT=gT, parts=pr, gt0=np.array(float(R)), gx=gx.reshape(-1),
                    lowered=np.array(lowered))


# ---- the cases: (name, m, field, origin, T[0], parameters, extra) ----
DYN = dict(enable_dyn=1, alpha_v=2.0, r_v=4.0, alpha_a=1.5, r_a=15.0)       # tests/test_gpu_time.py's block
CPU_CASES = [
    ("plain m2", 2, "random", (0.0, 0.0, 0.0), 0.7, {}, {}),
    ("dyn m3", 3, "random", (-1.0, -1.5, 0.0), 0.5, DYN, {}),
    ("dyn step1 m5", 5, "random", (0.0, 0.0, 0.0), 0.5, dict(DYN, step=1), {}),
    ("ws0 m3 signed", 3, "signed", (0.0, 0.0, 0.0), 0.6, dict(ws=0.0), {}),
    ("replay m3", 3, "random", (0.0, 0.0, 0.0), 0.02, {}, {}),
    ("out of map m3", 3, "random", (0.0, 0.0, 0.0), 0.5, {}, dict(outside=True)),
    ("cv1 m2", 2, "random", (0.0, 0.0, 0.0), 0.8, {}, dict(boxes=("cv", 1), t0=1.3)),
    ("cv8 dyn m5", 5, "random", (-1.0, -1.5, 0.0), 0.5, DYN, dict(boxes=("cv", 8), t0=0.9)),
    ("poly1 m3", 3, "constant", (0.0, 0.0, 0.0), 0.5, dict(step=1), dict(boxes=("poly", 1), t0=0.4)),
    ("poly8 m3 interval", 3, "random", (0.0, 0.0, 0.0), 0.5, {}, dict(boxes=("poly", 8), t0=1.1)),
    ("cv8 m3 tau<0 replay", 3, "random", (0.0, 0.0, 0.0), 0.02, dict(ws=0.0), dict(boxes=("cv", 8), t0=-0.3)),
    ("cv8 m3 replay", 3, "random", (0.0, 0.0, 0.0), 0.02, {}, dict(boxes=("cv", 8), t0=0.7)),
    ("poly8 m5 signed", 5, "signed", (0.0, 0.0, 0.0), 0.5, dict(ws=0.0), dict(boxes=("poly", 8), t0=0.5)),
]


def _build(j, case, oracle_mod):
    name, m, kind, origin, T0, kw, extra = case
    (org, res, grid, dist), T, Df, x = eb._case(m, kind, origin, T0, seed=130 + j, rows=1)
    if extra.get("outside"):
        xs = x.reshape(1, 3, -1).copy()
        xs[0, 2, 0] = org[2] + grid[2] * res + 1.5          # waypoint 1: z above the map
        x = xs.reshape(1, -1)
    t0 = extra.get("t0", 0.0)
    boxes = eb._boxes(*extra["boxes"], T, Df, x, t0, seed=160 + j) if "boxes" in extra else None
    if boxes is not None:      # (the map is 3.5 m wide: boxes of 0.3 .. 0.6 m leave corners outside them, where d / d tau lives)
        boxes["scale"] = boxes["scale"] * 0.3
    p = dict(oracle_mod.OPTI_NODE_PARAMS)
    p.update(kw)
    F = ref.Field(org, res, grid, dist)
    osdf = oracle_mod.Sdf(org, res, grid, dist.reshape(-1))
    return dict(name=name, m=m, T=T, Df=Df, x=x, p=p, F=F, osdf=osdf, t0=t0, boxes=boxes)


@pytest.fixture(scope="module")
def evaluated(oracle_mod):
    out = []
    for j, case in enumerate(CPU_CASES):
        ev = _build(j, case, oracle_mod)
        ev["ref"] = ref.reference(ev["T"], ev["Df"], ev["x"], ev["F"], ev["p"], t0=ev["t0"], boxes=ev["boxes"])
        ev["exact"] = exact_pass(ev["T"][0], ev["Df"][0], ev["x"][0], ev["F"], ev["p"], ev["t0"], ev["boxes"])
        out.append(ev)
    return out


def _worst(got, ev, keys=ref.ENTRIES):
    """Largest ratio per entry kind of `got` (dict of row-0 arrays) against the exact values, in the reference's units."""
    exact = dict(val={k: np.asarray(ev["exact"][k])[None] for k in ref.ENTRIES},
                 mag={k: ev["ref"]["mag"][k][:1] for k in ref.ENTRIES},
                 allow={k: ev["ref"]["allow"][k][:1] for k in ref.ENTRIES})
    r = ref.ratios({k: np.asarray(got[k])[None] for k in keys if got.get(k) is not None}, exact)
    return {k: float(np.nanmax(v)) for k, v in r.items()}


def _row(d):
    return {k: d[k][0] for k in ref.ENTRIES}


def _twin_lookup(ev, mutant=None):
    bx = ev["boxes"]
    if bx is None:
        return tm.StaticLookup(ev["osdf"])
    if "coef" in bx:
        return tm.PolyBoxLookup(ev["osdf"], bx["coef"], bx["scale"], bx["t_range"], mutant=mutant)
    return tm.BoxLookup(ev["osdf"], bx["p0"], bx["vel"], bx["scale"], mutant=mutant)


def _twins(ev, mutant=None):
    """name -> the twin's entries on row 0.  mutant: (twin name, its mutant) or None."""
    T, Df, x, p = ev["T"][0], ev["Df"][0], ev["x"][0], ev["p"]
    mt = lambda name: mutant[1] if mutant and mutant[0] == name else None
    out = {}
    if ev["boxes"] is None and ev["t0"] == 0.0:
        if mutant is None or mutant[0] == "time_twin":
            c, gT, parts = tt.cost_gradT(T, Df, x, ev["osdf"], p, mutant=mt("time_twin"))
            out["time_twin"] = dict(cost=c, gT=gT, parts=parts)
        if mutant is None or mutant[0] == "joint_twin":
            c, gx, gT, parts = jt.cost_grad(T, Df, x, ev["osdf"], p, mutant=mt("joint_twin"))
            out["joint_twin"] = dict(cost=c, gx=gx, gT=gT, parts=parts)
    if mutant is None or mutant[0] == "time_moving_twin":
        m_ = mt("time_moving_twin")
        look = _twin_lookup(ev, m_ if m_ in tm.LOOKUP_MUTANTS else None)
        c, gT, gt0, parts, _ = tm.cost_gradT(T, Df, x, look, p, ev["t0"], mutant=m_ if m_ in tm.PASS_MUTANTS else None)
        out["time_moving_twin"] = dict(cost=c, gT=gT, gt0=gt0, parts=parts)
    return out


def test_the_cases_cover_what_they_name(evaluated):
    by = {ev["name"]: ev for ev in evaluated}
    assert by["replay m3"]["ref"]["counts"][0, 0] == 29
    assert by["cv8 m3 tau<0 replay"]["ref"]["counts"][0, 0] == 29
    for name in ("cv1 m2", "cv8 dyn m5", "poly1 m3", "poly8 m3 interval", "cv8 m3 tau<0 replay", "poly8 m5 signed"):
        ev = by[name]
        assert ev["ref"]["lowered"].any() and np.array_equal(ev["ref"]["lowered"][0], ev["exact"]["lowered"]), name
        assert np.any(ev["exact"]["parts"][:, 4] != 0.0), name
    ev = by["cv8 m3 tau<0 replay"]                       # the first samples are before the boxes' clock starts
    assert ev["t0"] + 1e-3 < 0.0 < ev["t0"] + ev["T"][0].sum()
    ev = by["poly8 m3 interval"]                          # a validity interval ends inside the trajectory
    t2 = ev["boxes"]["t_range"][:, 1]
    assert np.any((t2 > ev["t0"]) & (t2 < ev["t0"] + ev["T"][0].sum()))
    ev = by["out of map m3"]                              # samples of the two segments at waypoint 1 leave the map
    assert np.any(ev["exact"]["parts"][:2, 1] > 0.0) and np.isfinite(ev["exact"]["gx"]).all()
    assert (by["ws0 m3 signed"]["F"].dist < 0).any()
    for ev in evaluated:                                   # no decision of these rows is within TIE of its threshold
        assert ev["ref"]["margins"]["sample count"][0] > ref.TIE, ev["name"]
        for k in ref.ENTRIES:
            assert np.all(ev["ref"]["mag"][k] >= np.abs(ev["ref"]["val"][k])), (ev["name"], k)


def test_the_bound_holds_for_the_reference_and_the_twins(evaluated):
    worst = {}
    for ev in evaluated:
        impls = dict(reference=_row(ev["ref"]["val"]), **_twins(ev))
        for name, got in impls.items():
            r = _worst(got, ev)
            fam = "MOV" if ev["boxes"] is not None else "gT / GX"
            for k, v in r.items():
                key = (fam, name, k)
                worst[key] = max(worst.get(key, 0.0), v)
                assert v <= KAPPA, (ev["name"], name, k, v)
    for key in sorted(worst):
        print(f"TIME ENTRYWISE {key[0]:8s} {key[1]:17s} {key[2]:6s}: largest |err| / (u * mag) against 40 digits {worst[key]:.3g}")
    assert max(worst.values()) > 0          # (the comparison is not vacuous)


FAMILY_ENTRIES = {"gT": ("cost", "gT", "parts"), "MOV": ("cost", "gT", "parts", "gt0"), "GX": ("gx",)}


def _today(got, base):
    """What the suite's 1e-5 checks look at: the cost relatively, gT / gt0 / gx / parts by the row's max-norm, and every
    parts column by its own max-norm (tests/test_gpu_time_moving.py) -> the largest of them."""
    out = [abs(got["cost"] - base["cost"]) / abs(base["cost"])]
    for k in ("gT", "gx", "parts"):
        out.append(np.max(np.abs(got[k] - base[k])) / max(np.max(np.abs(base[k])), 1e-300))
    out.append(abs(got["gt0"] - base["gt0"]) / max(abs(base["gt0"]), np.max(np.abs(base["gT"]))))
    for col in range(6):
        den = np.max(np.abs(base["parts"][:, col]))
        if den > 0:
            out.append(np.max(np.abs(got["parts"][:, col] - base["parts"][:, col])) / den)
    return float(max(out))


@pytest.mark.parametrize("family,variant", [(f, v) for f, vs in ref.WRONG.items() for v in vs])
def test_the_bound_catches_wrong_variants(evaluated, family, variant):
    """Each wrong line stays within today's 1e-5 on every case and leaves the bound on at least one."""
    worst = today = 0.0
    for ev in evaluated:
        if family == "MOV" and ev["boxes"] is None:
            continue
        got = _row(ref.reference(ev["T"], ev["Df"], ev["x"], ev["F"], ev["p"], t0=ev["t0"], boxes=ev["boxes"],
                                 variant=(variant,))["val"])
        today = max(today, _today(got, _row(ev["ref"]["val"])))
        worst = max(worst, *_worst(got, ev, FAMILY_ENTRIES[family]).values())
    print(f"TIME ENTRYWISE wrong {family:4s} {variant:18s}: off today's criterion by {today:.2e} (1e-5 passes); "
          f"largest |err| / (u * mag) {worst:.3g} (KAPPA {KAPPA})")
    assert today <= TOL_TODAY, (variant, today)
    assert worst > KAPPA, (variant, worst)


@pytest.mark.parametrize("variant", ref.OTHER)
def test_wrong_variants_outside_the_gap(evaluated, variant):
    """The issue's other candidates, recorded: R_s without the last segment's q, q_s counting a sample past the loop
    bound and the swapped acceleration parts in the jerk term are off today's 1e-5 criterion already (1.0, 6.8e-4 and
    5.4e-2 of a column's max-norm on these cases) and far outside the bound; the own term's i / 30 formed in float
    (6e-8 relative on a term that is itself small beside [3]) stays inside both (largest ratio 598 of 4096)."""
    worst = today = 0.0
    for ev in evaluated:
        got = _row(ref.reference(ev["T"], ev["Df"], ev["x"], ev["F"], ev["p"], t0=ev["t0"], boxes=ev["boxes"],
                                 variant=(variant,))["val"])
        today = max(today, _today(got, _row(ev["ref"]["val"])))
        worst = max(worst, *_worst(got, ev).values())
    print(f"TIME ENTRYWISE other {variant:18s}: off today's criterion by {today:.2e}; largest |err| / (u * mag) {worst:.3g}")
    assert (today > TOL_TODAY and worst > KAPPA) or (today <= TOL_TODAY and worst <= KAPPA), (variant, today, worst)


TWIN_MUTANTS = ([("time_twin", mu) for mu in tt.MUTANTS] + [("time_moving_twin", mu) for mu in tm.MUTANTS]
                + [("joint_twin", mu) for mu in jt.MUTANTS if mu != "no_rho"])     # (no_rho is in F, not in the pass)


@pytest.mark.parametrize("twin,mutant", TWIN_MUTANTS)
def test_the_bound_catches_the_twins_own_mutants(evaluated, twin, mutant):
    worst = 0.0
    for ev in evaluated:
        if twin == "time_moving_twin" and ev["boxes"] is None:
            continue
        if mutant == "no_interval_zero" and (ev["boxes"] is None or "coef" not in ev["boxes"]):
            continue
        for got in _twins(ev, (twin, mutant)).values():
            worst = max(worst, *_worst(got, ev).values())
    print(f"TIME ENTRYWISE mutant {twin} {mutant}: largest |err| / (u * mag) {worst:.3g}")
    assert worst > KAPPA, (twin, mutant, worst)


@pytest.mark.parametrize("variant", ref.ROUNDING)
def test_a_change_of_rounding_stays_within_the_bound(evaluated, variant):
    worst, differs = 0.0, 0
    for ev in evaluated:
        got = _row(ref.reference(ev["T"], ev["Df"], ev["x"], ev["F"], ev["p"], t0=ev["t0"], boxes=ev["boxes"],
                                 variant=(variant,))["val"])
        differs += any(not np.array_equal(got[k], ev["ref"]["val"][k][0]) for k in ref.ENTRIES)
        worst = max(worst, *_worst(got, ev).values())
    print(f"TIME ENTRYWISE rounding only {variant}: largest |err| / (u * mag) {worst:.3g}")
    assert differs >= 1 and worst <= KAPPA, (variant, worst)


@pytest.fixture(scope="module")
def maps(oracle_mod):
    return cases.Maps(oracle_mod)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_cases_do_not_rest_on_their_allowances(maps, name):
    """From the reference alone: at most ALLOWANCE_CAP of a GPU case's (row, entry) pairs carry an allowance above
    KAPPA * u * magnitude; a moving case lowers a corner in a later segment on a quarter of its rows and has a live
    R_s; every row's sample count is away from its threshold."""
    case = cases.build(maps, name)
    r = case["ref"]
    share = ref.allowance_share(r, KAPPA, case["entries"])
    later = r["lowered"][:, 1:].any(axis=1).mean()
    gT, R = r["val"]["gT"], r["val"]["parts"][..., 5]
    live = np.max(np.abs(R)) / np.max(np.abs(gT))
    print(f"TIME ENTRYWISE case {name}: rows {len(gT)}, allowance share {share:.4f}, rows lowered in a later segment "
          f"{later:.2f}, max |R_s| / max |gT| {live:.2e}, smallest margins "
          + ", ".join(f"{k} {v.min():.1e}" for k, v in r["margins"].items() if np.isfinite(v.min())))
    assert share <= ALLOWANCE_CAP, (name, share)
    assert np.all(r["margins"]["sample count"] > ref.TIE), name
    if case["boxes"] is not None and not case.get("static_lookup"):
        assert later >= 0.25, (name, later)
        assert live >= 1e-9, (name, live)
