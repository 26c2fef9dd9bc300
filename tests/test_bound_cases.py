"""The cases of tests/bound_cases.py are DECISIVE (CPU only).

tests/test_gpu_optimizer_bounds.py holds the device optimizer to the serial algorithm on every row of these cases and
excuses none.  That is fair only if the serial road of every committed case hangs on no near-tie: a decision that two
correct evaluations of the callback (1e-9 apart at the most, tests/test_gpu_fuzz.py::test_random_draw_optimizer) could
take differently.  So, for every case and every stop rule the device test uses, the road of oracle/mma_twin.py around
the oracle callback is walked with its observers, as tests/test_gpu_fuzz.py::_narrowest_margin does, and every
comparison on it must be either an exact equality (structural: a trial point that equals the base point is evaluated
to the same bits by any one implementation) or clear of a tie by 1e-6 relative — a thousand times the callbacks'
difference.  A seed that fails is replaced in bound_cases.SEEDS; the thresholds stay."""
import functools

import numpy as np
import pytest

from tests import bound_cases

MARGIN = 1e-6          # relative margin of every decision that is not an exact equality
STEP = 1e-9            # smallest step (relative to max(1, |x|)) of a coordinate that moved in both of the last two outers
CASES = [(m, rule) for m in bound_cases.SERIAL_M for rule in bound_cases.rules_for(m)]


@functools.lru_cache(maxsize=None)
def _scene():
    from oracle import oracle
    mp = bound_cases.scene_map()
    sdf = oracle.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    return oracle, sdf, oracle.make_params()


@functools.lru_cache(maxsize=8)
def _generator(T_bytes):
    """(the oracle's generator of one row's segment times: a dense inverse, a second at 118 segments)"""
    return _scene()[0].generator(np.frombuffer(T_bytes, dtype=np.float64))


def serial_road(T, Df, x0, lb, ub, evals, rule):
    """One row through oracle/mma_twin.py around the oracle callback.  Returns the twin's result and what the road
    hung on: `margin` (the narrowest relative margin of a decision that was not an exact equality, and which decision),
    `step` (the smallest step of a coordinate that moved in both of the last two outer iterations), `rejected` (inner
    evaluations whose step was rejected: rho grew)."""
    from oracle import mma_twin
    oracle, sdf, prm = _scene()
    gen = _generator(np.ascontiguousarray(T, dtype=np.float64).tobytes())
    info = dict(margin=np.inf, what=None, step=np.inf, rejected=0)
    evs = []                                                  # (xcur, fcur, inner_done) of every inner evaluation

    def note(v, what):
        if v < info["margin"]:
            info.update(margin=float(v), what=what)

    def observe(xcur, fcur, g, fbest):
        assert np.isfinite(fcur) and np.isfinite(g)
        if g != fcur:
            note(abs(g - fcur) / abs(fcur), "inner-loop test g >= f")
        if fcur != fbest:
            note(abs(fcur - fbest) / abs(fbest), "acceptance f < fbest")
        info["rejected"] += int(fcur > g)
        evs.append((xcur.copy(), fcur, g >= fcur))

    def observe_outer(xcur, xprev, xprevprev):
        a, b = np.abs(xcur - xprev), np.abs(xprev - xprevprev)
        moving = (a > 0) & (b > 0)
        if moving.any():
            info["step"] = min(info["step"], float(np.min((np.minimum(a, b) / np.maximum(1.0, np.abs(xcur)))[moving])))

    def f(x):
        return oracle.cost_grad(T, Df, x, sdf, prm, L=gen["L"], R=gen["R"])

    r = mma_twin.minimize(f, x0, lb, ub, evals, observe=observe, observe_outer=observe_outer, **rule)
    assert np.all(np.isfinite(r["fs"])) and np.all(np.isfinite(r["xs"]))
    # the stop rules' own comparisons (stop.c relstop, at the end of every outer iteration that is not the capped
    # evaluation): |new - old| against tol (|new| + |old|) / 2 — f alone, x as the all() over the coordinates
    ftol, xtol = rule.get("ftol_rel", 0.0), rule.get("xtol_rel", 0.0)
    xprev, fprev = r["xs"][0], r["fs"][0]
    for i, (xcur, fcur, done) in enumerate(evs):
        if not done or i + 2 >= evals:                        # (evaluation i + 2 of the run; the cap is looked at first)
            continue
        if ftol > 0 and fcur != fprev:
            note(abs(abs(fcur - fprev) / (ftol * (abs(fcur) + abs(fprev)) * 0.5) - 1.0), "ftol_rel test")
        if xtol > 0:
            moved = xcur != xprev
            if moved.any():
                ratio = np.abs(xcur - xprev)[moved] / (xtol * (np.abs(xcur) + np.abs(xprev))[moved] * 0.5)
                note(abs(float(np.max(ratio)) - 1.0), "xtol_rel test")
        xprev, fprev = xcur, fcur
    return r, info


@functools.lru_cache(maxsize=None)
def roads(m, rule_name):
    T, Df, x0, lb, ub, kinds = bound_cases.build(m)
    rule = bound_cases.rules_for(m)[rule_name]
    evals = bound_cases.evals_for(m)
    return (T, Df, x0, lb, ub, kinds), [serial_road(T[i], Df[i], x0[i], lb[i], ub[i], evals, rule)
                                         for i in range(len(kinds))]


@pytest.mark.parametrize("m,rule", CASES)
def test_no_decision_of_the_serial_road_is_a_near_tie(m, rule):
    (_, _, _, _, _, kinds), rs = roads(m, rule)
    for kind, (r, info) in zip(kinds, rs):
        assert info["margin"] >= MARGIN, (m, rule, kind, info)
        assert info["step"] >= STEP, (m, rule, kind, info)


@pytest.mark.parametrize("m,rule", CASES)
def test_the_product_header_walks_the_same_road(m, rule):
    """csrc/mma.hpp (oracle.mma_trace) against the twin: point, value, count and code to 1e-12; every point in its box."""
    oracle, sdf, prm = _scene()
    (T, Df, x0, lb, ub, kinds), rs = roads(m, rule)
    for i, (kind, (r, _)) in enumerate(zip(kinds, rs)):
        h = oracle.mma_trace(T[i], Df[i], x0[i], lb[i], ub[i], sdf, prm, bound_cases.evals_for(m),
                             **bound_cases.rules_for(m)[rule])
        what = (m, rule, kind)
        assert (h["nevals"], h["code"]) == (r["nevals"], r["code"]), what
        assert np.all(np.isfinite(h["fs"])), what
        assert abs(h["minf"] - r["minf"]) <= 1e-12 * abs(r["minf"]), what
        scale = max(1.0, float(np.max(np.abs(r["x"]))))
        assert np.max(np.abs(h["x"] - r["x"])) <= 1e-12 * scale, what
        assert np.max(np.abs(h["xs"] - r["xs"])) <= 1e-12 * max(1.0, float(np.max(np.abs(r["xs"])))), what
        assert np.max(np.abs(h["fs"] - r["fs"]) / np.abs(r["fs"])) <= 1e-12, what
        assert np.all(h["xs"] >= lb[i]) and np.all(h["xs"] <= ub[i]), what
        assert np.all(r["xs"] >= lb[i]) and np.all(r["xs"] <= ub[i]), what


@pytest.mark.parametrize("m", bound_cases.SERIAL_M)
def test_all_fixed_stops_as_nlopt_does(m):
    """Nothing can move: two evaluations and FTOL (3) under ftol_rel, XTOL (4) under xtol_rel or both — the `new == old`
    clause of relstop — and the cap with MAXEVAL (5) when no rule is set."""
    oracle, sdf, prm = _scene()
    T, Df, x0, lb, ub, kinds = bound_cases.build(m)
    i = kinds.index("all-fixed")
    cap = bound_cases.evals_for(m)
    for rule, want in ((dict(), (cap, 5)), (dict(ftol_rel=1e-3), (2, 3)), (dict(xtol_rel=1e-3), (2, 4)),
                       (dict(ftol_rel=1e-3, xtol_rel=1e-3), (2, 4))):
        r, info = serial_road(T[i], Df[i], x0[i], lb[i], ub[i], cap, rule)
        h = oracle.mma_trace(T[i], Df[i], x0[i], lb[i], ub[i], sdf, prm, cap, **rule)
        assert (r["nevals"], r["code"]) == want == (h["nevals"], h["code"]), (m, rule)
        assert np.array_equal(r["x"], x0[i]) and np.array_equal(h["x"], x0[i])
        assert info["margin"] == np.inf                       # every comparison on this road is an exact equality


@pytest.mark.parametrize("m", bound_cases.SERIAL_M)
def test_the_cases_are_not_vacuous(m):
    on_face = rejected = 0
    for rule in bound_cases.rules_for(m):
        (_, _, x0, lb, ub, kinds), rs = roads(m, rule)
        for i, (r, info) in enumerate(rs):
            free = lb[i] < ub[i]
            on_face += int(np.any(free & np.isfinite(lb[i]) & (r["x"] == lb[i])) or
                           np.any(free & np.isfinite(ub[i]) & (r["x"] == ub[i])))
            rejected += int(info["rejected"] > 0)
    assert on_face >= 1, "no row ends with a coordinate exactly on a finite face"
    assert rejected >= 1, "no row rejected a step"


def test_an_open_coordinate_leaves_its_first_asymptotes():
    """At least one row has a coordinate with an infinite bound that moved, in total, by more than its initial
    sigma = 1: past what the first approximation's asymptotes allowed."""
    far = 0
    for m, rule in CASES:
        (_, _, x0, lb, ub, kinds), rs = roads(m, rule)
        for i, (r, _) in enumerate(rs):
            open_ = np.isinf(lb[i]) | np.isinf(ub[i])
            far += int(np.any(np.abs(r["x"] - np.clip(x0[i], lb[i], ub[i]))[open_] > 1.0))
    assert far >= 1


@pytest.mark.parametrize("m", [m for m in bound_cases.SERIAL_M if len(bound_cases.rules_for(m)) > 1])
def test_the_tolerances_stop_a_third_of_the_rows_early(m):
    for name in ("ftol", "xtol", "both"):
        _, rs = roads(m, name)
        early = sum(r["code"] in (3, 4) and r["nevals"] < bound_cases.evals_for(m) for r, _ in rs)
        assert 3 * early >= len(rs), (m, name, early)


def _recorded_plan(elem, pin, m, B):
    """(spl, nt, long) of the optimizer loop's plan in tests/golden/launch_rule.txt, None where it is refused."""
    import os
    import re
    lines = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_rule.txt")).read().splitlines()
    batches = [int(v) for v in lines[1].split(":")[1].split()]
    legend = {}
    for ln in lines:
        mt = re.match(r"# (\w) = spl (\d+) nt (\d+) long (\d) nw (\d)$", ln)
        if mt:
            legend[mt.group(1)] = tuple(int(v) for v in mt.group(2, 3, 4))
    start = lines.index(f"plan for_optimizer=1 elem={elem} pin={pin}")
    col = max(i for i, b in enumerate(batches) if b <= B)
    for ln in lines[start + 1:]:
        if not ln[0].isdigit():
            break
        span, codes = ln.split()
        lo, hi = (int(v) for v in (span.split("-") + [span])[:2])
        if lo <= m <= hi:
            return legend.get(codes[col])
    raise AssertionError((elem, pin, m))


def test_every_geometry_runs_the_body_its_name_says():
    for elem, geoms in ((8, bound_cases.GEOMETRIES), (4, bound_cases.F32_GEOMETRIES)):
        for m, pin, body, plan in geoms:
            B = len(bound_cases.KINDS if m <= 13 else bound_cases.LONG_KINDS)
            assert _recorded_plan(elem, pin, m, B) == plan, (elem, m, pin, body)
            assert _recorded_plan(elem, pin, m, 1) == plan, (elem, m, pin, body, "a row alone")
    assert {(p, body) for _, _, body, p in bound_cases.GEOMETRIES} == {
        ((3, 1, 0), "ten-lanes"), ((6, 2, 0), "two-per-wavefront"), ((6, 1, 0), "five-lanes"), ((6, 1, 1), "chunked")}
    for pin in (0, 3, 6):
        assert _recorded_plan(8, pin, 119, 3) is None          # past what one wavefront's LDS holds with the state


def test_the_builder_keeps_its_row_order():
    """Row order is part of the case (bound_cases.KINDS): `all-fixed` beside a running row, every row with an infinite
    bound beside a finite one, an odd batch."""
    T, Df, x0, lb, ub, kinds = bound_cases.build(6)
    assert len(kinds) % 2 == 1 and set(kinds) == set(bound_cases.KINDS) and len(set(kinds)) == 12
    pair = {k: kinds[i ^ 1] for i, k in enumerate(kinds[:-1])}
    assert pair["all-fixed"] not in ("all-fixed", "positions-fixed", "every-fourth-fixed")
    open_row = np.isinf(lb).any(axis=1) | np.isinf(ub).any(axis=1)
    for i in range(0, len(kinds) - 1, 2):
        assert not (open_row[i] and open_row[i + 1]), (kinds[i], kinds[i + 1])
    assert open_row[-1]                                        # the lone row of the last wavefront has open bounds
    pos = bound_cases.position_mask(x0.shape[1])
    i = kinds.index("derivatives-free")
    assert np.isfinite(lb[i][pos]).all() and np.isinf(lb[i][~pos]).all() and np.isinf(ub[i][~pos]).all()
    i = kinds.index("start-outside")
    assert np.all((x0[i] > ub[i]) | (x0[i] < lb[i]))
    i = kinds.index("start-on-faces")
    assert np.array_equal(x0[i][pos], lb[i][pos]) and np.array_equal(x0[i][~pos], ub[i][~pos])
    i = kinds.index("all-fixed")
    assert np.array_equal(lb[i], x0[i]) and np.array_equal(ub[i], x0[i])
