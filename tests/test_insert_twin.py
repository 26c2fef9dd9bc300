"""The numpy restatement of the waypoint insertion (tests/insert_twin.py), checked without a GPU:

(1) the symbols, their bindings and the ABI version;
(2) curve preservation in exact arithmetic: on rows whose fp64 inputs are exactly consistent (dyadic junction data,
    segment times that are powers of two, so the Hermite coefficients are doubles) the twin's new (p, v, a) lie within
    16 u of the exact values times their magnitudes, and — with the exact (p, v, a) and the exact times in their place
    — the coefficient rows of the m + 1 new segments, formed exactly from their end conditions, are the old rows and
    the exact Taylor shift of the one that was cut;
(3) five mutants of the restatement, each caught;
(4) a known answer that does not use the twin's arithmetic: a constant-velocity row in dyadic numbers;
(5) the binding's call records against the recording stub of tests/test_binding_args.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from grad_traj_optimization_amd import _abi, insert
from tests import insert_twin as it
from tests.test_binding_args import (B, DEFECTS, F64, HANDLE, M, STREAM, T_FORMS, FakeTensor, allocations,  # noqa: F401
                                     make_context, p, t)

U = Fraction(1, 2 ** 53)


def test_symbols_bindings_and_abi_constants(gtop):
    lib = gtop.load_library()
    assert lib.gtop_abi_version() >= 12
    assert _abi.ABI_VERSION == 12
    names = {"gtop_insert_waypoints_device", "gtop_insert_waypoints"}
    assert {n for n, (since, _, _) in _abi.ENTRY_POINTS.items() if since == 12} == names
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert all(_abi.ENTRY_POINTS[n][0] == 12 for n in names)
    assert not names & set(_abi.entry_points(11)) and set(_abi.entry_points(12)) - set(_abi.entry_points(11)) == names
    assert len(_abi.ENTRY_POINTS["gtop_insert_waypoints_device"][2]) == 18
    assert len(_abi.ENTRY_POINTS["gtop_insert_waypoints"][2]) == 12
    for name in ("insert_waypoints_device", "insert_waypoints", "GtopInsert", "INSERT_INFO"):
        assert hasattr(insert, name) and hasattr(gtop, name), name
    assert [n for n, _ in insert.GtopInsert._fields_] == ["mode", "min_fraction", "push", "push_below", "bos", "vos",
                                                          "aos", "reserved"]
    o = insert.GtopInsert()
    assert (o.mode, o.min_fraction, o.push, o.push_below, o.bos, o.vos, o.aos, o.reserved) == (1, 0.1, 0, 0, 3, 8, 10, 0)
    assert (insert.GtopInsert.AT_TIME, insert.GtopInsert.LONGEST) == (0, 1) and len(insert.INSERT_INFO) == 6


# ---- (2) curve preservation ---------------------------------------------------------------------------------------
def consistent_row(m, seed):
    """A row whose fp64 x, Df, T and coefficients are EXACTLY consistent: junction data in multiples of 2^-6, times
    in {0.5, 1, 2, 4} (A^-1 of a power of two is dyadic), so every Hermite coefficient is a double."""
    rng = np.random.default_rng(seed)
    T = rng.choice([0.5, 1.0, 2.0, 4.0], m)
    Df = rng.integers(-256, 257, 18) / 64.0
    x = rng.integers(-256, 257, 9 * (m - 1)) / 64.0
    rows = it.segment_rows_exact(m, [Fraction(v) for v in Df], [Fraction(v) for v in x], [Fraction(v) for v in T])
    coeff = np.empty((m, 3, 6))
    for (s, axis), c in rows.items():
        coeff[s, axis] = [float(v) for v in c]
        assert all(Fraction(float(v)) == v for v in c)
    return x, Df, T, coeff, rows


def curve_preservation_failures(m, seed, when, mutant=None, **kw):
    """The checks of (2) on one row -> the names of those that fail (empty: the curve is preserved)."""
    x, Df, T, coeff, old = consistent_row(m, seed)
    r = it.insert_row(m, x, coeff, T, mode=it.AT_TIME, when=when, mutant=mutant, **kw)
    s, tl = int(r["info"][0]), float(r["info"][1])
    bad = []
    if r["x_out"].shape != (9 * m,) or r["T_out"].shape != (m + 1,):
        return ["shapes"]
    s_want, tl_want = it.walk(T, np.float64(when))
    if (s, tl) != (s_want, float(tl_want)) or r["info"][3] != 0:
        bad.append("decision")
    # the new junction against the exact curve, 16 u of the magnitudes sum |c_j| tl^j, sum j |c_j| tl^(j-1) and
    # sum j (j-1) |c_j| tl^(j-2): a term of the position passes at most 3 roundings for its power, one for its product
    # and up to 5 additions (the sixth, onto the leading zero, is exact), a term of a Horner form its factor's rounding and
    # at most 4 multiplications and 4 additions — at most 9 in every case, and (1 + u)^9 - 1 < 16 u
    x_new = [Fraction(float(v)) for v in r["x_out"]]
    exact = {}
    for axis in range(3):
        val, mag = it.exact_pva(coeff[s, axis], tl)
        for comp in range(3):
            at = axis * 3 * m + 3 * s + comp
            exact[at] = val[comp]
            if abs(x_new[at] - val[comp]) > 16 * U * mag[comp]:
                bad.append(f"new junction: axis {axis} component {comp}")
    for at, v in exact.items():
        x_new[at] = v
    # the times: T_out[s] is tl itself, T_out[s + 1] the rounded Ts - tl
    T_new = [Fraction(float(v)) for v in r["T_out"]]
    if r["T_out"][s] != tl or abs(T_new[s + 1] - (Fraction(float(T[s])) - Fraction(tl))) > U * Fraction(float(T[s])):
        bad.append("cut times")
    T_new[s], T_new[s + 1] = Fraction(tl), Fraction(float(T[s])) - Fraction(tl)
    if sum(T_new) != sum(Fraction(float(v)) for v in T):
        bad.append("time sum")
    # the m + 1 rows formed exactly from their end conditions
    new = it.segment_rows_exact(m + 1, [Fraction(v) for v in Df], x_new, T_new)
    for axis in range(3):
        for k in range(m + 1):
            if k <= s:
                want = old[(k, axis)]
            elif k == s + 1:
                want = it.taylor_shift(old[(s, axis)], tl)
            else:
                want = old[(k - 1, axis)]
            if new[(k, axis)] != want:
                bad.append(f"segment {k} axis {axis}")
    return bad


# (m, seed, the cut's trajectory time as a fraction of time_sum): first, middle and last segments
PRESERVE = [(2, 1, 0.11), (2, 2, 0.83), (3, 3, 0.5), (5, 4, 0.07), (5, 5, 0.52), (5, 6, 0.97), (8, 7, 0.61)]


def _when(m, seed, frac):
    T = consistent_row(m, seed)[2]
    return float(np.float64(frac) * np.add.reduce(T))


@pytest.mark.parametrize("m,seed,frac", PRESERVE)
def test_the_curve_is_preserved_in_exact_arithmetic(m, seed, frac):
    bad = curve_preservation_failures(m, seed, _when(m, seed, frac), min_fraction=1e-3)
    assert bad == [], bad


def test_the_cases_cut_first_middle_and_last_segments():
    cut = set()
    for m, seed, frac in PRESERVE:
        x, Df, T, coeff, _ = consistent_row(m, seed)
        s = int(it.insert_row(m, x, coeff, T, mode=it.AT_TIME, when=_when(m, seed, frac), min_fraction=1e-3)["info"][0])
        cut.add("first" if s == 0 else "last" if s == m - 1 else "middle")
    assert cut == {"first", "middle", "last"}


# ---- (3) mutants ---------------------------------------------------------------------------------------------------
def decision_failures(mutant=None):
    """LONGEST's tie-break, the fallback and the clamp on small rows with known answers."""
    bad = []
    m = 4
    x, coeff = np.zeros(9 * (m - 1)), np.zeros((m, 3, 6))
    T = np.array([1.0, 2.0, 0.5, 2.0])
    r = it.insert_row(m, x, coeff, T, mode=it.LONGEST, mutant=mutant)
    if r["info"][0] != 1 or r["info"][1] != 1.0:
        bad.append("first of the largest")
    for w in (-1.0, np.nan, np.inf):
        r = it.insert_row(m, x, coeff, T, mode=it.AT_TIME, when=w, mutant=mutant)
        if r["info"][0] != 1 or r["info"][2] != 1:
            bad.append(f"fallback {w}")
    # the clamp: 2^-10 into segment 1 with min_fraction 1/4 -> tl = 0.5 exactly; past the end -> last, tl = hi
    r = it.insert_row(m, x, coeff, T, mode=it.AT_TIME, when=1.0 + 2.0 ** -10, min_fraction=0.25, mutant=mutant)
    if tuple(r["info"][:4]) != (1.0, 0.5, 0.0, 1.0) or tuple(r["T_out"]) != (1.0, 0.5, 1.5, 0.5, 2.0):
        bad.append("clamp from below")
    r = it.insert_row(m, x, coeff, T, mode=it.AT_TIME, when=100.0, min_fraction=0.25, mutant=mutant)
    if tuple(r["info"][:4]) != (3.0, 1.5, 0.0, 1.0) or tuple(r["T_out"]) != (1.0, 2.0, 0.5, 1.5, 0.5):
        bad.append("clamp from above")
    r = it.insert_row(m, x, coeff, T, mode=it.AT_TIME, when=3.0, min_fraction=0.25, mutant=mutant)   # on a junction
    if tuple(r["info"][:4]) != (2.0, 0.125, 0.0, 1.0):
        bad.append("on a junction")
    r = it.insert_row(m, x, coeff, T, mode=it.AT_TIME, when=1.75, min_fraction=0.25, mutant=mutant)  # an idle clamp
    if tuple(r["info"][:4]) != (1.0, 0.75, 0.0, 0.0):
        bad.append("idle clamp")
    return bad


def test_decisions():
    assert decision_failures() == []


@pytest.mark.parametrize("mutant", it.MUTANTS)
def test_every_mutant_is_caught(mutant):
    """junction_shift, times_swapped and old_axis_stride break the curve; last_on_tie and no_clamp the decisions."""
    assert mutant in it.MUTANTS and len(it.MUTANTS) >= 5
    curve = [curve_preservation_failures(m, seed, _when(m, seed, frac), mutant=mutant, min_fraction=1e-3)
             for m, seed, frac in PRESERVE]
    decisions = decision_failures(mutant)
    if mutant in ("junction_shift", "times_swapped", "old_axis_stride"):
        assert all(curve), (mutant, curve)
    else:
        assert decisions, mutant
    assert any(curve) or decisions


# ---- (4) a known answer without the twin's arithmetic ---------------------------------------------------------------
def constant_velocity_row(m=5):
    """p0, v, T and the cut time are dyadic with few bits, all accelerations 0: every product and sum below is exact.
    -> (x, Df, T, coeff, when, the new waypoint (p (3,), v (3,), a (3,)), s, tl)"""
    p0 = np.array([1.5, -2.25, 0.75])
    v = np.array([0.5, 1.25, -0.375])
    T = np.array([1.0, 0.5, 2.0, 0.25, 1.5])[:m]
    starts = np.concatenate([[0.0], np.cumsum(T)])
    coeff = np.zeros((m, 3, 6))
    x = np.zeros((3, 3 * m - 3))
    for s in range(m):
        coeff[s, :, 0], coeff[s, :, 1] = p0 + v * starts[s], v
    for k in range(1, m):
        x[:, 3 * (k - 1)], x[:, 3 * (k - 1) + 1] = p0 + v * starts[k], v
    Df = np.zeros((3, 6))
    Df[:, 0], Df[:, 1], Df[:, 3], Df[:, 4] = p0, v, p0 + v * starts[m], v
    when = 2.0 + 0.8125                    # in segment 2 (it starts at 1.5), tl = 1.3125
    return x.reshape(-1), Df.reshape(-1), T, coeff, when, (p0 + v * when, v, np.zeros(3)), 2, 1.3125


def check_constant_velocity(x_out, T_out, info, m=5):
    _, _, T, _, when, (p_new, v_new, a_new), s, tl = constant_velocity_row(m)
    assert (info[0], info[1], info[2], info[3]) == (s, tl, 0, 0)
    X = np.asarray(x_out).reshape(3, 3 * m)
    assert np.array_equal(X[:, 3 * s], p_new) and np.array_equal(X[:, 3 * s + 1], v_new)
    assert np.array_equal(X[:, 3 * s + 2], a_new)
    assert T_out[s] == tl and T_out[s + 1] == T[s] - tl and np.add.reduce(T_out) == np.add.reduce(T)
    assert np.array_equal(np.delete(T_out, s + 1)[np.arange(m) != s], T[np.arange(m) != s])


def test_constant_velocity_known_answer():
    x, Df, T, coeff, when, _, _, _ = constant_velocity_row()
    r = it.insert_row(5, x, coeff, T, mode=it.AT_TIME, when=when, min_fraction=0.125)
    check_constant_velocity(r["x_out"], r["T_out"], r["info"])
    # and every other junction is where it was, one place on behind the cut
    X, X0 = r["x_out"].reshape(3, 15), x.reshape(3, 12)
    assert np.array_equal(X[:, :6], X0[:, :6]) and np.array_equal(X[:, 9:], X0[:, 6:])


# ---- (5) the binding ----------------------------------------------------------------------------------------------
OPTS = insert.GtopInsert(mode=0)


def _args(T_shape):
    return dict(x=t("x", (B, 9 * (M - 1))), coeff=t("coeff", (B, M, 18)), T=t("T", T_shape))


@pytest.mark.parametrize("T_shape,stride", T_FORMS)
def test_call_record_of_the_device_form(T_shape, stride, allocations):
    ctx = make_context()
    n_old, n_new = B * 9 * (M - 1), 9 * M
    report = t("report", (B, 12))
    given = dict(lb=t("lb", (B, 9 * (M - 1))), ub=t("ub", (B, 9 * (M - 1))), x_out=t("x_out", (B, n_new)),
                 T_out=t("T_out", (B, M + 1)), lb_out=t("lb_out", (B, n_new)), ub_out=t("ub_out", (B, n_new)),
                 info=t("info", (B, 6)))
    out = insert.insert_waypoints_device(ctx, OPTS, when=report, when_column=2, stream=STREAM, **_args(T_shape), **given)
    assert [o.name for o in out] == ["x_out", "T_out", "lb_out", "ub_out", "info"] and allocations == []
    (name, a), = ctx._L.calls
    assert name == "gtop_insert_waypoints_device" and a[0] == HANDLE and a[1] is OPTS
    assert a[2:] == (B, M, p("x"), p("coeff"), p("T"), stride, p("report") + 16, 12, p("lb"), p("ub"), p("x_out"),
                     p("T_out"), p("lb_out"), p("ub_out"), p("info"), STREAM)
    assert n_old == given["lb"].numel()
    # a (B,) tensor of times: stride 1; no bounds, outputs left out: x_out, T_out and info are allocated
    ctx = make_context()
    out = insert.insert_waypoints_device(ctx, OPTS, when=t("when", (B,)), stream=STREAM, **_args(T_shape))
    (_, a), = ctx._L.calls
    assert a[8:12] == (p("when"), 1, None, None) and a[14:16] == (None, None)
    assert [(fn, shape, dtype) for fn, shape, dtype, _ in allocations] == [("empty", (B, n_new), F64),
                                                                           ("empty", (B, M + 1), F64),
                                                                           ("empty", (B, 6), F64)]
    assert out[2] is None and out[3] is None and a[12] == p("new0") and a[13] == p("new1") and a[16] == p("new2")
    # LONGEST without when, without info
    ctx = make_context()
    out = insert.insert_waypoints_device(ctx, insert.GtopInsert(), want_info=False, stream=STREAM, **_args(T_shape))
    (_, a), = ctx._L.calls
    assert a[8] is None and a[16] is None and out[4] is None
    # the one stream rule
    ctx = make_context()
    import types
    insert.insert_waypoints_device(ctx, OPTS, when=t("when", (B,)), stream=types.SimpleNamespace(cuda_stream=12345),
                                   **_args(T_shape))
    assert ctx._L.calls[0][1][-1] == 12345


def test_refusals_of_the_device_form(allocations):
    good = dict(_args((B, M)), when=t("report", (B, 12)), lb=t("lb", (B, 9 * (M - 1))), ub=t("ub", (B, 9 * (M - 1))),
                x_out=t("x_out", (B, 9 * M)), T_out=t("T_out", (B, M + 1)), lb_out=t("lb_out", (B, 9 * M)),
                ub_out=t("ub_out", (B, 9 * M)), info=t("info", (B, 6)))
    tried = 0
    for name, value in good.items():
        for defect, spoil in DEFECTS.items():
            ctx = make_context()
            with pytest.raises(ValueError):
                insert.insert_waypoints_device(ctx, OPTS, when_column=2, stream=STREAM, **dict(good, **{name: spoil(value)}))
            assert ctx._L.calls == [], (name, defect)
            tried += 1
    assert tried == 5 * len(good)
    for bad in (dict(when_column=12), dict(when_column=-1), dict(ub=None), dict(lb=None, ub=None),
                dict(when=t("w3", (B, 2, 6)))):
        ctx = make_context()
        with pytest.raises(ValueError):
            insert.insert_waypoints_device(ctx, OPTS, stream=STREAM, **dict(dict(good, when_column=2), **bad))
        assert ctx._L.calls == []


def test_call_record_of_the_host_form():
    ctx = make_context()
    x = np.zeros((B, 9 * (M - 1)))
    x_out, T_out, lb_out, ub_out, info = insert.insert_waypoints(ctx, x, insert.GtopInsert())
    (name, a), = ctx._L.calls
    assert name == "gtop_insert_waypoints" and a[0] == HANDLE and a[2] == B and a[4:7] == (None, None, None)
    assert a[9:11] == (None, None) and lb_out is None and ub_out is None
    assert x_out.shape == (B, 9 * M) and T_out.shape == (B, M + 1) and info.shape == (B, 6)
    ctx = make_context()
    out = insert.insert_waypoints(ctx, x, OPTS, when=np.ones(B), lb=x - 1, ub=x + 1)
    (_, a), = ctx._L.calls
    assert all(v is not None for v in a[3:]) and out[2].shape == out[3].shape == (B, 9 * M)
    for bad in (dict(when=np.ones(B + 1)), dict(lb=x), dict(lb=x[:, 1:], ub=x)):
        with pytest.raises(ValueError):
            insert.insert_waypoints(make_context(), x, OPTS, **bad)
