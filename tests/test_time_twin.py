"""tests/time_twin.py — the numpy restatement of include/gtop_time.h — against what it restates: its cost is
consistent_twin.cost_grad's, its gT the derivative of that cost (central differences; four deliberately wrong variants
miss), its parts sum to the cost, the hand-derived case of tests/golden/TIME_ANALYTIC.md, and the optimizer's laws."""
import numpy as np
import pytest

from oracle import np_twin
from tests import consistent_twin as ct
from tests import time_twin as tt
from tests.test_consistent_gradient import DYN, PARAMS, LinearField, _fd_path, _scene

MODES = [dict(), DYN, dict(DYN, step=1)]
IDS = ["plain", "dyn", "dyn-step1"]
# tests/golden/TIME_ANALYTIC.md: the twin's two runs end within 1.81e-6 and 1.80e-6 of T* (relative), in 25 and 20-odd
# evaluations; asserted at ten times the larger
ANALYTIC_TOL = 1.8e-5


@pytest.mark.parametrize("extra", MODES, ids=IDS)
def test_cost_is_the_consistent_twins(oracle_mod, extra):
    """The per-segment closed form against the generator's matrices, on random maps: 1e-12."""
    b, sdf = _scene(oracle_mod, B=6)
    p = dict(PARAMS, **extra)
    worst = 0.0
    for i in range(len(b.x)):
        c_ref, _, info = ct.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, p, ct.CONSISTENT)
        c, gT, parts = tt.cost_gradT(b.T[i], b.Df[i], b.x[i], sdf, p)
        worst = max(worst, abs(c - c_ref) / abs(c_ref))
        # the parts sum to the cost; the collision + dyn part is the callback's, weighted
        assert abs((parts[:, 0].sum() + parts[:, 1].sum() + 1e-3) - c) <= 1e-13 * abs(c)
        cd_ref = p["wc"] * info["cost_colli"] + info["cost_dyn"]
        assert abs(parts[:, 1].sum() - cd_ref) <= 1e-12 * max(abs(cd_ref), 1e-300)
        assert np.array_equal(gT, parts[:, 2] + parts[:, 3]) and np.all(np.isfinite(gT))
    print(f"cost against consistent_twin: {worst:.2e}")
    assert worst <= 1e-12


def _fd(T, Df, x, sdf, p, h=1e-6):
    fd = np.zeros(len(T))
    for s in range(len(T)):
        Tp, Tm = T.copy(), T.copy()
        Tp[s] += h
        Tm[s] -= h
        fd[s] = (ct.cost_grad(Tp, Df, x, sdf, p, ct.CONSISTENT)[0] - ct.cost_grad(Tm, Df, x, sdf, p, ct.CONSISTENT)[0]) / (2 * h)
    return fd


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("extra", [dict(), DYN, dict(DYN, alpha=0.0)], ids=["plain", "dyn", "dyn-alpha0"])
def test_gT_is_the_derivative_of_the_cost_and_the_mutants_are_not(monkeypatch, extra, seed):
    """Central differences in T (h = 1e-6) of consistent_twin's cost with the float round trips switched off, on a
    linear field: within 1e-5 of the max-norm (the bound of test_consistent_gradient.py, for its reason: the 1e-5 of
    vel_norm biases one term by 1e-5/|v|).  Each mutant misses that bound by ten times in at least one of the modes;
    every one of them is checked in the modes where its term is live."""
    monkeypatch.setattr(ct, "to_float", lambda v: v)
    T, Df, x = _fd_path(4, seed)
    p = dict(PARAMS, **extra)
    sdf = LinearField()
    fd = _fd(T, Df, x, sdf, p)
    scale = np.max(np.abs(fd))
    _, gT, _ = tt.cost_gradT(T, Df, x, sdf, p)
    dev = np.max(np.abs(gT - fd)) / scale
    print(f"central differences in T: off by {dev:.2e} of the max-norm")
    assert dev <= 1e-5, dev
    for mutant in tt.MUTANTS:
        _, gm, _ = tt.cost_gradT(T, Df, x, sdf, p, mutant=mutant)
        off = np.max(np.abs(gm - fd)) / scale
        print(f"  mutant {mutant}: off by {off:.2e}")
        assert off >= 1e-4, (mutant, off)


def _rest_case(L=3.0, ws=1.0):
    """wc = 0, m = 2, waypoints at 0, L/2, L on the x axis, everything at rest (tests/golden/TIME_ANALYTIC.md)."""
    Df = np.zeros((3, 6))
    Df[0, 3] = L
    x = np.zeros((3, 3))
    x[0, 0] = L / 2
    return Df, x.reshape(-1), dict(PARAMS, ws=ws, wc=0.0)


class NoField:
    def query(self, pos):
        raise AssertionError("|wc| < 1e-4: no lookup")


def test_hand_derived_gradient():
    """Rest to rest over D = L/2 in time T costs 720 ws D^2 / T^5: gT = -3600 ws D^2 / T^6, to 1e-12."""
    L, ws = 3.0, 1.7
    Df, x, p = _rest_case(L, ws)
    for T in (np.array([1.0, 3.0]), np.array([0.5, 0.5]), np.array([0.02, 7.0])):
        c, gT, parts = tt.cost_gradT(T, Df, x, NoField(), p)
        c_ref = 720 * ws * (L / 2) ** 2 / T ** 5
        g_ref = -3600 * ws * (L / 2) ** 2 / T ** 6
        assert np.max(np.abs(parts[:, 0] - c_ref) / c_ref) <= 1e-12
        assert np.max(np.abs(gT - g_ref) / np.abs(g_ref)) <= 1e-12
        assert abs(c - (c_ref.sum() + 1e-3)) <= 1e-12 * c
        assert np.all(parts[:, 1] == 0.0) and np.all(parts[:, 3] == 0.0)


@pytest.mark.parametrize("start", [[1.0, 3.0], [0.5, 0.5]])
def test_optimizer_finds_the_analytic_optimum(start):
    """The fixed point of cost + rho sum(T) on that case is T* = (3600 ws D^2 / rho)^(1/6) per segment."""
    L, ws, rho = 3.0, 1.0, 2.0
    Df, x, p = _rest_case(L, ws)
    Tstar = (3600 * ws * (L / 2) ** 2 / rho) ** (1 / 6)
    trace = []
    T_out, info = tt.optimize_times(np.array(start), Df, x, NoField(), p, rho=rho, t_min=0.05, t_max=60.0,
                                    first_move=0.1, ftol_rel=1e-9, xtol_abs=0.0, max_evals=60, trace=trace)
    err = np.max(np.abs(T_out - Tstar)) / Tstar
    print(f"from {start}: T* = {Tstar:.9f}, reached within {err:.2e} in {int(info[2])} evaluations, code {int(info[0])}")
    assert err <= ANALYTIC_TOL, err
    assert info[0] == tt.FTOL and info[2] <= 60
    assert np.all(np.diff(trace) <= 0.0) and len(trace) == info[1] + 1          # F never rises
    assert info[3] == trace[0] and info[4] == trace[-1] and info[7] == T_out.sum()
    assert abs(info[4] - (info[5] + rho * T_out.sum())) <= 1e-15 * info[4]
    assert info[6] <= 1e-4 * rho                                                  # stationary: |g| small against rho


def test_optimizer_laws(oracle_mod):
    b, sdf = _scene(oracle_mod, B=3, m=4)
    p = dict(PARAMS)
    kw = dict(rho=1.0, t_min=0.2, t_max=2.5, first_move=0.05, ftol_rel=1e-7, xtol_abs=1e-10, max_evals=25)
    for i in range(len(b.x)):
        T_lo = np.array([0.1, 3.0, 0.9 * b.T[i][2], 0.0])             # below t_min; pinned (> t_max); active; none
        trace = []
        T_out, info = tt.optimize_times(b.T[i], b.Df[i], b.x[i], sdf, p, T_lo=T_lo, trace=trace, **kw)
        assert np.all(np.diff(trace) <= 0.0)                                       # F monotone
        lo = np.maximum(kw["t_min"], T_lo)
        assert T_out[1] == 3.0                                                     # pinned: untouched by the descent
        free = np.array([0, 2, 3])
        assert np.all(T_out[free] >= lo[free]) and np.all(T_out[free] <= kw["t_max"])   # bounds exact
        assert info[0] in (tt.FTOL, tt.XTOL, tt.MAXEVAL) and 1 <= info[2] <= kw["max_evals"]
        c, _, _ = tt.cost_gradT(T_out, b.Df[i], b.x[i], sdf, p)
        assert info[5] == c and info[4] <= info[3]
        # max_evals = 1: the clamped input, MAXEVAL
        T1, info1 = tt.optimize_times(b.T[i], b.Df[i], b.x[i], sdf, p, T_lo=T_lo, **dict(kw, max_evals=1))
        clamped = np.where(lo > kw["t_max"], lo, np.clip(b.T[i], lo, kw["t_max"]))
        assert np.array_equal(T1, clamped) and info1[0] == tt.MAXEVAL and info1[2] == 1 and info1[1] == 0
        assert info1[3] == info1[4] == info[3]
    # both weights 0 and rho = 0: every g is 0, XTOL after one evaluation
    T0, info0 = tt.optimize_times(b.T[0], b.Df[0], b.x[0], NoField(), dict(p, ws=0.0, wc=0.0), **dict(kw, rho=0.0))
    assert info0[0] == tt.XTOL and info0[2] == 1 and info0[1] == 0 and info0[6] == 0.0
    assert np.array_equal(T0, np.clip(b.T[0], kw["t_min"], kw["t_max"]))
