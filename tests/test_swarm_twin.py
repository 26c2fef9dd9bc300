"""The arithmetic of include/gtop_swarm.h without a GPU (tests/swarm_twin.py): in exact rational arithmetic the gradient
formula EQUALS the 7-point central difference quotient of S_b along every coordinate (S_b is a polynomial of degree 6 in
x while the active and flown sets do not change, so that quotient is exact); the d c / d q table is the difference of
the library's coefficient formula as include/gtop_time.h states it; the float64 twin lies within 2^12 u of the exact
one, entry by entry, against the sum of the terms' magnitudes (the bound of tests/test_gpu_entrywise.py); the
hand-derived case of tests/golden/SWARM_ANALYTIC.md; S_0 == S_1 for two rows; a pair at d2 == R2 exactly is inactive;
five mutants die."""
from fractions import Fraction

import numpy as np
import pytest

from tests import separation_twin as st
from tests import swarm_limit_cases as lc
from tests import swarm_twin as sw

H = Fraction(1, 2 ** 30)
FD_WEIGHTS = ((-3, Fraction(-1, 60)), (-2, Fraction(3, 20)), (-1, Fraction(-3, 4)), (1, Fraction(3, 4)),
              (2, Fraction(-3, 20)), (3, Fraction(1, 60)))
E_FLOOR = Fraction(1, 2 ** 10)
U64, KAPPA = 2.0 ** -53, 2 ** 12


def analytic_rows():
    c = np.zeros((2, 2, 18))
    c[:, 0, 1] = c[:, 1, 1] = 1.0
    c[:, 1, 0] = 2.0
    c[1, :, 6] = 0.5
    return c, np.array([2.0, 2.0]), dict(t0=None, t_lo=0.0, dt=0.5, n=9, hold_ends=0, w=2.0, radius=1.0)


def analytic_faults(mutant=None, N=sw.FLOAT):
    """What of tests/golden/SWARM_ANALYTIC.md a (mutant) twin misses."""
    c, T, o = analytic_rows()
    S, g, act, _ = sw.swarm_terms(c, T, N=N, mutant=mutant, **o)
    want = np.zeros((2, 9))
    want[0, 3:6] = (6.75, 0.0, 0.4482421875)
    want[1] = -want[0]
    faults = []
    if [float(v) for v in S] != [3.796875, 3.796875]:
        faults.append("S")
    if list(act) != [9, 9]:
        faults.append("active")
    if not np.array_equal(np.asarray(g, dtype=np.float64), want):
        faults.append("grad")
    return faults


def touching_faults(mutant=None, N=sw.FLOAT):
    """Two rows that stand 3, 4, 0 apart with R = 5: d2 == R2 exactly, which is not active."""
    c = np.zeros((2, 2, 18))
    c[1, :, 0], c[1, :, 6] = 3.0, 4.0
    S, g, act, least = sw.swarm_terms(c, np.array([1.0, 1.0]), None, 0.0, 0.25, 9, 0, 1.0, 5.0, N=N, mutant=mutant)
    faults = [] if least == 0 else ["the case is not at the radius"]
    if [float(v) for v in S] != [0.0, 0.0] or list(act) != [0, 0] or any(float(v) != 0.0 for v in g.reshape(-1)):
        faults.append("a term at the radius is active")
    return faults


def fd_case(m, hold, frozen, t0_kind, seed):
    """Dyadic rows, exact: (x, Df, T, frozen coefficients or None, t0, options)."""
    x, Df, T = sw.crossing_rows(3, m, seed, dyadic=True)
    t0 = None
    if t0_kind == "one":
        t0 = [0.25]
    elif t0_kind == "rows":   # row 2 starts after row 0 has landed: that pair has no common sample (hold_ends = 0)
        t0 = [0.0, np.round(float(np.sum(T[0])) * 8.0) / 16.0, float(np.sum(T[0])) + 0.25]
    span = float(np.max(np.sum(T, axis=1))) + (t0[-1] if t0 else 0.0)
    n = 16
    dt = np.ceil(span / (n - 1) * 16.0) / 16.0
    fz = None
    if frozen:
        xf, _, _ = sw.crossing_rows(3, m, seed + 100, dyadic=True)
        fz = sw.coefficients(xf, Df, T, sw.EXACT)
    return x, Df, T, fz, t0, dict(t_lo=0.0, dt=dt, n=n, hold_ends=hold, w=1.5, radius=2.0)


def fd_faults(case, mutant=None, rows=(0, 1, 2)):
    """Entries of the gradient formula that differ from the exact difference quotient; the case's own preconditions."""
    x, Df, T, fz, t0, o = case
    X = sw.EXACT.arr(x)

    def S_of(Xp):
        return sw.swarm_terms(sw.coefficients(Xp, Df, T, sw.EXACT), T, t0, frozen=fz, N=sw.EXACT, mutant=mutant,
                              want_grad=False, **o)

    S, g, act, least = sw.swarm_terms(sw.coefficients(X, Df, T, sw.EXACT), T, t0, frozen=fz, N=sw.EXACT, mutant=mutant, **o)
    assert act.sum() > 0 and least >= E_FLOOR, (act, float(least))
    faults = []
    for b in rows:
        for i in range(X.shape[1]):
            q = Fraction(0)
            for k, wgt in FD_WEIGHTS:
                Xp = X.copy()
                Xp[b, i] = X[b, i] + k * H
                Sp, _, actp, _ = S_of(Xp)
                assert np.array_equal(actp, act)   # the active set did not move
                q += wgt * Sp[b]
            if q / H != g[b, i]:
                faults.append((b, i))
    return faults


FD_CASES = [(2, 0, False, None, 1), (3, 1, True, None, 2), (6, 0, False, "rows", 3), (3, 0, True, "rows", 4),
            (2, 1, False, "one", 5), (6, 1, True, None, 6)]


@pytest.mark.parametrize("m,hold,frozen,t0_kind,seed", FD_CASES)
def test_the_gradient_is_the_exact_difference_quotient(m, hold, frozen, t0_kind, seed):
    case = fd_case(m, hold, frozen, t0_kind, seed)
    if t0_kind == "rows":   # one pair without a common sample, the others with
        x, Df, T, fz, t0, o = case
        fl = sw.sample_rows(sw.coefficients(x, Df, T, sw.EXACT), T, t0, o["t_lo"], o["dt"], o["n"], hold, sw.EXACT)[1]
        assert not (fl[0] & fl[2]).any() and (fl[0] & fl[1]).any() and (fl[1] & fl[2]).any()
    assert fd_faults(case, rows=(0, 1, 2) if m < 6 else (1,)) == []


def test_the_D_table_is_the_coefficient_formula_differentiated():
    for T0, T1 in ((Fraction(3, 4), Fraction(5, 2)), (Fraction(2), Fraction(1, 3))):
        rng = np.random.default_rng(7)
        x = sw.EXACT.arr(np.round(rng.uniform(-2, 2, (1, 9)) * 16) / 16)
        Df = sw.EXACT.arr(np.round(rng.uniform(-2, 2, (1, 18)) * 16) / 16)
        T = sw.EXACT.arr([T0, T1])
        base = sw.coefficients(x, Df, T, sw.EXACT)
        for axis in range(3):
            for q, (end_name, start_name) in enumerate((("pT", "p0"), ("vT", "v0"), ("aT", "a0"))):
                xp = x.copy()
                xp[0, axis * 3 + q] += 1                      # c is linear in q: the difference IS the derivative
                d = sw.coefficients(xp, Df, T, sw.EXACT) - base
                for s, name, Ts in ((0, end_name, T0), (1, start_name, T1)):
                    want = [Fraction(c) / Ts ** p for c, p in sw.D_TABLE[name]]
                    assert list(d[0, s, 6 * axis:6 * axis + 6]) == want, (name, axis)
                    other = [a for a in range(3) if a != axis]
                    assert all(v == 0 for a in other for v in d[0, s, 6 * a:6 * a + 6])


def float_against_exact(x, Df, T, fz, t0, o):
    """The float twin within KAPPA u of the exact one on every entry of S and the gradient, against the magnitudes;
    returns (the worst ratio, the active terms)."""
    worst = 0.0
    ce = sw.coefficients(x, Df, T, sw.EXACT)
    cf = np.asarray(ce, dtype=np.float64)   # the coefficients rounded once: both twins start from the same rows
    ff = None if fz is None else np.asarray(fz, dtype=np.float64)
    exact = sw.swarm_terms(cf, T, t0, frozen=ff, N=sw.EXACT, **o)
    flt = sw.swarm_terms(cf, T, t0, frozen=ff, N=sw.FLOAT, **o)
    mag = sw.swarm_terms(cf, T, t0, frozen=ff, N=sw.EXACT, mag=True, **o)
    assert np.array_equal(exact[2], flt[2]) and exact[2].sum() > 0   # the same active terms
    for e, f, mg in ((exact[0], flt[0], mag[0]), (exact[1].reshape(-1), flt[1].reshape(-1), mag[1].reshape(-1))):
        for ev, fv, mv in zip(e, f, mg):
            err = abs(Fraction(float(fv)) - ev)
            assert err <= KAPPA * Fraction(U64) * mv, (o["n"], o["hold_ends"], float(err), float(mv))
            if mv > 0:
                worst = max(worst, float(err / (Fraction(U64) * mv)))
    return worst, int(exact[2].sum())


def test_float_twin_against_the_exact_one_entrywise():
    worst = 0.0
    for m, hold, frozen, t0_kind, seed in FD_CASES:
        worst = max(worst, float_against_exact(*fd_case(m, hold, frozen, t0_kind, seed))[0])
    print(f"worst |float - exact| / (u * magnitude) = {worst:.3f}")
    assert worst > 0.0   # the float twin does round: the bound is not vacuous


@pytest.mark.parametrize("B,m,n,hold,frozen,seed", lc.TWIN_CASES, ids=[f"m{c[1]}-n{c[2]}" for c in lc.TWIN_CASES])
def test_float_twin_against_the_exact_one_at_long_rows(B, m, n, hold, frozen, seed):
    """The same bound where the sums are long: the segment counts and sample counts of tests/swarm_limit_cases.py at
    which the device is compared with the float twin bit for bit (a second pass of the variables at m = 9, of the
    segment table at m = 65, more than one stage of samples at n = 300)."""
    x, Df, T = sw.crossing_rows(B, m, seed, dyadic=True)
    span = float(np.max(np.sum(T, axis=1)))
    dt = np.ceil(span / (n - 1) * 256.0) / 256.0
    fz = None
    if frozen:
        xf, _, _ = sw.crossing_rows(B, m, seed + 100, dyadic=True)
        fz = sw.coefficients(xf, Df, T, sw.EXACT)
    o = dict(t_lo=0.0, dt=dt, n=n, hold_ends=hold, w=1.5, radius=2.0)
    worst, active = float_against_exact(x, Df, T, fz, None, o)
    print(f"m = {m}, n = {n}: {active} active terms, worst |float - exact| / (u * magnitude) = {worst:.4f}")
    assert worst > 0.0 and active >= 100


def test_positions_are_the_separation_twins():
    x, Df, T = sw.crossing_rows(5, 3, 11)
    c = sw.coefficients(x, Df, T)
    for hold in (0, 1):
        pos, flown, _, _ = sw.sample_rows(c, T, [0.0, 0.1, 0.2, 0.3, 5.0], 0.05, 0.07, 40, hold)
        ref, ref_flown, _ = st.sample_rows(c, T, [0.0, 0.1, 0.2, 0.3, 5.0], 0.05, 0.07, 40, hold)
        assert np.array_equal(flown, ref_flown) and np.array_equal(pos[flown], ref[flown])


def test_the_analytic_case():
    assert analytic_faults() == [] and analytic_faults(N=sw.EXACT) == []


def test_two_rows_pay_the_same_bits():
    for seed in range(6):
        x, Df, T = sw.crossing_rows(2, 3, 20 + seed, spread=0.5, shared_T=seed % 2 == 0)
        S, g, act, _ = sw.swarm_terms(sw.coefficients(x, Df, T), T, None, 0.0, 0.05, 64, seed % 2, 3.0, 1.5)
        assert act[0] == act[1] > 0 and S[0] == S[1] and np.array_equal(S[:1].view(np.uint64), S[1:].view(np.uint64))


def test_a_pair_at_the_radius_is_inactive():
    assert touching_faults() == [] and touching_faults(N=sw.EXACT) == []


@pytest.mark.parametrize("mutant", sw.MUTANTS)
def test_mutants_die(mutant):
    small = fd_case(2, 0, False, None, 1)
    killed = analytic_faults(mutant) + touching_faults(mutant)
    if not killed:
        killed = fd_faults(small, mutant, rows=(0,))
    assert killed, mutant
    # and each by the check that is about it
    by = {"inclusive": touching_faults, "self_pair": analytic_faults, "junction": analytic_faults,
          "wrong_D": analytic_faults, "no_dt": analytic_faults}[mutant]
    assert by(mutant), mutant
    if mutant in ("junction", "wrong_D"):
        assert fd_faults(small, mutant, rows=(0,)), mutant
