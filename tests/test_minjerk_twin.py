"""The exact twin of the minimum-jerk start point (tests/minjerk_twin.py) on the CPU: its matrix against its definition
and against the oracle's R, the analytic case exactly, the value criterion on a plain fp64 elimination over every input
the GPU test uses (the inputs are fair), and mutants of that elimination, each far outside the criterion."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import np_twin
from tests import minjerk_twin as mt


@pytest.mark.parametrize("T", [1.0, 0.5, 2.75, 0.05])
def test_the_table_is_the_definition(T):
    assert mt.segment_matrix(T) == mt.segment_matrix_derived(T)
    if T == 1.0:
        assert mt.segment_matrix(T) == [[Fraction(v) for v in row] for row in mt.M1]


@pytest.mark.parametrize("m", [2, 3, 5])
def test_k_and_the_known_terms_are_the_oracles_r(m):
    """The v, a rows of np_twin.generator(T)["R"]: their unknown columns are K, and applied to the known entries
    (positions and the boundary pairs) they are the twin's known vector — to rounding of the oracle's dense fp64."""
    rng = np.random.default_rng(m)
    T = rng.uniform(0.4, 2.5, size=m)
    R = np_twin.generator(T)["R"]
    unk = [6 + 3 * (k - 1) + der for k in range(1, m) for der in (1, 2)]
    K = np.array([[float(v) for v in row] for row in mt.dense(T)])
    assert np.allclose(R[np.ix_(unk, unk)], K, rtol=1e-9, atol=1e-9 * np.abs(K).max())
    d = rng.uniform(-3.0, 3.0, size=3 * m + 3)            # [start p v a | end p v a | wp1 p v a | ...]
    known = d.copy()
    known[unk] = 0.0
    got = R[unk] @ known
    want = np.array([float(v) for v in mt.known_vector(T, d[0:6], d[6::3])])
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    assert np.array_equal(K, K.T) and np.all(np.linalg.eigvalsh(K) > 0)


@pytest.mark.parametrize("m", [2, 6, 13])
def test_the_analytic_case_exactly(m):
    """tests/golden/MINJERK_ANALYTIC.md: constant velocity is the minimiser, in exact arithmetic."""
    T, Df, x_in, x_want = mt.analytic(m)
    _, u_want = mt.split(m, x_want)
    u = mt.solve(T, Df, x_in)
    for a in range(3):
        assert u[a] == [Fraction(float(v)) for v in u_want[a]]
    assert np.max(mt.ratios(T, Df, x_in, x_want)) == 0.0


def test_the_exact_solution_has_no_residual_and_the_elimination_is_close_to_it():
    T, Df, x = mt.base_rows(7, "wide", False)
    u = mt.solve(T[1], Df[1], x[1])
    pos, _ = mt.split(7, x[1])
    for a in range(3):
        for entries, known in mt.rows(T[1], Df[1].reshape(3, 6)[a], pos[a]):
            assert sum(k * u[a][j] for j, k in entries) + sum(v for v, _ in known) == 0
    _, got = mt.split(7, mt.eliminate(T[1], Df[1], x[1]))
    want = np.array([[float(v) for v in ua] for ua in u])
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


@pytest.mark.parametrize("m", mt.SEGMENTS)
def test_a_plain_fp64_elimination_meets_the_value_criterion_on_every_gpu_input(m):
    """The inputs of tests/test_gpu_minjerk.py are fair: numpy's fp64, unfused, passes on every base row."""
    worst = 0.0
    for (mm, t_range, shared) in mt.cases():
        if mm != m:
            continue
        T, Df, x = mt.base_rows(m, t_range, shared)
        for b in range(mt.BASE_ROWS):
            out = mt.eliminate(T[b], Df[b], x[b])
            pos_in, _ = mt.split(m, x[b])
            pos_out, _ = mt.split(m, out)
            assert np.array_equal(pos_in, pos_out)
            worst = max(worst, mt.worst_ratio(T[b], Df[b], x[b], out))
    print(f"m = {m}: worst |r| / (u mag) = {worst:.1f}")
    assert worst <= mt.BOUND_K


@pytest.mark.parametrize("mutant", mt.MUTANTS)
def test_mutants_exceed_four_times_the_bound(mutant):
    for m, t_range, shared in ((6, "narrow", False), (13, "wide", True)):
        T, Df, x = mt.base_rows(m, t_range, shared)
        out = mt.eliminate(T[0], Df[0], x[0], mutant=mutant)
        assert np.max(mt.ratios(T[0], Df[0], x[0], out)) > 4 * mt.BOUND_K, (mutant, m)
