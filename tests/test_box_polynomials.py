"""Moving obstacles on polynomial predictions, on the CPU: the C-ABI's new symbols and the host helper
gtop_box_polynomial_centres — the centre arithmetic of every kernel, stated once more on the host — against the exact
rational arithmetic of tests/box_poly_twin.py, bit for bit."""
import ctypes

import numpy as np
import pytest

from tests import box_poly_twin as bpt

ERR_INVALID = 1


def _draws(n=200, seed=11):
    """(coef (3, 6), t_range or None, time) draws: coefficients of mixed size, times inside, outside and on the bounds,
    no t_range, infinite bounds on either side or both, and t1 == t2."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        coef = rng.normal(size=(3, 6)) * 10.0 ** rng.integers(-3, 3, (3, 6))
        t1 = float(rng.uniform(-2.0, 6.0))
        t2 = t1 + float(rng.uniform(0.0, 6.0))
        kind = i % 8
        tr = [t1, t2]
        if kind == 1:
            tr = None
        elif kind == 2:
            tr = [-np.inf, t2]
        elif kind == 3:
            tr = [t1, np.inf]
        elif kind == 4:
            tr = [-np.inf, np.inf]
        elif kind == 5:
            tr = [t1, t1]
        t = float(rng.uniform(-6.0, 16.0))
        if kind == 6:
            t = t1 if i % 16 == 6 else t2          # exactly on a bound
        out.append((coef, tr, t))
    return out


def test_symbols_bindings_and_abi_version(gtop):
    lib = ctypes.CDLL(gtop.library_path())
    for name in ("gtop_set_moving_box_polynomials", "gtop_get_moving_box_kind", "gtop_box_polynomial_centres"):
        assert hasattr(lib, name), name
    assert lib.gtop_abi_version() >= 7
    for name in ("set_moving_box_polynomials", "moving_box_kind"):
        assert hasattr(gtop.GtopContext, name), name
    assert hasattr(gtop, "box_polynomial_centres")
    assert (gtop.GtopContext.BOXES_CONST_VEL, gtop.GtopContext.BOXES_POLYNOMIAL) == (0, 1)


def test_the_twins_fast_fma_is_the_fraction_fma():
    """box_poly_twin.fma (integer ratios) against fma_fraction (fractions.Fraction, the definition) on every Horner step
    of the draws, and on operands that cancel, underflow towards zero and differ hugely in size."""
    n = 0
    for coef, tr, t in _draws():
        tc = t if tr is None else bpt.clamp_time(t, *tr)
        for k in range(3):
            r = float(coef[k][5])
            for i in (4, 3, 2, 1, 0):
                a, b = bpt.fma(r, tc, coef[k][i]), bpt.fma_fraction(r, tc, coef[k][i])
                assert a == b and np.signbit(a) == np.signbit(b)
                r = a
                n += 1
    assert n == 200 * 15
    for a, b, c in ((1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0), (1e-200, 1e-150, 5e-324), (3.0, 1e300, -1e284),
                    (0.1, 10.0, -1.0), (2.0 ** -600, 2.0 ** -600, 2.0 ** 600), (0.0, 5.0, 0.0)):
        assert bpt.fma(a, b, c) == bpt.fma_fraction(a, b, c)
    assert bpt.fma(0.1, 10.0, -1.0) == 2.0 ** -54          # a true fma: 0.1 * 10 rounds to 1.0 when rounded first


def test_centres_agree_with_the_twin_bit_for_bit(gtop):
    draws = _draws()
    seen = dict(outside=0, inside=0, null=0, inf=0, point=0)
    for coef, tr, t in draws:
        got = gtop.box_polynomial_centres(coef[None], [t], None if tr is None else [tr])
        want = bpt.centres(coef[None], t, None if tr is None else [tr], fma_=bpt.fma_fraction)
        assert got.shape == (1, 1, 3)
        assert np.array_equal(got[0], want), (coef, tr, t, got, want)
        seen["null"] += tr is None
        if tr is not None:
            seen["inf"] += bool(np.isinf(tr).any())
            seen["point"] += tr[0] == tr[1]
            seen["outside" if (t < tr[0] or t > tr[1]) else "inside"] += 1
    print(seen)
    assert all(v >= 10 for v in seen.values()), seen
    # the same through one call: several boxes, several times, the (ntimes, nbox, 3) layout
    bounded = [d for d in draws if d[1] is not None][:12]
    coef = np.array([d[0] for d in bounded])
    tr = np.array([d[1] for d in bounded])
    times = np.array([d[2] for d in draws[:9]])
    got = gtop.box_polynomial_centres(coef, times, tr)
    assert got.shape == (9, 12, 3)
    for i, t in enumerate(times):
        assert np.array_equal(got[i], bpt.centres(coef, t, tr, fma_=bpt.fma_fraction))


def test_a_degree_one_row_is_one_fma(gtop):
    rng = np.random.default_rng(5)
    for _ in range(50):
        c0, c1 = rng.normal(size=3) * 10.0, rng.normal(size=3)
        coef = np.zeros((1, 3, 6))
        coef[0, :, 0], coef[0, :, 1] = c0, c1
        t = float(rng.uniform(-5.0, 20.0))
        got = gtop.box_polynomial_centres(coef, [t])[0, 0]
        want = np.array([bpt.fma_fraction(c1[k], t, c0[k]) for k in range(3)])
        assert np.array_equal(got, want)


def test_the_helper_refuses_bad_arguments(gtop):
    lib = gtop.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    coef = np.zeros((2, 3, 6))
    times = np.array([0.5, 1.5])
    out = np.full((2, 2, 3), 7.0)
    p = lambda a: a.ctypes.data_as(dp)
    assert lib.gtop_box_polynomial_centres(2, p(coef), None, 2, p(times), p(out)) == 0
    assert np.all(out == 0.0)
    out[:] = 7.0
    assert lib.gtop_box_polynomial_centres(2, None, None, 2, p(times), p(out)) == ERR_INVALID
    assert lib.gtop_box_polynomial_centres(2, p(coef), None, 2, None, p(out)) == ERR_INVALID
    assert lib.gtop_box_polynomial_centres(2, p(coef), None, 2, p(times), None) == ERR_INVALID
    assert lib.gtop_box_polynomial_centres(-1, p(coef), None, 2, p(times), p(out)) == ERR_INVALID
    for bad in ([[0.0, 1.0], [2.0, 1.0]], [[np.nan, 1.0], [0.0, 1.0]], [[0.0, 1.0], [0.0, np.nan]]):
        tr = np.array(bad)
        assert lib.gtop_box_polynomial_centres(2, p(coef), p(tr), 2, p(times), p(out)) == ERR_INVALID, bad
        with pytest.raises(gtop.GtopError) as e:
            gtop.box_polynomial_centres(coef, times, tr)
        assert e.value.code == ERR_INVALID
    bad_coef = coef.copy()
    bad_coef[1, 2, 3] = np.inf
    assert lib.gtop_box_polynomial_centres(2, p(bad_coef), None, 2, p(times), p(out)) == ERR_INVALID
    assert np.all(out == 7.0)                                   # a refused call writes nothing
    tr = np.array([[0.0, 0.0], [-np.inf, np.inf]])              # t1 == t2 and infinite bounds are fine
    assert lib.gtop_box_polynomial_centres(2, p(coef), p(tr), 2, p(times), p(out)) == 0
