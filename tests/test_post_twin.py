"""The exact twin of tests/post_twin.py, without a GPU: hand-derived known answers, agreement with the oracle (an
independent double implementation) on the inputs of tests/test_gpu_post.py at that module's derived bounds, and the
sensitivity of those checks: a plain-float model of the kernels, correct or with one of the listed defects, is run
through the same comparisons — the correct one passes, every mutant moves a checked number by more than four times its
bound or changes an exact quantity."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import post_cases as cases
from tests import post_twin as twin
from tests import post_bounds as gp


# ---------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------
def test_jerk_of_a_cubic():
    """x = t^3: the integral of (x''')^2 = 36 over T is 36 T."""
    c = np.zeros((2, 18))
    c[:, 3] = 1.0
    val, mag, _ = twin.stats(c, [2.0, 1.0], 0.25)
    assert val[2] == 36 * 3 and mag[2] == 36 * 3
    assert val[7] == 0 and val[0] == 3.0


def test_constant_velocity_line():
    """A line run at constant velocity: the length is the distance between the first and the last sample."""
    T = [0.5, 0.25, 0.75]
    v = (3.0, -4.0, 12.0)                                        # |v| = 13
    c = np.zeros((3, 18))
    start = 0.0
    for s in range(3):
        for a in range(3):
            c[s, 6 * a], c[s, 6 * a + 1] = v[a] * start, v[a]
        start += T[s]
    smp = twin.samples(c, T, 0.125)
    val, mag, info = twin.stats(c, T, 0.125, smp=smp)
    assert smp["n"] == 13 and val[8] == 13.0
    first, last = smp["pts"][0], smp["pts"][-1]
    assert abs(val[1] - twin.fsqrt(sum((last[a] - first[a]) ** 2 for a in range(3)))) < Fraction(1, 10 ** 60)
    assert abs(val[1] - 13 * Fraction(3, 2)) < Fraction(1, 10 ** 60)
    assert val[3] == 13 and val[4] == 13 and val[5] == 0 and val[6] == 0 and val[2] == 0


def test_end_time_velocity_for_every_sample():
    """The reference evaluates the velocity with pow(ts, i), the segment DURATION (:158-159): x = t^3 reports 3 T^2
    for every counted step of the segment, so the mean is the count-weighted mean of the end-time values."""
    c = np.zeros((2, 18))
    c[:, 3] = 1.0
    val, mag, info = twin.stats(c, [2.0, 1.0], 0.5)
    assert info["counts"] == [4, 2]
    assert val[4] == 12 and val[3] == Fraction(4 * 12 + 2 * 3, 6)
    assert val[6] == 12 and val[5] == Fraction(4 * 12 + 2 * 6, 6)    # acceleration 6 T


def test_accumulated_time_decides_the_count():
    """T = 0.03, dt = 0.01: eval_t = 0, 0.01, 0.02 are below T; a fourth step is counted if and only if the
    ACCUMULATED 0.01 + 0.01 + 0.01 compares below 0.03.  In IEEE double it is 0.03 itself: three steps."""
    third = 0.01 + 0.01 + 0.01
    assert twin.segment_counts([0.03], 0.01) == [3 + (third < 0.03)] == [3]
    # getTraj's `<=` keeps the sample at the accumulated 0.03 if and only if it compares <= time_sum
    assert len(twin.sample_times([0.03], 0.01)) == 3 + (third <= 0.03) == 4
    # where accumulation and product part ways: 0.01 added six times is 0.060000000000000005, above 6 * 0.01 = T
    acc6 = 0.0
    for _ in range(6):
        acc6 += 0.01
    assert acc6 > 0.06 == 6 * 0.01
    assert twin.segment_counts([0.06], 0.01) == [6]
    assert len(twin.sample_times([0.06], 0.01)) == 6 and len(twin.sample_times([0.06], 0.01, product_times=True)) == 7
    assert twin.sample_times([0.07], 0.01)[6] == acc6 and twin.sample_times([0.07], 0.01, product_times=True)[6] == 0.06


def test_walk_boundaries():
    T = [0.25, 0.5, 0.125]
    assert twin.walk(T, 0.25) == (1, 0.0) and twin.walk(T, 0.25, strict_boundary=True) == (0, 0.25)
    assert twin.walk(T, 0.875) == (2, 0.125)                     # t == time_sum: the last segment, extended
    assert twin.walk(T, 1.0) == (2, 0.25)
    assert twin.walk([0.5], 3.0) == (0, 3.0)


def test_hermite_solve_reproduces_a_quintic():
    """The rational solve returns the polynomial whose derivatives it was given."""
    c = [Fraction(v) for v in (3, -2, 5, 7, -11, 13)]
    Ts = 0.75
    A = twin.hermite_matrix(Ts)
    d = [float(sum(A[r][j] * c[j] for j in range(6))) for r in range(6)]      # exact: small binary fractions
    got, mag = twin.hermite_coefficients(d, Ts)
    assert got == c and all(m >= abs(g) for m, g in zip(mag, got))


def test_setup_restatement_quirk():
    wp = np.array([[0.0, 0, 0], [3, 4, 0], [3, 4, 12], [3, 4, 12.5]])
    T = twin.segment_time(wp, mean_v=2.0, init_time=0.3)
    assert T.tolist() == [2.5 + 0.3, 6.0, 0.25]                  # only segment 0 gets init_time
    Df, x0 = twin.initial_d(wp)
    assert Df.tolist() == [[0, 0, 0, 3, 0, 0], [0, 0, 0, 4, 0, 0], [0, 0, 0, 12.5, 0, 0]]
    assert x0.tolist() == [[3, 0, 0, 3, 0, 0], [4, 0, 0, 4, 0, 0], [0, 0, 0, 12, 0, 0]]


# ---------------------------------------------------------------------------------------------------------------------
# the twin against the oracle, on the GPU test's inputs, at the GPU test's bounds
# ---------------------------------------------------------------------------------------------------------------------
def _trajectory_inputs():
    for family in cases.PROBES:
        yield ("probe", family), cases.probe(family)
    for n in cases.CHUNK_COUNTS:
        yield ("chunk", n), cases.chunk_case(n)
    for m in cases.SEGMENT_COUNTS:
        for seg_v, seg_a in cases.arrangements(m):
            yield ("segments", m, seg_v, seg_a), cases.segment_case(m, seg_v, seg_a)
    for B in cases.BATCHES:
        T, dt, coeff = cases.batch_case(B)
        for b in range(min(B, 3)):
            yield ("batch", B, b), (T[b], dt, coeff[b])
        T, dt, coeff = cases.batch_case(B, shared_times=True)
        yield ("shared", B), (T, dt, coeff[0])


TRAJECTORY_INPUTS = dict(_trajectory_inputs())


@pytest.mark.parametrize("key", list(TRAJECTORY_INPUTS), ids=["-".join(map(str, k)) for k in TRAJECTORY_INPUTS])
def test_twin_against_oracle_trajectories(oracle_mod, key):
    T, dt, coeff = TRAJECTORY_INPUTS[key]
    smp, ref = gp.twin_of(key, coeff, T, dt)
    cap = smp["n"] + 2
    n, pts = oracle_mod.traj_samples(coeff, T, dt, max_samples=cap)
    assert n == smp["n"]
    buf = np.zeros((cap, 3))
    buf[:n] = pts
    gp.hold_samples(key + ("oracle",), buf, smp, cap, probe=key[0] == "probe")
    gp.hold_stats(key + ("oracle",), oracle_mod.traj_stats(coeff, T, dt), ref, serial=True)


def test_twin_against_oracle_decisions_every_batch_row(oracle_mod):
    T, dt, coeff = cases.batch_case(1025)
    for b in range(1025):
        st = oracle_mod.traj_stats(coeff[b], T[b], dt)
        assert st[0] == twin.time_sum(T[b]) and st[8] == len(twin.sample_times(T[b], dt))


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("m", cases.COEF_M)
def test_twin_against_oracle_coefficients(oracle_mod, m, shared):
    """oracle.coefficients goes the reference's way: L = A^-1 Ct with the 6m x 6m A inverted by LU.  Its error is
    that of the inversion (u times the condition of A, which holds 1 and T^5 side by side), not a count of roundings:
    on these inputs it reaches 1.3e5 u |A^-1| |d|, so K_COEF cannot be asked of it.  It is held to what
    tests/test_setup_post.py holds the kernel to against it (1e-9 of the trajectory's largest coefficient), here
    against the exact solve; the independent double implementation that meets K_COEF u |A^-1| |d| before a GPU is
    involved is the closed form in Python floats (test_sensitivity_dropped_half_A)."""
    T, Df, x = cases.coef_case(m, shared)
    for b in range(cases.COEF_B):
        Tb = T if shared else T[b]
        got = oracle_mod.coefficients(Tb, Df[b].reshape(3, 6), x[b])
        ref = twin.coefficients(Tb, Df[b], x[b])
        exact = np.array([[float(ref[(s, a)][0][j]) for a in range(3) for j in range(6)] for s in range(m)])
        assert np.allclose(got, exact, rtol=1e-9, atol=1e-9 * np.abs(exact).max())


def test_twin_against_oracle_setup(oracle_mod):
    wp = cases.grid_setup_case()
    for b in range(0, cases.GRID_B, 7):
        assert twin.segment_time(wp[b], 1.8, 0.3).tobytes() == oracle_mod.segment_time(wp[b], 1.8, 0.3).tobytes()
        Df, x0 = twin.initial_d(wp[b])
        Df_o, x0_o = oracle_mod.initial_d(wp[b])
        assert Df.tobytes() == Df_o.tobytes() and x0.tobytes() == x0_o.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: a plain-float model of the kernels, with switches for the defects the GPU tests are there to catch
# ---------------------------------------------------------------------------------------------------------------------
def _poly(c, t):
    t2 = t * t
    t3, t4 = t2 * t, t2 * t2
    t5 = t4 * t
    s = 0.0
    for term in (t5 * c[5], t4 * c[4], t3 * c[3], t2 * c[2], t * c[1], c[0]):
        s += term
    return s


def model_trajectory(coeff, T, dt, cap, strict_boundary=False, product_times=False, max64=False, sum64=False,
                     carry0=False):
    """(stats[9], samples (cap, 3)) the way eval_trajectories_kernel forms them, in Python floats."""
    T = [float(v) for v in T]
    m = len(T)
    cf = np.asarray(coeff, dtype=np.float64).reshape(m, 18).tolist()
    ts = twin.time_sum(T)
    times = twin.sample_times(T, dt, product_times)
    out = np.zeros((cap, 3))
    length, prev = 0.0, None
    for base in range(0, len(times), 64):
        chunk = 0.0
        for k in range(base, min(base + 64, len(times))):
            i, tl = twin.walk(T, times[k], strict_boundary)
            p = [_poly(cf[i][6 * a:6 * a + 6], tl) for a in range(3)]
            if k < cap:
                out[k] = p
            if k > 0:
                pl = [0.0, 0.0, 0.0] if (carry0 and k == base) else prev
                chunk += math.sqrt(sum((p[a] - pl[a]) * (p[a] - pl[a]) for a in range(3)))
            prev = p
        length += chunk
    cnt = twin.segment_counts(T, dt)
    acc_cost = jerk = sum_v = sum_a = 0.0
    max_v = max_a = -1.0
    num = 0
    for s in range(m):
        Ts = T[s]
        Tp = [1.0, Ts, Ts * Ts, Ts * Ts * Ts, (Ts * Ts) * (Ts * Ts), (Ts * Ts) * (Ts * Ts) * Ts]
        c = cf[s]
        vel, acc = [], []
        jk = 0.0
        for a in range(3):
            cc = c[6 * a:6 * a + 6]
            q = 0.0
            for j in range(3, 6):
                col = 0.0
                for i in range(3, 6):
                    col += cc[i] * (float(i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2)) * Tp[i + j - 5] / float(i + j - 5))
                q += col * cc[j]
            jk += q
            vel.append(sum(Tp[i] * ((i + 1.0) * cc[i + 1]) for i in range(5)))
            acc.append(sum(Tp[i] * (float((i + 2) * (i + 1)) * cc[i + 2]) for i in range(4)))
        vn = math.sqrt(sum(v * v for v in vel))
        an = math.sqrt(sum(v * v for v in acc))
        if not (sum64 and s >= 64):
            acc_cost += (sum((2 * c[6 * a + 2]) ** 2 for a in range(3))) * Ts
            jerk += jk
            sum_v += cnt[s] * vn
            sum_a += cnt[s] * an
            num += cnt[s]
        if cnt[s] and not (max64 and s >= 64):
            max_v, max_a = max(max_v, vn), max(max_a, an)
    return np.array([ts, length, jerk, sum_v / num, max_v, sum_a / num, max_a, acc_cost, float(len(times))]), out


def model_coefficients(T, Df, x, drop_half_A=False):
    """(m, 18) by the closed form of coefficients_kernel, in Python floats."""
    T = [float(v) for v in T]
    m = len(T)
    out = np.zeros((m, 18))
    d = twin.derivatives(m, Df, x)
    for s in range(m):
        for k in range(3):
            p0, v0, a0, pT, vT, aT = d(s, k)
            Ts = T[s]
            T2, iT = Ts * Ts, 1.0 / Ts
            iT3 = iT * iT * iT
            P = pT - p0 - v0 * Ts - 0.5 * a0 * T2
            V = (vT - v0 - a0 * Ts) * Ts
            A = (aT - a0) * T2
            half_A = 0.0 if drop_half_A else 0.5 * A
            out[s, 6 * k:6 * k + 6] = [p0, v0, 0.5 * a0, (10 * P - 4 * V + half_A) * iT3, (-15 * P + 7 * V - A) * (iT3 * iT),
                                       (6 * P - 3 * V + 0.5 * A) * (iT3 * iT * iT)]
    return out


def _verdict(stats, samples, smp, ref, cap, probe=False):
    """(passes, caught): passes = every exact quantity equal and every ratio within K; caught = an exact quantity
    differs or a ratio exceeds 4 K."""
    worst, bad = gp.compare_samples(samples, smp, cap)
    if probe:
        bad = bad + gp.compare_probe(samples, smp, cap)
    out, bad2 = gp.compare_stats(stats, ref)
    exact_diff = bool(bad or bad2)
    ratios = [(worst, gp.K_POINT)] + list(out.values())
    return (not exact_diff and all(r <= k for r, k in ratios)), (exact_diff or any(r > 4 * k for r, k in ratios))


def _case(key, case):
    T, dt, coeff = case
    smp, ref = gp.twin_of(key, coeff, T, dt)
    return T, dt, coeff, smp, ref, smp["n"] + 2


SEG_SENSITIVE = ("segments", 130, 64, 107)

TRAJECTORY_MUTANTS = [
    ("strict_boundary", ("probe", "binary"), dict(strict_boundary=True)),
    ("product_times", ("probe", "decimal"), dict(product_times=True)),
    ("maxima over the first 64 segments", SEG_SENSITIVE, dict(max64=True)),
    ("sums over the first 64 segments", SEG_SENSITIVE, dict(sum64=True)),
    ("carried point replaced by zero", ("chunk", 129), dict(carry0=True)),
]


def _input(key):
    if key[0] == "probe":
        return cases.probe(key[1])
    if key[0] == "chunk":
        return cases.chunk_case(key[1])
    return cases.segment_case(*key[1:])


@pytest.mark.parametrize("name,key,mut", TRAJECTORY_MUTANTS, ids=[t[0] for t in TRAJECTORY_MUTANTS])
def test_sensitivity_trajectory_mutants(name, key, mut):
    assert key != SEG_SENSITIVE or key[2:] in [tuple(a) for a in cases.arrangements(key[1])]
    T, dt, coeff, smp, ref, cap = _case(key, _input(key))
    probe = key[0] == "probe"
    ok, _ = _verdict(*model_trajectory(coeff, T, dt, cap), smp, ref, cap, probe)
    assert ok, "the unmutated model misses the bound"
    _, caught = _verdict(*model_trajectory(coeff, T, dt, cap, **mut), smp, ref, cap, probe)
    assert caught, f"{name}: not seen by the comparisons of the GPU test"


@pytest.mark.parametrize("switch", ["strict_boundary", "product_times"])
def test_sensitivity_twin_switches(switch):
    """The twin's own switches change an exact quantity of the probe: the reference they would be is not the one the
    kernel is held to."""
    key = ("probe", "binary" if switch == "strict_boundary" else "decimal")
    T, dt, coeff, smp, ref, cap = _case(key, _input(key))
    mutated = twin.samples(coeff, T, dt, **{switch: True})
    assert (mutated["idx"], mutated["tloc"]) != (smp["idx"], smp["tloc"])
    stats, samples = model_trajectory(coeff, T, dt, cap)         # the correct model fails against the mutated twin
    assert gp.compare_probe(samples, mutated, cap)


def test_sensitivity_row_reads_row_zero_times():
    T, dt, coeff = cases.batch_case(3)
    for b in (1, 2):
        smp, ref = gp.twin_of(("batch", 3, b), coeff[b], T[b], dt)
        cap = 160
        assert _verdict(*model_trajectory(coeff[b], T[b], dt, cap), smp, ref, cap)[0]
        assert _verdict(*model_trajectory(coeff[b], T[0], dt, cap), smp, ref, cap)[1]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("m", cases.COEF_M)
def test_sensitivity_dropped_half_A(m, shared):
    T, Df, x = cases.coef_case(m, shared)
    for b in range(cases.COEF_B):
        Tb = T if shared else T[b]
        ref = twin.coefficients(Tb, Df[b], x[b])
        assert gp.compare_coefficients(model_coefficients(Tb, Df[b], x[b]), ref) <= gp.K_COEF
        assert gp.compare_coefficients(model_coefficients(Tb, Df[b], x[b], drop_half_A=True), ref) > 4 * gp.K_COEF


def test_grid_stride_reference_subset():
    """The elements the grid-stride test solves exactly: all of the second pass, and the model within K on them."""
    T, Df, x = cases.grid_coef_case()
    m = cases.GRID_COEF_M
    b = cases.GRID_B - 1
    keys = [(s, a) for s in range(m - 4, m) for a in range(3)]
    got = model_coefficients(T, Df[b], x[b])
    assert gp.compare_coefficients(got, twin.coefficients(T, Df[b], x[b], only=keys)) <= gp.K_COEF
    assert cases.LANES // (3 * m) < cases.GRID_B - 1             # whole rows lie in the second pass
