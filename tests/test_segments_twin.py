"""The per-segment report and the segment-time reallocation on the CPU: the C-ABI's new symbols and bindings, and the
numpy twin (tests/segments_twin.py) tied to what exists — on the oracle's per-sample data (validate_twin.report) its
rows obey the laws include/gtop.h states against validate_twin.reduce_report; hand-made known answers for the reduction
and for both retime modes; and every deliberate mistake the twin can be asked to make is caught by those checks."""
import ctypes

import numpy as np
import pytest

from tests import segments_twin as st
from tests import validate_twin as vt
from tests.test_validate import _boxes, _scene


def test_symbols_bindings_and_abi_version(gtop):
    lib = ctypes.CDLL(gtop.library_path())
    L = gtop.load_library()
    for name, nargs in (("gtop_validate_segments_device", 10), ("gtop_validate_segments", 6),
                        ("gtop_reallocate_times_device", 11), ("gtop_reallocate_times", 7)):
        assert hasattr(lib, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == nargs, name
    assert lib.gtop_abi_version() >= 9
    for name in ("validate_segments", "validate_segments_device", "reallocate_times", "reallocate_times_device"):
        assert hasattr(gtop.GtopContext, name), name
    assert len(gtop.GtopContext.SEG_REPORT) == st.N_SEG == 10
    o = gtop.GtopRetime(mode=gtop.GtopRetime.LIMITS, max_vel=2.0, per_axis=True, scale_x=True, max_ratio=3.0)
    assert (o.mode, o.mean_v, o.init_time, o.max_vel, o.max_acc, o.per_axis, o.uniform, o.scale_x, o.max_ratio) == \
        (1, 1.8, 0.3, 2.0, 0.0, 1, 0, 1, 3.0)
    assert ctypes.sizeof(o) == 64          # int32 + pad, 4 doubles, 3 int32 + pad, 1 double
    # without a context every entry refuses (GTOP_ERR_INVALID) before it touches anything
    assert L.gtop_validate_segments_device(None, 1, 6, None, None, 6, 0.01, None, None, None) == 1
    assert L.gtop_validate_segments(None, 1, None, 0.01, None, None) == 1
    assert L.gtop_reallocate_times_device(None, None, 1, 6, None, None, None, 6, None, None, None) == 1
    assert L.gtop_reallocate_times(None, None, 1, None, 0.01, None, None) == 1


# ---- the reduction on the oracle's per-sample data ----
def _segments_of(info, m, margin, mutant=None):
    return st.reduce_segments(m, info["t"], info["seg"], info["dist"], info["out"], info["v"], info["a"], margin,
                              mutant=mutant)


def test_twin_obeys_the_laws_on_the_oracles_samples(oracle_mod):
    mp, b, sdf = _scene(oracle_mod)
    p0, vel, scale = _boxes(b, np.random.default_rng(3), 8)
    failing = passing = lowered = 0
    for i in range(len(b.x)):
        coeff = oracle_mod.coefficients(b.T[i], b.Df[i], b.x[i])
        rows = {}
        for use_boxes in (False, True):
            R, info = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3, p0, vel, scale, t0=0.4 * i, use_boxes=use_boxes)
            t, seg = st.segment_of_samples(b.T[i])
            assert np.array_equal(t, info["t"]) and np.array_equal(seg, info["seg"])      # the walk, restated
            S = _segments_of(info, b.m, 0.3)
            assert st.check_laws(S, R) == [], (i, use_boxes)
            rows[use_boxes] = S
            failing += np.count_nonzero(S[:, 4] > 0)
            passing += np.count_nonzero((S[:, 4] == 0) & (S[:, 0] > 0))
        lowered += np.count_nonzero(rows[True][:, 2] < rows[False][:, 2])
        assert np.array_equal(rows[True][:, [0, 1, 6, 7, 8, 9]], rows[False][:, [0, 1, 6, 7, 8, 9]])
    assert failing > 0 and passing > 0 and lowered > 0, (failing, passing, lowered)


def test_twin_obeys_the_laws_with_segments_shorter_than_the_step(oracle_mod):
    """Segment times below dt_sample: segments without a sample, a run of two, and an empty last-but-one segment."""
    mp, b, sdf = _scene(oracle_mod, B=2)
    T = np.array([1.003, 0.003, 0.003, 0.505, 0.002, 0.8])
    coeff = oracle_mod.coefficients(T, b.Df[0], b.x[0])
    R, info = vt.report(oracle_mod, coeff, T, sdf, 0.3)
    S = _segments_of(info, 6, 0.3)
    assert S[:, 0].tolist() == [101, 0, 0, 51, 0, 80]
    assert np.array_equal(S[[1, 2, 4]], np.tile(st.EMPTY_ROW, (3, 1))) and S[:, 1].tolist() == [0, -1, -1, 101, -1, 152]
    assert st.check_laws(S, R) == []


# ---- hand-made known answers ----
HAND_T = np.array([0.025, 0.003, 0.03, 0.02])     # samples 0 .. 2 | none | 3 .. 5 | 6, 7


def _hand_rows(mutant=None):
    t, seg = st.segment_of_samples(HAND_T, 0.01, mutant=mutant)
    assert len(t) == 8
    dist = np.array([1.0, 0.3, 0.5, 0.3, 0.2, 0.2, -1.0, 0.9])
    oom = dist == -1.0
    v = np.array([[k, 0.0, 0.0] for k in range(8)]) * [1.0, 0, 0] + [0.0, 3.0, -4.0]      # |v|^2 = k^2 + 25
    a = np.array([[0.0, -2.0 * k, 1.0] for k in range(8)])
    return t, seg, st.reduce_segments(4, t, seg, dist, oom, v, a, 0.3, mutant=mutant)


def test_hand_made_reduction():
    t, seg, S = _hand_rows()
    assert seg.tolist() == [0, 0, 0, 2, 2, 2, 3, 3]
    want = np.array([[3, 0, 0.3, t[1], 1, 0, np.sqrt(29.0), np.sqrt(17.0), 4.0, 4.0],
                     st.EMPTY_ROW,
                     [3, 3, 0.2, t[4], 3, 0, np.sqrt(50.0), np.sqrt(101.0), 5.0, 10.0],
                     [2, 6, -1.0, t[6], 1, 1, np.sqrt(74.0), np.sqrt(197.0), 7.0, 14.0]])
    assert np.array_equal(S, want), (S, want)


def _boundary_counts(mutant=None):
    """T = [0.02, 0.02]: the sample at 0.01 + 0.01 == 0.02 lies exactly on the boundary and belongs to segment 1;
    the last segment is extended to the sample at time_sum."""
    t, seg = st.segment_of_samples(np.array([0.02, 0.02]), 0.01, mutant=mutant)
    assert t[2] == 0.02
    return np.bincount(seg, minlength=2).tolist()


def test_a_boundary_sample_belongs_to_the_later_segment():
    assert _boundary_counts()[0] == 2 and sum(_boundary_counts()) >= 4


HAND_X = np.array([3.0, 0.5, -0.25, 3.0, 1.5, 0.75,          # x: positions 3, 3; (v, a) of the two junctions
                   4.0, -1.0, 2.0, 4.0, 0.25, -0.5,
                   0.0, 2.0, 1.0, 12.0, -3.0, 4.0])
HAND_DF = np.array([0.0, 0, 0, 6.0, 0, 0, 0.0, 0, 0, 8.0, 0, 0, 0.0, 0, 0, 12.0, 0, 0])


def test_hand_made_length_mode():
    """(0,0,0) -> (3,4,0) -> (3,4,12) -> (6,8,12): lengths 5, 12, 5."""
    assert st.retime_length(3, HAND_X, HAND_DF, 2.0, 0.25).tolist() == [2.75, 6.0, 2.75]
    assert st.retime_length(3, HAND_X, HAND_DF, 2.0, 0.0).tolist() == [2.5, 6.0, 2.5]


def _hand_seg():
    S = np.tile(st.EMPTY_ROW, (3, 1))                 # the last segment has no sample: V = A = 0
    S[0, [0, 1, 6, 7, 8, 9]] = [10, 0, 2.0, 1.0, 1.5, 0.5]
    S[1, [0, 1, 6, 7, 8, 9]] = [10, 10, 4.0, 9.0, 3.0, 6.0]
    return S


def test_hand_made_limits_mode():
    T = np.array([1.0, 2.0, 0.004])
    S = _hand_seg()
    # velocity alone: ratios 1, 2, 1
    T1, x1 = st.retime_limits(3, HAND_X, T, S, max_vel=2.0)
    assert T1.tolist() == [1.0, 4.0, 0.004] and np.array_equal(x1, HAND_X)
    # acceleration alone: sqrt(9 / 4) = 1.5
    T2, _ = st.retime_limits(3, HAND_X, T, S, max_acc=4.0)
    assert T2.tolist() == [1.0, 3.0, 0.004]
    # both, max_ratio biting
    T3, _ = st.retime_limits(3, HAND_X, T, S, max_vel=2.0, max_acc=4.0, max_ratio=1.25)
    assert T3.tolist() == [1.0, 2.5, 0.004]
    # per axis: 3 / 2 against sqrt(6 / 4)
    T4, _ = st.retime_limits(3, HAND_X, T, S, max_vel=2.0, max_acc=4.0, per_axis=True)
    assert T4.tolist() == [1.0, 3.0, 0.004]
    # limits switched off (<= 0): nothing moves, bit for bit, whatever the other switches say
    for kw in (dict(), dict(max_vel=0.0, max_acc=-1.0, uniform=True, scale_x=True)):
        T5, x5 = st.retime_limits(3, HAND_X, T, S, **kw)
        assert np.array_equal(T5, T) and np.array_equal(x5, HAND_X)
    # uniform: every segment takes 2; scale_x: both junctions touch the stretched segment, rho = 2
    T6, x6 = st.retime_limits(3, HAND_X, T, S, max_vel=2.0, uniform=True, scale_x=True)
    assert T6.tolist() == [2.0, 4.0, 0.008]
    want = HAND_X.copy().reshape(3, 6)
    want[:, [1, 4]] /= 2.0
    want[:, [2, 5]] /= 4.0
    assert np.array_equal(x6, want.reshape(-1))
    # not uniform: the same x (rho = max(1, 2) at both junctions), the first and last time kept
    T7, x7 = st.retime_limits(3, HAND_X, T, S, max_vel=2.0, scale_x=True)
    assert T7.tolist() == [1.0, 4.0, 0.004] and np.array_equal(x7, x6)
    assert np.array_equal(x7.reshape(3, 6)[:, [0, 3]], HAND_X.reshape(3, 6)[:, [0, 3]])       # positions never move


def test_bounds_of_velocity_and_acceleration_over_a_curve():
    """acc_bound / vel_bound dominate the sampled derivatives of a random quintic."""
    rng = np.random.default_rng(2)
    coeff = rng.normal(size=(3, 18))
    T = np.array([0.7, 1.3, 0.9])
    kin = vt.kinematics(coeff, T, 0.01)
    assert np.abs(kin["a"]).max() <= st.acc_bound(coeff, T) and np.abs(kin["v"]).max() <= st.vel_bound(coeff, T)
    assert st.acc_bound(coeff, T) <= 40 * np.abs(kin["a"]).max()          # and are not vacuous


@pytest.mark.parametrize("mutant", st.MUTANTS)
def test_mutants_are_caught(mutant):
    T = np.array([1.0, 2.0, 0.004])
    if mutant == "strict_margin":            # `<` for `<=`: the sample AT the margin
        assert _hand_rows(mutant)[2][0, 4] == 0 != _hand_rows()[2][0, 4]
        t, seg, S = _hand_rows(mutant)
        R = np.zeros(12)
        R[[0, 1, 2, 3, 4, 6]] = [8, -1.0, t[6], 6, 5, 1]
        R[7:11] = [np.sqrt(74.0), np.sqrt(197.0), 7.0, 14.0]
        assert st.check_laws(S, R) == ["samples below the margin"] and st.check_laws(_hand_rows()[2], R) == []
    elif mutant == "boundary_to_earlier":
        assert _boundary_counts(mutant)[0] == 3 != _boundary_counts()[0]
    elif mutant == "init_time_first_only":
        assert st.retime_length(3, HAND_X, HAND_DF, 2.0, 0.25, mutant=mutant).tolist() == [2.75, 6.0, 2.5]
    elif mutant == "no_sqrt_acc":
        assert st.retime_limits(3, HAND_X, T, _hand_seg(), max_acc=4.0, mutant=mutant)[0].tolist() == [1.0, 4.5, 0.004]
    elif mutant == "rho_min":
        _, x = st.retime_limits(3, HAND_X, T, _hand_seg(), max_vel=2.0, scale_x=True, mutant=mutant)
        assert np.array_equal(x, HAND_X)         # min(1, 2) = 1 at both junctions: nothing rescaled, which the known answer refutes
    else:
        raise AssertionError(mutant)


def test_segment_and_retime_kernels_use_no_scratch_memory(tmp_path):
    """The rule tests/test_validate.py asserts for csrc/gtop_validate.hip, for the two new files: no scratch and no
    VGPR spill, from the cross-compile alone (tools/kernel_resources.py, source=)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    for source, want in (("gtop_segments.hip", ["traj_segments_kernel<false>", "traj_segments_kernel<true>"]),
                         ("gtop_retime.hip", ["retime_length_kernel", "retime_limits_kernel"])):
        rows, _ = kr.analyse(asm_out=str(tmp_path / (source + ".s")), source=source)
        assert sorted(r["kernel"] for r in rows) == want, rows
        bad = [r for r in rows if r["scratch"] or r["vgpr_spill"]]
        assert not bad, bad
