"""The kinematic certificate without a GPU: the companion header's symbols and binding table, the frozen surface of
include/gtop.h beside them, and the numpy twin (tests/kinematics_twin.py) held to the rule's own properties.

(1) Leaf-wise soundness: for every leaf, the largest of each figure over 201 evenly spaced times of the leaf, ends
    included, is <= the leaf's upper bound.  The dense figures carry a rounding error of a few eps of the Horner sums,
    2^-12 of the 2^-40 slack the bounds include.
(2) The hand-made cubic, whose velocity bound at level-0 interval 32 is carried by the remainder term alone.
(3) Mutants of the twin, each caught by the check named for it in CAUGHT_BY.
(4) The rows the device tests run with a limit come out as those tests expect, in the twin alone; so does the
    composition with the LIMITS reallocation.
(5) The kernel uses no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kinematics_twin as kt
from tests import segments_twin as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_certify_kinematics_device", "gtop_certify_kinematics_batch", "gtop_select_best_kin_certified_device")


# ---- the surface ----
def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import kinematics as gk
    L = gk.kin_library()
    assert L.gtop_kin_abi_version() == 1 == gk.KIN_ABI_VERSION == gtop.KIN_ABI_VERSION
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_kin_abi_version"} <= exported
    for name in ("GtopKinOpts", "KIN_REPORT", "KIN_SEG", "KIN_ENTRY_POINTS", "certify_kinematics_device",
                 "certify_kinematics_batch", "select_best_kin_certified_device"):
        assert hasattr(gtop, name) and name in gtop.__all__, name
    assert (gk.EXCEEDS, gk.UNDECIDED, gk.WITHIN) == (-1, 0, 1)
    assert len(gk.KIN_REPORT) == 11 and len(gk.KIN_SEG) == 10 == len(gtop.GtopContext.SEG_REPORT)
    o = gk.GtopKinOpts()
    assert (o.max_vel, o.max_acc, o.per_axis, o.max_depth, o.max_refine, o.reserved) == (0.0, 0.0, 0, 2, 256, 0)


def test_binding_table_covers_the_header(gtop):
    import ctypes as C
    from grad_traj_optimization_amd import kinematics as gk
    text = open(os.path.join(ROOT, "include", "gtop_kinematics.h")).read()
    body = text[text.index("#ifndef GTOP_KINEMATICS_H_"):]
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gk.KIN_ENTRY_POINTS) == set(NAMES) | {"gtop_kin_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gk.KIN_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # the struct as the header lays it out: two doubles and four 32-bit words
    assert C.sizeof(gk.GtopKinOpts) == 32
    assert [f[0] for f in gk.GtopKinOpts._fields_] == ["max_vel", "max_acc", "per_axis", "max_depth", "max_refine", "reserved"]
    for macro, value in (("GTOP_KIN_ABI_VERSION", 1), ("GTOP_KIN_REPORT", 11), ("GTOP_KIN_SEG", 10)):
        assert re.search(rf"^#define {macro} {value}$", body, flags=re.M), macro


def test_the_surface_of_gtop_h_is_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert not [n for n in _abi.ENTRY_POINTS if "kin_" in n or "kinematics" in n]
    text = open(os.path.join(ROOT, "include", "gtop.h")).read()
    assert "kinematics" not in text and "gtop_kin" not in text and "GTOP_KIN" not in text
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    declared = set(re.findall(r"\b(gtop_[a-z0-9_]+)\(", code))
    assert len(declared) == 108 and declared == set(_abi.ENTRY_POINTS)


# ---- the rule's own properties, as named checks ----
def dense_of_leaf(c, a, w, n=201):
    return kt.figures(c, a + w * (np.arange(n) / (n - 1.0))).max(axis=0)


def failed_checks(coeff, T, max_vel, max_acc, per_axis, max_depth=2, max_refine=256, mutant=None):
    """The names of the checks one certificate of the twin (or of a mutant of it) fails."""
    c3 = np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6)
    kin, seg, info = kt.certify(coeff, T, max_vel, max_acc, per_axis, max_depth, max_refine, mutant=mutant)
    leaves, bad = info["leaves"], set()
    iv, ia = (2, 3) if per_axis else (0, 1)
    # leaf_sound: a leaf's bound holds at every time of the leaf
    for s, a, w, ub, _ in leaves:
        if np.any(dense_of_leaf(c3[s], a, w) > ub):
            bad.add("leaf_sound")
    # tiling: the leaves of a segment tile [0, Ts] — each starts where the one before it ends
    for s in range(len(T)):
        mine = sorted((a, w) for ss, a, w, _, _ in leaves if ss == s)
        ends = [a + w for a, w in mine]
        if mine[0][0] != 0.0 or abs(ends[-1] - T[s]) > 1e-12 * T[s] or any(
                abs(mine[i + 1][0] - ends[i]) > 1e-12 * T[s] for i in range(len(mine) - 1)):
            bad.add("tiling")
    # ub_over_leaves: a segment's bounds are the largest over its leaves, violating ones included — no more, no less
    for s in range(len(T)):
        want = np.max([ub for ss, _, _, ub, _ in leaves if ss == s], axis=0)
        if not np.array_equal(seg[s, 6:10], want):
            bad.add("ub_over_leaves")
    # lo_every_level: lo is at least the figure at the midpoint of every leaf, of whatever level
    for s, a, w, _, _ in leaves:
        if np.any(kt.figures(c3[s], np.array([a + 0.5 * w]))[0] > seg[s, 2:6]):
            bad.add("lo_every_level")
    # chosen_figure: the row's bounds are the segments' in the columns per_axis names, and bound the dense figure
    dense = kt.dense_max(coeff, T).max(axis=0)
    if not (kin[1] == seg[:, 6 + iv].max() and kin[4] == seg[:, 6 + ia].max() and kin[2] == seg[:, 2 + iv].max()
            and kin[5] == seg[:, 2 + ia].max() and kin[1] >= dense[iv] and kin[4] >= dense[ia]):
        bad.add("chosen_figure")
    # laws: lo <= ub; WITHIN means the bound keeps every active limit; the counts add up
    if not (np.all(seg[:, 2:6] <= seg[:, 6:10]) and kin[2] <= kin[1] and kin[5] <= kin[4]
            and seg[:, 1].sum() == kin[9]
            and (kin[0] != 1 or ((max_vel <= 0 or kin[1] <= max_vel) and (max_acc <= 0 or kin[4] <= max_acc)))):
        bad.add("laws")
    return bad


ROWS = [(m, b) for m in (2, 3, 7) for b in range(3)]


@pytest.fixture(scope="module")
def rows():
    return {m: kt.random_rows(3, m, 100 + m) for m in (2, 3, 7)}


@pytest.mark.parametrize("m,b", ROWS)
def test_leafwise_soundness_and_laws_on_random_quintics(rows, m, b):
    coeff, T = rows[m][0][b], rows[m][1][b]
    dense = kt.dense_max(coeff, T).max(axis=0)
    for per_axis in (False, True):
        iv, ia = (2, 3) if per_axis else (0, 1)
        for fv, fa in ((0.0, 0.0), (1.001, 1.001), (0.8, 0.0), (0.0, 1.0001), (1.0001, 0.9)):
            assert not failed_checks(coeff, T, fv * dense[iv], fa * dense[ia], per_axis), (m, b, per_axis, fv, fa)


def test_the_cubic_needs_the_remainder_term():
    coeff, T = kt.cubic_row()
    assert not failed_checks(coeff, T, 0.0, 0.0, False)
    _, _, info = kt.certify(coeff, T)
    (leaf,) = [lf for lf in info["leaves"] if lf[0] == 0 and lf[1] == 0.5]
    c = coeff.reshape(2, 3, 6)[0]
    v_mid, a_mid, _ = kt.derivatives(c[0], np.float64(65.0 / 128.0))
    assert a_mid == 0.0                                                      # the first-order term vanishes
    v_end = kt.derivatives(c[0], np.array([0.5, 0.515625]))[0]
    assert np.all(v_end == 1.2265625) and v_mid + 0.5 * 6.0 * (1.0 / 128.0) ** 2 == 1.2265625   # exactly
    assert 1.2265625 <= leaf[3][0] <= 1.2265625 * (1 + 2.0 ** -36)            # the bound holds, by the slack alone


# mutant -> (the check that catches it, the case: row, limits as factors of the dense maxima, per_axis)
CAUGHT_BY = {
    "no_remainder": ("leaf_sound", "cubic", (0.0, 0.0), False),
    "child32": ("tiling", (3, 0), (1.000001, 0.0), False),
    "ub_all": ("ub_over_leaves", (3, 0), (1.000001, 0.0), False),
    "ub_no_viol": ("ub_over_leaves", (3, 1), (0.8, 0.0), False),
    "lo_level0": ("lo_every_level", (3, 0), (1.000001, 0.0), False),
    "swap_axis": ("chosen_figure", (3, 2), (0.0, 0.0), False),
}


@pytest.mark.parametrize("mutant", kt.MUTANTS)
def test_every_mutant_is_caught_by_its_check(rows, mutant):
    check, case, (fv, fa), per_axis = CAUGHT_BY[mutant]
    coeff, T = kt.cubic_row() if case == "cubic" else (rows[case[0]][0][case[1]], rows[case[0]][1][case[1]])
    dense = kt.dense_max(coeff, T).max(axis=0)
    assert not failed_checks(coeff, T, fv * dense[0], fa * dense[1], per_axis)
    assert check in failed_checks(coeff, T, fv * dense[0], fa * dense[1], per_axis, mutant=mutant), mutant


# ---- the rows of the device tests ----
@pytest.mark.parametrize("B,m,seed", kt.BATCHES)
def test_rows_with_a_limit_are_decided_as_the_device_tests_expect(B, m, seed):
    coeff, T = kt.random_rows(B, m, seed)
    max_vel, max_acc, dense = kt.batch_limits(coeff, T)
    for per_axis, mv, ma in ((False, max_vel, max_acc), (True, max_vel, 0.0)):
        kin, _, _ = kt.certify_rows(coeff, T, mv, ma, per_axis)
        want = [kt.expected_verdict(coeff[b], T[b], mv, ma, per_axis) for b in range(B)]
        print(B, m, per_axis, "verdicts", np.bincount((kin[:, 0] + 1).astype(int), minlength=3), "free", want.count(None))
        for b in range(B):
            assert want[b] is None or kin[b, 0] == want[b], (b, kin[b], want[b], dense[b])
        assert np.count_nonzero(kin[:, 0] == 0) <= B // 10
        if B == 1:
            assert want == [1] and kin[0, 0] == 1           # the row chosen to be WITHIN, at max_depth 2


@pytest.mark.parametrize("B,m,seed", kt.COMPOSITION)
def test_composition_with_the_limits_reallocation_is_within_in_the_twin(oracle_mod, B, m, seed):
    """coefficients -> certificate (seg) -> LIMITS, uniform, scale_x on seg -> coefficients -> certificate against
    max_vel (1 + 2^-20): WITHIN, in numpy alone.  A uniform stretch by lambda of a rest-to-rest row divides the velocity
    by lambda exactly, up to rounding: the stretched curve's true maximum is at most max_vel, and the factor leaves the
    rounding of the stretch and of the new coefficients (1e-13 relative at worst) a margin of 1e-6."""
    wp, T, Df, x = kt.rest_to_rest_problem(B, m, seed)
    max_vel, stretched = kt.COMPOSITION_MAX_VEL, 0
    for b in range(B):
        coeff = oracle_mod.coefficients(T[b], Df[b], x[b])
        kin, seg, _ = kt.certify(coeff, T[b], max_vel)
        T2, x2 = st.retime_limits(m, x[b], T[b], seg, max_vel=max_vel, uniform=True, scale_x=True,
                                  max_ratio=kt.COMPOSITION_MAX_RATIO)
        assert np.all(T2 < kt.COMPOSITION_MAX_RATIO * T[b])
        stretched += bool(np.all(T2 > T[b])) and kin[0] == -1
        coeff2 = oracle_mod.coefficients(T2, Df[b], x2)
        kin2, _, _ = kt.certify(coeff2, T2, max_vel * (1.0 + 2.0 ** -20))
        assert kin2[0] == 1 and kin2[1] <= max_vel * (1.0 + 2.0 ** -20), (b, kin2)
    print(B, m, "rows stretched", stretched)
    assert stretched >= B // 2


def test_the_kernel_uses_no_scratch(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows, _ = kernel_resources.analyse(asm_out=str(tmp_path / "kin.s"), source="gtop_kinematics.hip")
    assert [r["kernel"] for r in rows] == ["traj_kinematics_kernel"]
    print(rows)
    assert rows[0]["scratch"] == 0 and rows[0]["vgpr_spill"] == 0
