"""The trajectory report and the selection on the CPU: the C-ABI's new symbols and bindings, and the numpy restatement
(tests/validate_twin.py) tied to code that exists by identities — a brute-force argmin over the oracle's query at the
oracle's sample points, the static query, a shift of the boxes' clock, central differences of the oracle's sample
positions, and a hand-derived quintic (tests/golden/VALIDATE_ANALYTIC.md)."""
import ctypes

import numpy as np

from grad_traj_optimization_amd import problem
from tests import validate_twin as vt


def _scene(oracle_mod, grid=(48, 40, 24), density=0.04, B=6, m=6, seed=7):
    mp = problem.make_map(grid, density=density, seed=seed)
    b = problem.make_trajectories(B, m, mp, seed=seed + 1)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    return mp, b, sdf


def _boxes(b, rng, nbox, moving=True):
    """Boxes near the batch's own waypoints (so that they matter), 1 .. 2 m wide."""
    j = rng.integers(0, len(b.x), nbox)
    w = rng.integers(0, b.m + 1, nbox)
    p0 = b.waypoints[j, w] + rng.uniform(-0.3, 0.3, (nbox, 3))
    vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * (1.0, 1.0, 0.2) if moving else np.zeros((nbox, 3))
    scale = rng.uniform(1.0, 2.0, (nbox, 3))
    return p0, vel, scale


def test_symbols_bindings_and_abi_version(gtop):
    lib = ctypes.CDLL(gtop.library_path())
    for name in ("gtop_validate_trajectories_device", "gtop_select_best_device", "gtop_validate_batch"):
        assert hasattr(lib, name), name
        assert getattr(gtop.load_library(), name).argtypes is not None
    assert lib.gtop_abi_version() >= 5
    for name in ("validate_batch", "validate_device", "select_best_device"):
        assert hasattr(gtop.GtopContext, name), name
    lim = gtop.GtopLimits(margin=0.3, max_vel=2.0, per_axis=True, use_boxes=True)
    assert (lim.margin, lim.max_vel, lim.max_acc, lim.per_axis, lim.allow_out_of_map, lim.use_boxes) == (0.3, 2.0, 0.0, 1, 0, 1)
    assert ctypes.sizeof(lim) == 40 and len(gtop.GtopContext.TRAJ_REPORT) == 12


def test_twin_clearance_is_the_brute_force_argmin(oracle_mod):
    mp, b, sdf = _scene(oracle_mod)
    rng = np.random.default_rng(3)
    p0, vel, scale = _boxes(b, rng, 8)
    lowered = 0
    for i in range(len(b.x)):
        coeff = oracle_mod.coefficients(b.T[i], b.Df[i], b.x[i])
        t0 = 0.4 * i
        r, info = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3, p0, vel, scale, t0=t0, use_boxes=True)
        n, pts = oracle_mod.traj_samples(coeff, b.T[i], 0.01, 8192)
        assert r[0] == n == len(pts) and r[11] == oracle_mod.traj_stats(coeff, b.T[i])[0]
        best, best_k, below = None, -1, []
        for k in range(n):     # brute force, one query at a time
            d = sdf.edt_query(pts[k], t0 + info["t"][k], p0, vel, scale)[0][0]
            if best is None or d < best:
                best, best_k = d, k
            if d <= 0.3:
                below.append(k)
        assert (r[1], r[3], r[2]) == (best, best_k, info["t"][best_k]), i
        assert r[4] == len(below) and r[5] == (info["t"][below[0]] if below else -1.0) and r[6] == 0
        r_static, _ = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3)
        lowered += bool(r[1] < r_static[1])
    assert lowered >= 1, lowered    # the boxes matter somewhere in this batch


def test_twin_static_identities(oracle_mod):
    """tau < 0 for every sample, or no boxes: the static query getDistWithGradTrilinear at the same points."""
    mp, b, sdf = _scene(oracle_mod, B=4)
    rng = np.random.default_rng(5)
    p0, vel, scale = _boxes(b, rng, 8)
    for i in range(len(b.x)):
        coeff = oracle_mod.coefficients(b.T[i], b.Df[i], b.x[i])
        r0, info = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3)
        r1, _ = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3, p0, vel, scale, t0=-1e3, use_boxes=True)
        r2, _ = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3, t0=2.0, use_boxes=True)      # boxes asked for, none set
        r3, _ = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3, p0, vel, scale, t0=2.0, use_boxes=False)
        assert np.array_equal(r0, r1) and np.array_equal(r0, r2) and np.array_equal(r0, r3), i
        static = np.array([sdf.query(p)[0] for p in info["points"]])
        assert np.array_equal(static, info["dist"]) and r0[1] == static.min() and r0[3] == np.argmin(static)


def test_twin_clock_shift(oracle_mod):
    mp, b, sdf = _scene(oracle_mod, B=8)
    rng = np.random.default_rng(9)
    p0, vel, scale = _boxes(b, rng, 8)
    delta, changed = 1.75, 0
    for i in range(len(b.x)):
        coeff = oracle_mod.coefficients(b.T[i], b.Df[i], b.x[i])
        r1, i1 = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3, p0, vel, scale, t0=delta, use_boxes=True)
        r2, i2 = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3, p0 + vel * delta, vel, scale, t0=0.0, use_boxes=True)
        assert np.max(np.abs(i1["dist"] - i2["dist"])) <= 1e-11, i
        assert abs(r1[1] - r2[1]) <= 1e-11 and np.array_equal(r1[[0, 6, 7, 8, 9, 10, 11]], r2[[0, 6, 7, 8, 9, 10, 11]])
        r0, _ = vt.report(oracle_mod, coeff, b.T[i], sdf, 0.3)
        changed += bool(r1[1] < r0[1])
    assert changed >= len(b.x) // 4, changed


def test_twin_velocity_and_acceleration_against_central_differences(oracle_mod):
    """v_k ~ (p_{k+1} - p_{k-1}) / (t_{k+1} - t_{k-1}), a_k ~ (p_{k+1} - 2 p_k + p_{k-1}) / h^2 on the ORACLE's sample
    positions, for samples whose two neighbours lie in the same segment.  Step: the sampling step h = 0.01 itself.
    Tolerance, per sample and axis, from Taylor's theorem and the positions' rounding:
      velocity:      h^2/6  * M3 + 2 dp / (2h)      M3 >= max |p'''| on [t-h, t+h]
      acceleration:  h^2/12 * M4 + 4 dp / h^2       M4 >= max |p''''| there
    with M3, M4 the sums of the absolute values of the derivative's terms at |t| + h (an upper bound for a polynomial
    on the interval) and dp = 16 eps * sum_j |c_j| t^j a generous bound of one evaluated position's rounding error (6
    terms, pow() within an ulp); the accumulated sample times differ from multiples of h by ~1e-15 relative, which the
    velocity quotient uses as they are and the second difference ignores (covered by the factor 2 below)."""
    mp, b, sdf = _scene(oracle_mod, B=4, m=6, seed=11)
    h, eps = 0.01, np.finfo(np.float64).eps
    checked = 0
    for i in range(len(b.x)):
        coeff = oracle_mod.coefficients(b.T[i], b.Df[i], b.x[i])
        kin = vt.kinematics(coeff, b.T[i], h)
        n, pts = oracle_mod.traj_samples(coeff, b.T[i], h, 8192)
        assert n == len(kin["t"])
        c = coeff.reshape(-1, 3, 6)
        j = np.arange(6)
        for k in range(1, n - 1):
            s = kin["seg"][k]
            if kin["seg"][k - 1] != s or kin["seg"][k + 1] != s:
                continue
            u = abs(kin["loc"][k]) + h
            for ax in range(3):
                ca = np.abs(c[s, ax])
                m3 = sum(j[q] * (j[q] - 1) * (j[q] - 2) * ca[q] * u ** (q - 3) for q in range(3, 6))
                m4 = sum(j[q] * (j[q] - 1) * (j[q] - 2) * (j[q] - 3) * ca[q] * u ** (q - 4) for q in range(4, 6))
                dp = 16 * eps * sum(ca[q] * u ** q for q in range(6))
                v_fd = (pts[k + 1, ax] - pts[k - 1, ax]) / (kin["t"][k + 1] - kin["t"][k - 1])
                a_fd = (pts[k + 1, ax] - 2 * pts[k, ax] + pts[k - 1, ax]) / (h * h)
                assert abs(v_fd - kin["v"][k, ax]) <= 2 * (h * h / 6 * m3 + dp / h), (i, k, ax)
                assert abs(a_fd - kin["a"][k, ax]) <= 2 * (h * h / 12 * m4 + 4 * dp / (h * h)), (i, k, ax)
                checked += 1
    assert checked > 3000, checked


def test_twin_known_answer_quintic():
    """tests/golden/VALIDATE_ANALYTIC.md"""
    coeff = np.array([[0, 0, 0, 0, 0, 0.1, 1, 2, 0, 0, 0, 0, 0.5, 0, 0.5, 0, 0, 0]], dtype=np.float64)
    T = np.array([1.5])
    kin = vt.kinematics(coeff, T, 0.01)
    t = np.float64(0.0)
    while t + np.float64(0.01) <= 1.5:
        t = t + np.float64(0.01)
    assert kin["t"][-1] == t and len(kin["t"]) in (150, 151) and abs(t - 1.5) < 0.011
    r = vt.reduce_report(kin["t"], np.ones(len(kin["t"])), np.zeros(len(kin["t"]), dtype=bool), kin, 0.3)
    want = known_answer_quintic(t)
    assert np.all(np.abs(r[7:12] - want) <= 1e-12 * np.abs(want)), (r[7:12], want)
    assert r[0] == len(kin["t"]) and r[4] == 0 and r[5] == -1.0 and r[1] == 1.0 and r[3] == 0


def known_answer_quintic(t):
    """entries 7 .. 11 for the quintic of tests/golden/VALIDATE_ANALYTIC.md, t = the last sample's time"""
    return np.array([np.sqrt(t ** 8 / 4 + 4 + t * t), np.sqrt(4 * t ** 6 + 1), max(t ** 4 / 2, 2.0, t),
                     max(2 * t ** 3, 1.0), 1.5])


def test_selection_twin_against_a_loop():
    seen_none = seen_some = 0
    for name, rep, cost, lim in vt.selection_cases():
        ok, best = vt.select(rep, cost, **lim)
        ok2, best2 = vt.select_loop(rep, cost, **lim)
        assert np.array_equal(ok, ok2) and np.array_equal(best, best2), name
        assert best[1] == ok.sum()
        seen_none += best[0] == -1
        seen_some += best[0] >= 0
        if name == "ties":
            assert best[0] == 90 and ok[[90, 170, 250]].all() and not ok[40]
        if name == "nan and inf costs":
            assert not ok[[3, 5, 7]].any() and best[0] not in (3, 5, 7) and ok[:20].sum() == 17
        if name.startswith("nobody"):
            assert best[0] == -1 and best[1] == 0
    assert seen_none >= 3 and seen_some >= 8
    # each limit bites on its own, and switching it off restores the row count
    name, rep, cost, _ = vt.selection_cases()[0]
    base = vt.select(rep, cost)[1][1]
    assert vt.select(rep, cost, max_vel=3.0)[1][1] < base and vt.select(rep, cost, max_acc=4.0)[1][1] < base
    assert vt.select(rep, cost, max_vel=3.0, per_axis=True)[1][1] > vt.select(rep, cost, max_vel=3.0)[1][1]
    assert vt.select(rep, cost, allow_out_of_map=True)[1][1] > base


def test_report_kernels_use_no_scratch_memory(tmp_path):
    """The rule tests/test_capi.py asserts for the evaluation kernels, for csrc/gtop_validate.hip: no scratch and no
    VGPR spill, from the cross-compile alone (tools/kernel_resources.py, source=)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows, _ = kr.analyse(asm_out=str(tmp_path / "gtop_validate.s"), source="gtop_validate.hip")
    names = sorted(r["kernel"] for r in rows)
    assert names == ["select_finish_kernel", "select_kernel"] + [
        f"traj_report_kernel<{w}, {poly}>" for w in (1, 2, 4) for poly in ("false", "true")], names
    bad = [r for r in rows if r["scratch"] or r["vgpr_spill"]]
    assert not bad, bad
