"""The consistent gradient mode on the CPU (include/gtop.h, gtop_set_gradient_mode): the C-ABI's new symbols, and the
numpy restatement with a mode argument (tests/consistent_twin.py) — tied to the C oracle in mode 0, and in mode 1 to
what "consistent" claims: finite differences of the cost, exact zeros on idle axes, and a hand-derived known answer
(tests/golden/CONSISTENT_ANALYTIC.md)."""
import ctypes
import os
import re

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from oracle import np_twin
from tests import consistent_twin as ct
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(ws=1.0, wc=5.0, alpha=10.0, r=0.5, d0=0.8, alpha_v=0.0, r_v=1.5, v0=2.5, alpha_a=0.0, r_a=1.5, a0=3.5,
              step=2, enable_dyn=0)
DYN = dict(enable_dyn=1, alpha_v=2.0, r_v=0.5, v0=1.0, alpha_a=1.5, r_a=1.0, a0=1.0)
NAMES = ("gtop_set_gradient_mode", "gtop_get_gradient_mode", "gtop_group_set_gradient_mode")


def test_header_declares_the_gradient_mode():
    src = open(os.path.join(ROOT, "include", "gtop.h")).read()
    assert re.search(r"#define GTOP_GRADIENT_REFERENCE\s+0\b", src) and re.search(r"#define GTOP_GRADIENT_CONSISTENT\s+1\b", src)
    assert re.search(r"int gtop_set_gradient_mode\(gtop_ctx \*ctx, int mode\);", src)
    assert re.search(r"int gtop_get_gradient_mode\(const gtop_ctx \*ctx, int \*mode\);", src)
    assert re.search(r"int gtop_group_set_gradient_mode\(gtop_group \*g, int mode\);", src)
    shim = open(os.path.join(ROOT, "grad_traj_optimization_amd", "csrc", "grad_traj_optimizer.hpp")).read()
    assert re.search(r"int gradient_mode = 0;", shim)


def test_symbols_bindings_and_abi_version(gtop):
    lib = ctypes.CDLL(gtop.library_path())
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.gtop_abi_version() >= 6
    assert hasattr(gtop.GtopContext, "set_gradient_mode") and isinstance(gtop.GtopContext.gradient_mode, property)
    assert hasattr(gtop.GtopGroup, "set_gradient_mode")
    assert (gtop.GtopContext.GRADIENT_REFERENCE, gtop.GtopContext.GRADIENT_CONSISTENT) == (0, 1)


def test_entry_points_refuse_a_null_object(gtop):
    """(An invalid mode on a live context: tests/test_gpu_consistent_gradient.py — a context needs a device.)"""
    lib = gtop.load_library()
    mode = ctypes.c_int(7)
    assert lib.gtop_set_gradient_mode(None, 1) == 1
    assert lib.gtop_get_gradient_mode(None, ctypes.byref(mode)) == 1 and mode.value == 7
    assert lib.gtop_group_set_gradient_mode(None, 1) == 1


def _scene(oracle_mod, B=10, m=5, seed=21):
    mp = problem.make_map((48, 40, 24), density=0.04, seed=seed)
    b = problem.make_trajectories(B, m, mp, seed=seed + 1, boundary="random")
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    return b, sdf


@pytest.mark.parametrize("extra", [dict(), DYN, dict(DYN, step=1)], ids=["plain", "dyn", "dyn-step1"])
def test_twin_mode0_is_the_oracle_and_mode1_keeps_the_cost(oracle_mod, extra):
    """Mode 0 against the C oracle at the level the README states for the restatements; mode 1's cost bit for bit."""
    b, sdf = _scene(oracle_mod)
    p = dict(PARAMS, **extra)
    prm = oracle_mod.make_params(**p)
    differ = 0
    for i in range(len(b.x)):
        c_or, g_or = oracle_mod.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, prm)
        c0, g0, _ = ct.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, p, ct.REFERENCE)
        assert scenes.rel_err(c0, g0, c_or, g_or) <= (1e-12, 1e-12), i
        c1, g1, _ = ct.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, p, ct.CONSISTENT)
        assert c1 == c0, i
        differ += bool(np.max(np.abs(g1 - g0)) > 1e-3 * np.max(np.abs(g0)))
    assert differ >= len(b.x) // 2, differ   # (rows near obstacles: the modes are not the same function)


class LinearField:
    """dist = a + b . p everywhere: what trilinear interpolation of such voxel values returns exactly."""
    a, b = 1.5, np.array([0.05, -0.03, 0.04])

    def query(self, pos):
        return self.a + float(self.b @ np.asarray(pos)), self.b.copy()


def _fd_path(m=4, seed=0):
    """A gently curving path at about 1.8 m/s with non-zero velocity at both ends: the `1e-5` of vel_norm biases the
    quotient vel/vel_norm by 1e-5/|v| of that term, so no sample may sit at rest."""
    rng = np.random.default_rng(seed)
    d = np.array([1.0, 0.4, 0.2])
    d /= np.linalg.norm(d)
    wp = np.zeros((m + 1, 3))
    for i in range(1, m + 1):
        wp[i] = wp[i - 1] + 1.8 * d + rng.uniform(-0.3, 0.3, 3)
    T = np.linalg.norm(np.diff(wp, axis=0), axis=1) / 1.8
    v = 1.8 * d
    Df, x = np.zeros((3, 6)), np.zeros((3, 3 * m - 3))
    for k in range(3):
        Df[k] = [wp[0, k], v[k] + 0.1 * rng.standard_normal(), 0.3 * rng.standard_normal(),
                 wp[m, k], v[k] + 0.1 * rng.standard_normal(), 0.3 * rng.standard_normal()]
        for w in range(1, m):
            x[k, 3 * (w - 1):3 * w] = [wp[w, k], v[k] + 0.2 * rng.standard_normal(), 0.5 * rng.standard_normal()]
    return T, Df, x.reshape(-1)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("extra", [dict(), dict(DYN, alpha=0.0)], ids=["collision", "dyn-alpha0"])
def test_mode1_is_the_derivative_of_the_cost_and_mode0_is_not(monkeypatch, extra, seed):
    """Central differences (h = 1e-6) of the returned cost with the float round trips switched off, on a linear field:
    mode 1 within 1e-5 of the gradient's max-norm (the bias of vel_norm's 1e-5 is bounded by 1e-5/|v| of one term),
    mode 0 off by at least 1e-3 on the same scene."""
    monkeypatch.setattr(ct, "to_float", lambda v: v)
    T, Df, x = _fd_path(4, seed)
    p = dict(PARAMS, **extra)
    sdf, gen, h = LinearField(), np_twin.generator(T), 1e-6
    fd = np.zeros_like(x)
    for j in range(len(x)):
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        fd[j] = (ct.cost_grad(T, Df, xp, sdf, p, gen=gen)[0] - ct.cost_grad(T, Df, xm, sdf, p, gen=gen)[0]) / (2 * h)
    dev = []
    for mode in (ct.REFERENCE, ct.CONSISTENT):
        _, g, _ = ct.cost_grad(T, Df, x, sdf, p, mode, gen=gen)
        dev.append(np.max(np.abs((g - ct.GRAD_EPS) - fd)) / np.max(np.abs(fd)))
    print(f"finite differences: mode 0 off by {dev[0]:.2e}, mode 1 by {dev[1]:.2e} of the max-norm")
    assert dev[1] <= 1e-5, dev
    assert dev[0] >= 1e-3, dev


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_idle_axes_of_an_axis_aligned_path_get_no_push(axis):
    """A straight path along one axis, accelerating, dyn on: velocity and acceleration of the other two axes are
    exactly zero at every sample, and sgn(+-0) = 0 leaves the block's contribution to their entries exactly 0 — where
    the reference's gradient (no sign factor) pushes them."""
    m = 4
    T = np.array([0.9, 1.1, 1.0, 0.8])
    tau = np.r_[0.0, np.cumsum(T)]
    Df, x = np.zeros((3, 6)), np.zeros((3, 3 * m - 3))
    for k in range(3):
        p0 = (0.5, -0.25, 1.5)[k]
        if k == axis:
            st = [(p0 + 1.2 * t + 0.15 * t * t, 1.2 + 0.3 * t, 0.3) for t in tau]
        else:
            st = [(p0, 0.0, 0.0)] * (m + 1)
        Df[k] = list(st[0]) + list(st[m])
        for w in range(1, m):
            x[k, 3 * (w - 1):3 * w] = st[w]
    p = dict(PARAMS, **DYN)
    _, _, info1 = ct.cost_grad(T, Df, x.reshape(-1), LinearField(), p, ct.CONSISTENT)
    _, _, info0 = ct.cost_grad(T, Df, x.reshape(-1), LinearField(), p, ct.REFERENCE)
    idle = [k for k in range(3) if k != axis]
    assert np.all(info1["g_dyn"][idle] == 0.0)
    assert np.abs(info1["g_dyn"][axis]).max() > 0.0
    assert np.abs(info0["g_dyn"][idle]).max() > 1e-3   # (the case tells the modes apart)


def analytic_case():
    z = np.load(os.path.join(ROOT, "tests", "golden", "consistent_analytic.npz"))
    p = dict(zip((str(k) for k in z["pkeys"]), (float(v) for v in z["D_params"])))
    p["step"], p["enable_dyn"] = int(p["step"]), int(p["enable_dyn"])
    return z, p


def test_hand_derived_known_answer():
    """tests/golden/CONSISTENT_ANALYTIC.md, case D (constant acceleration along x, alpha = 0, dyn on), at the 1e-7 the
    derivation states; mode 0 misses it."""
    z, p = analytic_case()

    class Const:
        def query(self, pos):
            return 1.3, np.zeros(3)

    c, g, info = ct.cost_grad(z["D_T"], z["D_Df"], z["D_x"], Const(), p, ct.CONSISTENT)
    assert scenes.rel_err(c, g, float(z["D_cost"]), z["D_grad"]) <= (1e-7, 1e-7)
    # the idle axes: nothing from the block (what is left beside the offset of :425-432 is the jerk term's rounding)
    assert np.all(info["g_dyn"][1:] == 0.0) and np.all(z["D_grad"][len(g) // 3:] == 1e-5)
    c0, g0, _ = ct.cost_grad(z["D_T"], z["D_Df"], z["D_x"], Const(), p, ct.REFERENCE)
    assert c0 == c and scenes.rel_err(c0, g0, float(z["D_cost"]), z["D_grad"])[1] > 1e-2


def test_twin_takes_the_timed_lookup(oracle_mod):
    """tests/moving_twin.TimedLookup plugs into the twin as into np_twin.cost_grad: without boxes the moving-cost
    evaluation is the static one, in both modes."""
    from tests import moving_twin
    b, sdf = _scene(oracle_mod, B=3)
    none = np.zeros((0, 3))
    for i in range(len(b.x)):
        for mode in (ct.REFERENCE, ct.CONSISTENT):
            look = moving_twin.TimedLookup(sdf, moving_twin.sample_times(b.T[i], 0.5), none, none, none)
            c, g, _ = ct.cost_grad(b.T[i], b.Df[i], b.x[i], look, PARAMS, mode)
            c_s, g_s, _ = ct.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, PARAMS, mode)
            assert c == c_s and np.array_equal(g, g_s)


def test_consistent_bodies_use_no_scratch_memory(tmp_path):
    """tests/test_capi.py's build-time check on the consistent-gradient object (csrc/gtop_kernels.hip — the bodies of
    csrc/gtop_wave_kernel.h — compiled with -DGTOP_CONSISTENT_TU): no body spills, every body has a collision term, the latency body keeps its two wavefronts
    per SIMD, and nothing names a hand-issued load's registers before the wait that covers it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    asm = str(tmp_path / "gtop_kernels_consistent.s")
    rows, _ = kr.analyse(extra=("-DGTOP_CONSISTENT_TU",), asm_out=asm)
    assert len(rows) >= 60
    assert all("GtopConsistent<" in r["kernel"] for r in rows), [r["kernel"] for r in rows if "GtopConsistent<" not in r["kernel"]]
    bad = [r for r in rows if r["scratch"] or r["vgpr_spill"]]
    assert not bad, bad
    hot = [r for r in rows
           if r["kernel"].startswith("gtop_eval_wave_kernel<double, false, 3, 1, true, 2, GtopConsistent<GtopNoMma>, false, false, 1>")]
    assert len(hot) == 1 and hot[0]["waves_per_simd"] == 2, hot
    seen, violations = kr.check_asm_loads(asm)
    assert seen >= 12 and not violations, violations[:5]
