"""The moving-obstacle cost on the CPU: the C-ABI's new symbols, and the independent restatement (tests/moving_twin.py)
tied to the existing cost path by identities that need no new code under test — no boxes, parked boxes (a static field
F' = min(F, box distance)), and a shift of the boxes' clock."""
import ctypes
import os

import numpy as np

from grad_traj_optimization_amd import problem
from oracle import np_twin
from tests import moving_twin, scenes

PARAMS = dict(ws=1.0, wc=5.0, alpha=10.0, r=0.5, d0=0.8, alpha_v=0.0, r_v=1.5, v0=2.5, alpha_a=0.0, r_a=1.5, a0=3.5,
              step=2, enable_dyn=0)


def _scene(oracle_mod, B=16, m=6, seed=7):
    mp = problem.make_map((48, 40, 24), density=0.04, seed=seed)
    b = problem.make_trajectories(B, m, mp, seed=seed + 1)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    return mp, b, sdf


def _np_sdf(mp, sdf, field=None):
    f = sdf.dist.reshape(sdf.grid) if field is None else field
    return np_twin.Sdf(mp.origin, mp.resolution, sdf.grid, f, max_range=np.array(sdf.c.max_range[:]))


def _boxes(b, rng, nbox, moving=True):
    """Boxes near the batch's own waypoints (so that they matter), 1 .. 2 m wide."""
    j = rng.integers(0, len(b.x), nbox)
    w = rng.integers(0, b.m + 1, nbox)
    p0 = b.waypoints[j, w] + rng.uniform(-0.3, 0.3, (nbox, 3))
    vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * (1.0, 1.0, 0.2) if moving else np.zeros((nbox, 3))
    scale = rng.uniform(1.0, 2.0, (nbox, 3))
    return p0, vel, scale


def test_symbols_and_abi_version(gtop):
    lib = ctypes.CDLL(gtop.library_path())
    for name in ("gtop_set_moving_cost", "gtop_get_moving_cost", "gtop_set_start_times", "gtop_set_start_times_device"):
        assert hasattr(lib, name), name
    assert lib.gtop_abi_version() >= 4
    for name in ("set_moving_cost", "moving_cost", "set_start_times", "set_start_times_device"):
        assert hasattr(gtop.GtopContext, name), name
    assert gtop.GtopContext.MOVING_COST_MAX_BOXES >= 32


def test_twin_without_boxes_is_the_static_evaluation(oracle_mod):
    mp, b, sdf = _scene(oracle_mod)
    nps = _np_sdf(mp, sdf)
    prm = oracle_mod.make_params(**PARAMS)
    none = np.zeros((0, 3))
    rng = np.random.default_rng(3)
    p0, vel, scale = _boxes(b, rng, 8)
    for i in range(len(b.x)):
        c_np, g_np, _ = np_twin.cost_grad(b.T[i], b.Df[i], b.x[i], nps, PARAMS)
        c_or, g_or = oracle_mod.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, prm)
        # no boxes; and boxes, but every tau < 0 (static only, src/edt_environment.cpp:91-94)
        for boxes, t0 in ((( none, none, none), 0.0), ((p0, vel, scale), -1e3)):
            c, g, info = moving_twin.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, PARAMS, *boxes, t0=t0)
            assert not info["lowered"].any()
            assert c == c_np and np.array_equal(g, g_np), i
            assert scenes.rel_err(c, g, c_or, g_or) <= (1e-12, 1e-12), i


def test_twin_with_parked_boxes_is_the_static_evaluation_on_the_min_field(oracle_mod):
    mp, b, sdf = _scene(oracle_mod)
    rng = np.random.default_rng(5)
    p0, vel, scale = _boxes(b, rng, 8, moving=False)
    Fp = moving_twin.parked_field(sdf, p0, scale)
    assert (Fp < sdf.dist.reshape(sdf.grid)).any()
    nps = _np_sdf(mp, sdf, Fp)
    sdf_p = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf_p.dist[:] = Fp.reshape(-1)
    prm = oracle_mod.make_params(**PARAMS)
    n = np.array(sdf.grid)
    changed = 0
    for i in range(len(b.x)):
        c, g, info = moving_twin.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, PARAMS, p0, vel, scale, t0=0.7 * i)
        # (the two lookups could differ only where a base index clamps: none does, with the batch's 1 m margin)
        assert np.all(info["base_idx"] >= 0) and np.all(info["base_idx"] <= n - 2), i
        c_np, g_np, _ = np_twin.cost_grad(b.T[i], b.Df[i], b.x[i], nps, PARAMS)
        assert c == c_np and np.array_equal(g, g_np), i
        c_or, g_or = oracle_mod.cost_grad(b.T[i], b.Df[i], b.x[i], sdf_p, prm)
        assert scenes.rel_err(c, g, c_or, g_or) <= (1e-12, 1e-12), i
        c_st, _ = oracle_mod.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, prm)
        changed += bool(info["lowered"].any() and abs(c - c_st) > 1e-6 * abs(c_st))
    assert changed >= len(b.x) // 2, changed   # the boxes matter: this is not the static evaluation on F


def test_twin_clock_shift(oracle_mod):
    mp, b, sdf = _scene(oracle_mod)
    rng = np.random.default_rng(9)
    p0, vel, scale = _boxes(b, rng, 8)
    delta = 1.75
    changed = 0
    for i in range(len(b.x)):
        c1, g1, info = moving_twin.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, PARAMS, p0, vel, scale, t0=delta)
        c2, g2, _ = moving_twin.cost_grad(b.T[i], b.Df[i], b.x[i], sdf, PARAMS, p0 + vel * delta, vel, scale, t0=0.0)
        assert scenes.rel_err(c1, g1, c2, g2) <= (1e-11, 1e-11), i
        changed += bool(info["lowered"].any())
    assert changed >= len(b.x) // 4, changed


def test_sample_times_are_the_callbacks_own():
    """The tau list walks the callback's loop: as many entries as np_twin.cost_grad takes samples, tiny segments
    included (the sample count hangs on the accumulated time, src/grad_traj_optimizer.cpp:353)."""
    T = np.array([0.9, 0.02, 1.3, 0.0301])
    taus = moving_twin.sample_times(T, 2.0)
    n = 0
    for s in range(len(T)):
        t, dt = 1e-3, T[s] / 30.0
        while t < T[s]:
            n += 1
            t += dt
    assert len(taus) == n
    assert taus[0] == 2.0 + 1e-3 and np.all(np.diff(taus) > 0)
    assert os.path.exists(os.path.join(os.path.dirname(__file__), "moving_twin.py"))
