"""GradTrajOptimizer::Config::reallocate_time, segmentReport and reallocateSegmentTime (the C++ shim) through
tests/cpp/retime_shim.cpp.  With reallocate_time = 0 every output is what the scene runner gives today; with 1 the
solve is the same and getSegmentTime() holds the LENGTH-mode times of gtop_reallocate_times for the same free
derivatives, the coefficients follow them; the per-segment report and the limit-driven reallocation are the Python
binding's on the same inputs."""
import json
import os
import subprocess

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_EVALS = 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_reallocate_time_in_the_shim(gtop, tmp_path):
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)
    m = wp.shape[0] - 1
    obstacles = scenes.opti_node_obstacles()
    f = scenes.write_scene(tmp_path / "scene.txt", scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES,
                           obstacles, wp)
    exe = os.path.join(ROOT, "grad_traj_optimization_amd", "gtop_retime_shim")
    assert os.path.exists(exe), "build() did not produce gtop_retime_shim"
    run = subprocess.run([exe, str(f), str(MAX_EVALS)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    txt = run.stdout
    out = json.loads(txt[txt.index('{\n"reallocate0"'):txt.rindex("}") + 1], parse_int=float)
    r0, r1, lim_state = out["reallocate0"], out["reallocate1"], out["limits"]
    assert r0["ok"] == r1["ok"] == lim_state["ok"] == 1
    # reallocate_time = 0: what the scene runner gives today, bit for bit
    today = scenes.run_scene(f, MAX_EVALS, on_device=1)
    T0 = problem.segment_times(wp[None])[0]
    assert np.array_equal(_bits(r0["segment_time"]), _bits(today["segment_time"]))
    assert np.array_equal(_bits(r0["segment_time"]), _bits(T0))
    assert np.array_equal(_bits(r0["x"]), _bits(today["x1"])) and np.array_equal(_bits(r0["coeff"]), _bits(today["coeff1"]))
    # reallocate_time = 1: the same solve, then the block
    x1 = np.array(r1["x"])
    assert np.array_equal(_bits(x1), _bits(r0["x"]))
    Df, _ = problem.initial_derivatives(wp[None])
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES)
        ctx.update_sdf_map(obstacles)
        ctx.set_params()
        ctx.set_problem(T0[None], Df)
        limits = gtop.GtopLimits(margin=0.3)
        T_len, _ = ctx.reallocate_times(x1[None], gtop.GtopRetime(mode=gtop.GtopRetime.LENGTH, mean_v=1.8, init_time=0.3))
        assert np.array_equal(_bits(r1["segment_time"]), _bits(T_len[0]))
        assert not np.array_equal(_bits(T_len[0]), _bits(T0))
        S0 = ctx.validate_segments(x1[None], limits)
        assert np.array_equal(_bits(r0["segments"]), _bits(S0.reshape(-1)))
        # the limit-driven form on the first run's state
        opt = gtop.GtopRetime(mode=gtop.GtopRetime.LIMITS, max_vel=out["max_vel"], scale_x=True, max_ratio=4.0)
        assert out["max_vel"] == 0.8 * S0[0, :, 6].max()
        T_lim, x_lim = ctx.reallocate_times(x1[None], opt, limits)
        assert np.array_equal(_bits(lim_state["segment_time"]), _bits(T_lim[0]))
        assert np.array_equal(_bits(lim_state["x"]), _bits(x_lim[0]))
        assert np.any(T_lim[0] > T0) and np.any(x_lim[0] != x1)
        # the coefficients and the report follow the new times
        for state, T, x in ((r1, T_len, x1[None]), (lim_state, T_lim, x_lim)):
            ctx.set_problem(T, Df)
            coeff, _ = ctx.trajectory_stats(x)
            assert np.allclose(np.array(state["coeff"]).reshape(m, 18), coeff[0], rtol=1e-12, atol=1e-12)
            assert np.array_equal(_bits(state["segments"]), _bits(ctx.validate_segments(x, limits).reshape(-1)))
        assert not np.allclose(np.array(r1["coeff"]), np.array(r0["coeff"]))
    finally:
        ctx.close()
