"""GradTrajOptimizer::timeGradientMoving and optimizeSegmentTimesMoving (the C++ shim) through
tests/cpp/timeopt_moving_shim.cpp: without boxes they give timeGradient's numbers; with a box set (the mode on)
timeGradient refuses and the segment-time gradient of the optimised trajectory is, bit for bit, the Python binding's
time_gradient_moving_batch at the same free derivatives; optimizeSegmentTimesMoving gives optimize_times_moving's bits
and replaces the object's segment times; a call before a path is set and one with bad options fail and change nothing."""
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
T0_START = 0.4


def test_time_gradient_and_time_optimizer_under_a_box_in_the_shim(gtop, tmp_path):
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)
    obstacles = scenes.opti_node_obstacles()
    f = scenes.write_scene(tmp_path / "scene.txt", scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES,
                           obstacles, wp)
    T0 = problem.segment_times(wp[None])[0]
    m = len(T0)
    # one box that reaches waypoint 2 when the trajectory does, across its course
    vel = np.array([-0.3, 0.4, 0.0])
    p0 = wp[2] - vel * (T0_START + T0[:2].sum())
    scale = np.array([0.8, 0.8, 1.0])
    exe = os.path.join(ROOT, "grad_traj_optimization_amd", "gtop_timeopt_moving_shim")
    assert os.path.exists(exe), "build() did not produce gtop_timeopt_moving_shim"
    args = [exe, str(f), str(MAX_EVALS), repr(T0_START)] + [repr(float(v)) for v in (*p0, *vel, *scale)]
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    txt = run.stdout
    out = json.loads(txt[txt.index('{\n"no_path"'):txt.rindex("}") + 1])
    assert out["no_path"] == {"gradient": 0, "optimized": 0, "ok": 0}
    assert out["bad"] == {"optimized": 0, "ok": 0, "unchanged": 1}
    assert out["static_same"] == 1 and out["static_refused"] == 1
    assert out["gradient_ok"] == 1 and out["optimized"] == 1
    x = np.array(out["x"])
    assert np.array_equal(np.array(out["T"]), T0)
    Df, _ = problem.initial_derivatives(wp[None])
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES)
        ctx.update_sdf_map(obstacles)
        ctx.set_params()
        ctx.set_problem(T0[None], Df)
        ctx.set_moving_boxes(p0[None], vel[None], scale[None])
        ctx.set_moving_cost(True)
        ctx.set_start_times(T0_START)
        cost, gT, gt0, parts = gtop.time_gradient_moving_batch(ctx, x[None])

        def same(a, b):
            a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
            return np.array_equal(a.view(np.uint64), b.view(np.uint64))

        assert same(out["cost"], cost) and same(out["gT"], gT[0]) and same(out["parts"], parts[0]) and same(out["gt0"], gt0)
        assert len(out["gT"]) == m and len(out["parts"]) == 6 * m
        assert gt0[0] != 0.0 and np.any(parts[0, :, 5] != 0.0)              # the box is felt
        T_new, info = gtop.optimize_times_moving(ctx, gtop.GtopTimeOpt(rho=2.0, max_evals=30), x[None])
        assert same(out["T_new"], T_new[0]) and same(out["info"], info[0])
        assert info[0, 4] <= info[0, 3] and info[0, 1] >= 1 and not np.array_equal(T_new[0], T0)
        # the object's problem is the new times: its next gradient call ran on them
        ctx.set_problem(T_new, Df)
        c_new, _, _, _ = gtop.time_gradient_moving_batch(ctx, x[None], want_parts=False)
        assert same(out["cost_at_T_new"], c_new) and same(out["cost_at_T_new"], info[0, 5:6])
    finally:
        ctx.close()
