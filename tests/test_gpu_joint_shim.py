"""GradTrajOptimizer::jointGradient and optimizeJoint (the C++ shim) through tests/cpp/joint_shim.cpp: the joint gradient
of the optimised trajectory is, bit for bit, the Python binding's joint_gradient_batch at the same free derivatives;
optimizeJoint gives optimize_joint's bits and replaces the object's Dp and segment times; a call before a path is set
and one with bad options fail and change nothing."""
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


def test_joint_gradient_and_joint_optimizer_in_the_shim(gtop, tmp_path):
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)
    obstacles = scenes.opti_node_obstacles()
    f = scenes.write_scene(tmp_path / "scene.txt", scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES,
                           obstacles, wp)
    exe = os.path.join(ROOT, "grad_traj_optimization_amd", "gtop_joint_shim")
    assert os.path.exists(exe), "build() did not produce gtop_joint_shim"
    run = subprocess.run([exe, str(f), str(MAX_EVALS)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    txt = run.stdout
    out = json.loads(txt[txt.index('{\n"no_path"'):txt.rindex("}") + 1])
    assert out["no_path"] == {"gradient": 0, "optimized": 0, "ok": 0}
    assert out["bad"] == {"optimized": 0, "ok": 0, "unchanged": 1}
    assert out["gradient_ok"] == 1 and out["optimized"] == 1
    x = np.array(out["x"])
    T0 = problem.segment_times(wp[None])[0]
    assert np.array_equal(np.array(out["T"]), T0)
    m = len(T0)
    Df, _ = problem.initial_derivatives(wp[None])
    lb, ub = gtop.GtopContext.default_bounds(wp[None])
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES)
        ctx.update_sdf_map(obstacles)
        ctx.set_params()
        ctx.set_problem(T0[None], Df)
        cost, gx, gT, parts = gtop.joint_gradient_batch(ctx, x[None])

        def same(a, b):
            a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
            return np.array_equal(a.view(np.uint64), b.view(np.uint64))

        assert same(out["cost"], cost) and same(out["gx"], gx[0]) and same(out["gT"], gT[0]) and same(out["parts"], parts[0])
        assert len(out["gT"]) == m and len(out["gx"]) == 9 * (m - 1) and len(out["parts"]) == 4 * m
        x_new, T_new, info = gtop.optimize_joint(ctx, gtop.GtopJointOpt(rho=2.0, max_evals=15), x[None], lb, ub)
        assert same(out["x_new"], x_new[0]) and same(out["T_new"], T_new[0]) and same(out["info"], info[0])
        assert info[0, 3] < info[0, 2] and info[0, 1] == 15 and not np.array_equal(T_new[0], T0)
        # the object's problem is the new point: its next gradient call ran there
        ctx.set_problem(T_new, Df)
        c_new, _, _, _ = gtop.joint_gradient_batch(ctx, x_new, want_parts=False)
        assert same(out["cost_at_new"], c_new) and same(out["cost_at_new"], info[0, 4:5])
    finally:
        ctx.close()
