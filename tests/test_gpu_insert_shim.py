"""GradTrajOptimizer::insertWaypoint (the C++ shim) through tests/cpp/insert_shim.cpp.  The solved state is what the
scene runner gives today; each insertion is the Python binding's gtop_insert_waypoints on the state before it, bit for
bit, and the coefficients follow the new problem; a refused call changes nothing; the optimizer then runs on the
problem of two segments more and ends no worse than it started."""
import json
import os
import subprocess

import numpy as np
import pytest

from grad_traj_optimization_amd import insert, problem
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_EVALS = 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_insert_waypoint_in_the_shim(gtop, tmp_path):
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)
    m = wp.shape[0] - 1
    obstacles = scenes.opti_node_obstacles()
    f = scenes.write_scene(tmp_path / "scene.txt", scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES,
                           obstacles, wp)
    exe = os.path.join(ROOT, "grad_traj_optimization_amd", "gtop_insert_shim")
    assert os.path.exists(exe), "build() did not produce gtop_insert_shim"
    run = subprocess.run([exe, str(f), str(MAX_EVALS)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    txt = run.stdout
    out = json.loads(txt[txt.index('{\n"solved"'):txt.rindex("}") + 1])
    solved, at, kept, longest, resolved = (out[k] for k in ("solved", "at_time", "after_refusal", "longest", "resolved"))
    assert all(s["ok"] == 1 for s in (solved, at, kept, longest, resolved)) and out["refused"] == 1
    today = scenes.run_scene(f, MAX_EVALS, on_device=1)
    assert np.array_equal(_bits(solved["x"]), _bits(today["x1"])) and np.array_equal(_bits(solved["coeff"]), _bits(today["coeff1"]))
    T0 = problem.segment_times(wp[None])[0]
    assert np.array_equal(_bits(solved["segment_time"]), _bits(T0))
    Df, _ = problem.initial_derivatives(wp[None])
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES)
        ctx.update_sdf_map(obstacles)
        ctx.set_params()
        lim = gtop.GtopLimits(margin=0.3)

        def state_follows(state, T, x, segments):
            ctx.set_problem(T[None], Df)
            coeff, _ = ctx.trajectory_stats(x[None])
            assert len(state["segment_time"]) == segments and len(state["x"]) == 9 * (segments - 1)
            assert np.allclose(np.array(state["coeff"]).reshape(segments, 18), coeff[0], rtol=1e-12, atol=1e-12)
            rep, _, _ = ctx.validate_batch(x[None], lim)
            assert np.array_equal(_bits(state["report"]), _bits(rep[0, [0, 1, 2, 11]]))
            return rep[0]

        x0 = np.array(solved["x"])
        rep0 = state_follows(solved, T0, x0, m)
        # the waypoint at the time of the least clearance
        x1, T1, _, _, info1 = insert.insert_waypoints(ctx, x0[None], gtop.GtopInsert(mode=0, min_fraction=0.1), when=[rep0[2]])
        assert np.array_equal(_bits(at["x"]), _bits(x1[0])) and np.array_equal(_bits(at["segment_time"]), _bits(T1[0]))
        assert np.array_equal(_bits(at["info"]), _bits(info1[0])) and info1[0, 2] == 0
        rep1 = state_follows(at, T1[0], x1[0], m + 1)
        # the same curve: as many samples (or one more or less at the very end), the clearance where it was
        assert abs(rep1[0] - rep0[0]) <= 1 and abs(rep1[1] - rep0[1]) < 1e-9 and abs(rep1[11] - rep0[11]) < 1e-12
        # the refused call changed nothing
        for k in ("x", "segment_time", "coeff", "report"):
            assert np.array_equal(_bits(kept[k]), _bits(at[k])), k
        # the longest segment, pushed
        opt = gtop.GtopInsert(mode=1, min_fraction=0.1, push=0.25, push_below=1.0)
        x2, T2, _, _, info2 = insert.insert_waypoints(ctx, x1, opt)
        assert np.array_equal(_bits(longest["x"]), _bits(x2[0])) and np.array_equal(_bits(longest["segment_time"]), _bits(T2[0]))
        assert np.array_equal(_bits(longest["info"]), _bits(info2[0]))
        assert info2[0, 0] == int(np.argmax(T1[0])) and info2[0, 1] == 0.5 * T1[0].max()
        state_follows(longest, T2[0], x2[0], m + 2)
        # the optimizer ran on m + 2 segments and moved the point
        assert len(resolved["segment_time"]) == m + 2 and np.array_equal(_bits(resolved["segment_time"]), _bits(T2[0]))
        x3 = np.array(resolved["x"])
        assert x3.shape == (9 * (m + 1),) and np.any(x3 != x2[0]) and np.all(np.isfinite(x3))
        state_follows(resolved, T2[0], x3, m + 2)
    finally:
        ctx.close()
