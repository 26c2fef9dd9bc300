"""GradTrajOptimizer::certifyKinematics (the C++ shim) through tests/cpp/kinematics_shim.cpp: the kinematic certificate of
the optimised trajectory is, bit for bit, the Python binding's certify_kinematics_batch at the same free derivatives;
the return value is `verdict == WITHIN`; a call before a path is set and one with bad options fail without a
certificate."""
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


def test_certify_kinematics_in_the_shim(gtop, tmp_path):
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)
    obstacles = scenes.opti_node_obstacles()
    f = scenes.write_scene(tmp_path / "scene.txt", scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES,
                           obstacles, wp)
    exe = os.path.join(ROOT, "grad_traj_optimization_amd", "gtop_kinematics_shim")
    assert os.path.exists(exe), "build() did not produce gtop_kinematics_shim"
    run = subprocess.run([exe, str(f), str(MAX_EVALS)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    txt = run.stdout
    out = json.loads(txt[txt.index('{\n"no_path"'):txt.rindex("}") + 1])
    assert out["no_path"] == {"within": 0, "ok": 0}
    assert out["bad_depth"]["within"] == 0 and out["bad_depth"]["ok"] == 0
    x = np.array(out["x"])
    T0 = problem.segment_times(wp[None])[0]
    Df, _ = problem.initial_derivatives(wp[None])
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.set_params()
        ctx.set_problem(T0[None], Df)
        for name, opts in (("off", (0.0, 0.0, False, 2, 256)), ("tight", (0.01, 0.01, False, 2, 256)),
                           ("generous", (100.0, 1000.0, True, 2, 256)), ("level0", (100.0, 0.0, False, 0, 0))):
            want = gtop.certify_kinematics_batch(ctx, x[None], gtop.GtopKinOpts(*opts), want_seg=False)[0][0]
            got = np.array(out[name]["kin"], dtype=np.float64)
            print(name, got)
            assert out[name]["ok"] == 1
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, got, want)
            assert out[name]["within"] == int(want[0] == 1)
        assert out["tight"]["kin"][0] == -1 and out["tight"]["within"] == 0       # no flight of this path keeps 1 cm/s
        assert out["generous"]["kin"][0] == 1 and out["generous"]["within"] == 1
        assert out["off"]["kin"][0] == 1 and out["off"]["kin"][9] == 0             # no limit: nothing to refine
        assert out["off"]["kin"][10] == sum(T0.tolist(), 0.0) and out["level0"]["kin"][9] == 0
        assert out["off"]["kin"][2] <= out["off"]["kin"][1] <= out["generous"]["kin"][1] * 3 ** 0.5 * (1 + 1e-9)
    finally:
        ctx.close()
