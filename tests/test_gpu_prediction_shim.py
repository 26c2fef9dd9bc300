"""GradTrajOptimizer::fitObstaclePredictions (the C++ shim) through tests/cpp/predict_fit_shim.cpp on the reference's own
scene with two observed objects that cross the path: the info rows it returns are the host fit's, bit for bit (and the
twin's); the report with the fitted boxes in force equals the Python binding's after set_moving_box_polynomials with
the fit's coef, t_range and inflated extents; a list with an empty history is refused and changes nothing."""
import json
import os
import subprocess

import numpy as np
import pytest

from grad_traj_optimization_amd import prediction as gp
from grad_traj_optimization_amd import problem
from tests import predict_twin as pt
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("mode", [pt.POLYFIT, pt.CONST_VEL])
def test_fit_obstacle_predictions_in_the_shim(gtop, tmp_path, mode):
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)
    f = scenes.write_scene(tmp_path / "scene.txt", scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES,
                           scenes.opti_node_obstacles(), wp)
    t_start = 1.5
    T = problem.segment_times(wp[None])[0]
    when = t_start + np.array([T[:3].sum(), T[:7].sum()])       # each object is over its waypoint when the trajectory is
    rng = np.random.default_rng(17)
    vel, acc = np.array([(0.6, -0.4, 0.0), (-0.5, 0.3, 0.05)]), np.array([(0.4, 0.3, 0.0), (-0.3, 0.5, 0.05)])
    counts, H = (9, 14), 14
    hist = np.zeros((2, H, 4))
    for b in range(2):
        t = np.sort(rng.uniform(when[b] - 2.5, when[b] - 0.6, counts[b]))
        u = (t - when[b])[:, None]
        hist[b, :counts[b], :3] = wp[[3, 7][b]] + vel[b] * u + 0.5 * acc[b] * u * u + 0.02 * rng.normal(size=(counts[b], 3))
        hist[b, :counts[b], 3] = t
    scale = np.array([(1.2, 1.0, 1.5), (1.0, 1.4, 1.1)])
    kw = dict(degree=4, lam=0.2, horizon=2.0, inflate=1.25, regularise_horizon=1)
    with open(f, "a") as out:
        out.write("start_time %.17g\nhistories 2\n" % t_start)
        for b in range(2):
            out.write("%d\n" % counts[b])
            for i in range(counts[b]):
                out.write(" ".join("%.17g" % v for v in hist[b, i]) + "\n")
            out.write(" ".join("%.17g" % v for v in scale[b]) + "\n")
    exe = os.path.join(ROOT, "grad_traj_optimization_amd", "gtop_predict_fit_shim")
    assert os.path.exists(exe), "build() did not produce gtop_predict_fit_shim"
    args = [mode, kw["degree"], kw["lam"], kw["horizon"], kw["inflate"], kw["regularise_horizon"]]
    run = subprocess.run([exe, str(f), *(repr(v) for v in args)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    txt = run.stdout
    res = json.loads(txt[txt.index('{"report_static_pass"'):txt.rindex("}") + 1])

    opts = gp.GtopPredictOpts(mode=mode, degree=kw["degree"], lambda_=kw["lam"], horizon=kw["horizon"],
                              inflate=kw["inflate"], regularise_horizon=kw["regularise_horizon"])
    coef, t_range, info, _ = gp.fit_predictions(hist, counts, opts)
    twin = pt.fit(hist, counts, None, mode=mode, degree=kw["degree"], lam=kw["lam"], horizon=kw["horizon"],
                  regularise_horizon=kw["regularise_horizon"])
    assert np.array_equal(bits(info), bits(twin[2])) and np.array_equal(bits(coef), bits(twin[0]))
    assert np.all(info[:, 0] <= pt.LOWERED) and info[:, 6:9].max() > 1e-3
    got_info = np.array(res["info"], dtype=np.float64).reshape(2, 12)
    assert np.array_equal(bits(got_info), bits(info))           # the host fit's bits
    assert res["refused"] == 1 and res["refused_last"][0] == pt.EMPTY
    assert res["report_after_refusal"] == res["report_static"]  # the refused list changed nothing

    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES)
        ctx.update_sdf_map(scenes.opti_node_obstacles())
        Df, _ = problem.initial_derivatives(wp[None])
        ctx.set_problem(np.array(res["segment_times"])[None], Df)
        ctx.set_start_times(t_start)
        x = np.array(res["x"])[None]
        lim = gtop.GtopLimits(margin=0.3, use_boxes=True)
        static, ok_static, _ = ctx.validate_batch(x, lim, cost=np.zeros(1))
        ctx.set_moving_box_polynomials(coef, 2.0 * pt.half_extents(scale, kw["inflate"], info), t_range)
        report, ok, _ = ctx.validate_batch(x, lim, cost=np.zeros(1))
        assert np.array_equal(bits(np.array(res["report_static"])), bits(static[0]))
        assert np.array_equal(bits(np.array(res["report"])), bits(report[0]))
        assert res["report_pass"] == int(ok[0]) and res["report_static_pass"] == int(ok_static[0])
        assert report[0, 1] < static[0, 1]                      # the fitted boxes are in the shim's report
    finally:
        ctx.close()
