#!/usr/bin/env python3
"""What the minimum-jerk start point (gtop_min_jerk_start_device) costs and what it buys.  No threshold is set for
either: the tool writes down what comes out.

(1) Device-clock time of one launch, between two one-lane stamp kernels (gtop_device_clock_stamp, as bench.py times
    its region), for B x m = 1024 x 6, 16384 x 6, 8192 x 40 and 1 x 227 — beside one gtop_eval_device launch (fp64) of
    the same shape from the same process.  200^3 map, random-walk waypoints inside it.
(2) The device optimizer (gtop_optimize_device, default bounds) on the scene of tests/scenes.py (the opti_node scene:
    two walls, 11 waypoints) from the straight-line start and from the minimum-jerk start of the same waypoints: the
    cost at the start (after the optimizer's clamp into its box the start may differ: the cost given is the
    evaluation's at the unclamped point) and the best cost after 10, 25 and 50 evaluations, in both gradient modes.

usage: tools/minjerk_time.py [--out profiles/min_jerk]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1024, 6), (16384, 6), (8192, 40), (1, 227))
EVALS = (10, 25, 50)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_jerk"))
    a = ap.parse_args()

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import problem
    from tests import minjerk_plan, scenes

    dev = torch.device("cuda:0")
    ctx = gtop.GtopContext(0)
    hz = ctx.clock_hz()
    init = torch.tensor([2 ** 63 - 1, 0], dtype=torch.int64, device=dev)
    stamps = init.clone()

    def span(fn, reps):
        """us per call of fn over `reps` back-to-back calls, by the device clock; sustained clocks first."""
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.05:
            fn()
            torch.cuda.synchronize()
        best = None
        for _ in range(5):
            stamps.copy_(init)
            ctx.clock_stamp(stamps)
            for _ in range(reps):
                fn()
            ctx.clock_stamp(stamps)
            torch.cuda.synchronize()
            st = stamps.tolist()
            us = (st[1] - st[0]) / hz * 1e6 / reps
            best = us if best is None else min(best, us)
        return best

    # ---- (1) launch times
    mp = problem.make_map(200, density=0.02, seed=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    ctx.set_params()
    times = []
    for B, m in SHAPES:
        b = problem.make_trajectories(B, m, mp, seed=1, boundary="random")
        x, Df, T = (torch.tensor(v, device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T))
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        grad = torch.empty_like(x)
        reps = 20 if B * m <= 8192 else 5
        plan = minjerk_plan.plan(B, m)
        t_mj = span(lambda: ctx.min_jerk_start_device(x, Df, T), reps)     # (in place: a repeated call reads the same positions)
        t_ev = span(lambda: ctx.eval_device(x, Df, T, cost, grad), reps)
        times.append(dict(B=B, m=m, lanes_per_workgroup=plan["lanes"], workgroups=plan["blocks"], lds_bytes=plan["lds_bytes"],
                          min_jerk_us=t_mj, eval_us=t_ev))
        print(f"B = {B} m = {m}: min-jerk {t_mj:.1f} us, eval {t_ev:.1f} us", flush=True)

    # ---- (2) the two starts under the optimizer
    ctx.init_sdf_map(scenes.OPTI_NODE_MAP_SIZE, scenes.OPTI_NODE_ORIGIN, scenes.OPTI_NODE_RES)
    ctx.update_sdf_map(scenes.opti_node_obstacles())
    wp = np.asarray(scenes.OPTI_NODE_PATH, dtype=np.float64)[None]
    T, Df, x_line = ctx.setup_paths_device(torch.tensor(wp, device=dev))
    x_jerk = ctx.min_jerk_start_device(x_line.clone(), Df, T)
    lb, ub = (torch.tensor(v, device=dev) for v in gtop.GtopContext.default_bounds(wp))
    torch.cuda.synchronize()
    out_of_box = int(((x_jerk < lb) | (x_jerk > ub)).sum().item())
    scene_rows = []
    for mode_name, consistent in (("reference", False), ("consistent", True)):
        ctx.set_gradient_mode(consistent)
        for name, x0 in (("straight line", x_line), ("minimum jerk", x_jerk)):
            c0, _ = ctx.eval_device(x0, Df, T)
            row = dict(scene="opti_node", gradient=mode_name, start=name, cost_at_start=float(c0.cpu()[0]))
            for k in EVALS:
                _, cmin = ctx.optimize_device(x0.clone(), Df, T, lb, ub, k)
                torch.cuda.synchronize()
                row[f"best_after_{k}"] = float(cmin.cpu()[0])
            scene_rows.append(row)
            print(row, flush=True)
    ctx.set_gradient_mode(False)
    ctx.close()

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "minjerk_time.json"), "w") as f:
        json.dump(dict(launch_times=times, scenes=scene_rows, min_jerk_entries_outside_the_default_box=out_of_box), f, indent=1)
    with open(os.path.join(a.out, "minjerk_time.md"), "w") as f:
        f.write("fp64; device-clock spans (gtop_device_clock_stamp around back-to-back launches, minimum of 5 spans), one "
                "process; 200^3 map, random-walk waypoints, boundary velocity and acceleration non-zero\n\n")
        f.write("| B x m | lanes per workgroup | workgroups | LDS per workgroup, B | min-jerk launch, us | one gtop_eval_device launch, us | min-jerk / eval |\n")
        f.write("|---|---|---|---|---|---|---|\n")
        for t in times:
            f.write(f"| {t['B']} x {t['m']} | {t['lanes_per_workgroup']} | {t['workgroups']} | {t['lds_bytes']} | "
                    f"{t['min_jerk_us']:.1f} | {t['eval_us']:.1f} | {t['min_jerk_us'] / t['eval_us']:.3f} |\n")
        f.write("\nThe two starts under the device optimizer (gtop_optimize_device, default bounds bos 3 / vos 8 / aos 10, "
                "the launch file's parameters) on the scene of tests/scenes.py; cost at the start as the evaluation "
                f"gives it; {out_of_box} of the minimum-jerk start's entries lie outside the default box and are clamped "
                "by the optimizer.  No threshold: rows where the straight line ends lower are what they are.\n\n")
        f.write("| scene | gradient | start | cost at start | " + " | ".join(f"best after {k}" for k in EVALS) + " |\n")
        f.write("|---|---|---|---|" + "---|" * len(EVALS) + "\n")
        for r in scene_rows:
            f.write(f"| {r['scene']} | {r['gradient']} | {r['start']} | {r['cost_at_start']:.6g} | "
                    + " | ".join(f"{r[f'best_after_{k}']:.6g}" for k in EVALS) + " |\n")


if __name__ == "__main__":
    main()
