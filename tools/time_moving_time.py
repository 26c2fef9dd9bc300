#!/usr/bin/env python3
"""Device time of the segment-time entry points under the moving-obstacle cost (include/gtop_time_moving.h), at B
trajectories of m = 6 segments on a random map with 1, 8 and 32 constant-velocity boxes, beside what they stand next to
on the same build and in the same run:

  static_gradient   gtop_time_gradient_device, the mode off (once per batch size: it reads no boxes)
  moving_gradient   gtop_time_gradient_moving_device, the mode on
  moving_eval       gtop_eval_device, the mode on, the same boxes
  moving_optimize   one gtop_optimize_times_moving_device of exactly 20 evaluations; also given per evaluation

Device times are spans of the device's own clock between two one-lane stamp kernels (gtop_device_clock_stamp) around
`reps` back-to-back launches, never host timers: the least of five spans per round, and the rounds' least and greatest
of that (tools/timeopt_time.py's method).  The optimizer is held to 20 evaluations by stop tolerances of zero; the
evaluations it used are read back and recorded.  The boxes start at waypoints of the rows and drift at up to 0.5 m/s.
It appends one JSON line per measurement to <out>/time_moving_time.jsonl, writes <out>/time_moving_time.md, and reads
nothing but what it generates from a seed.

usage: tools/time_moving_time.py [--batches 1024,16384] [--boxes 1,8,32] [--rounds 3] [--out profiles/time_moving]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, EVALS = 6, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,16384")
    ap.add_argument("--boxes", default="1,8,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_moving"))
    a = ap.parse_args()

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import problem

    mp = problem.make_map((100, 100, 40), density=0.03, seed=7)
    ctx = gtop.GtopContext(0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    dev = torch.device("cuda:0")
    hz = ctx.clock_hz()
    init = torch.tensor([2 ** 63 - 1, 0], dtype=torch.int64, device=dev)
    stamps = init.clone()

    def span(fn, reps):
        """us per call of fn over `reps` back-to-back calls, by the device clock; sustained clocks first."""
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.2:
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

    os.makedirs(a.out, exist_ok=True)
    rows = []

    def record(what, B, nbox, fn, reps, **extra):
        us = [span(fn, reps) for _ in range(a.rounds)]
        row = dict(what=what, B=B, m=M, boxes=nbox, us_min=min(us), us_max=max(us), rounds=us, reps=reps,
                   device=torch.cuda.get_device_properties(0).name, **{k: v() for k, v in extra.items()})
        print(json.dumps(row), flush=True)
        with open(os.path.join(a.out, "time_moving_time.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
        rows.append(row)

    for B in (int(v) for v in a.batches.split(",")):
        b = problem.make_trajectories(B, M, mp, seed=8)
        x, Df, T = (torch.tensor(np.ascontiguousarray(v), device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T))
        cost = torch.zeros(B, dtype=torch.float64, device=dev)
        gT = torch.zeros(B, M, dtype=torch.float64, device=dev)
        gt0 = torch.zeros(B, dtype=torch.float64, device=dev)
        grad = torch.zeros(B, 9 * (M - 1), dtype=torch.float64, device=dev)
        T_out = torch.zeros(B, M, dtype=torch.float64, device=dev)
        info = torch.zeros(B, 8, dtype=torch.float64, device=dev)
        o = gtop.GtopTimeOpt(rho=1.0, t_min=0.05, t_max=60.0, first_move=0.02, ftol_rel=0.0, xtol_abs=0.0, max_evals=EVALS)
        ctx.set_moving_cost(False)
        record("static_gradient", B, 0, lambda: gtop.time_gradient_device(ctx, x, Df, T, cost=cost, gT=gT), 50)
        for nbox in (int(v) for v in a.boxes.split(",")):
            rng = np.random.default_rng(100 + nbox)
            r, w = rng.integers(0, B, nbox), rng.integers(1, M, nbox)
            vel = rng.uniform(-0.5, 0.5, (nbox, 3))
            when = np.array([b.T[r[i], :w[i]].sum() for i in range(nbox)])
            p0 = b.waypoints[r, w] - vel * when[:, None]
            ctx.set_moving_boxes(p0, vel, rng.uniform(0.4, 1.0, (nbox, 3)))
            ctx.set_moving_cost(True)
            record("moving_gradient", B, nbox,
                   lambda: gtop.time_gradient_moving_device(ctx, x, Df, T, cost=cost, gT=gT, gt0=gt0), 50)
            record("moving_eval", B, nbox, lambda: ctx.eval_device(x, Df, T, cost=cost, grad=grad), 50)
            record("moving_optimize", B, nbox,
                   lambda: gtop.optimize_times_moving_device(ctx, o, x, Df, T, T_out=T_out, info=info), 10,
                   evals_min=lambda: float(info[:, 2].min()), evals_mean=lambda: float(info[:, 2].mean()),
                   evals_max=lambda: float(info[:, 2].max()))
            ctx.set_moving_cost(False)
    ctx.close()

    def cell(what, B, nbox):
        r = [q for q in rows if (q["what"], q["B"], q["boxes"]) == (what, B, nbox)]
        return r[0] if r else None

    with open(os.path.join(a.out, "time_moving_time.md"), "w") as f:
        f.write(f"# Segment-time entry points under the moving-obstacle cost, m = {M}\n\n"
                f"{rows[0]['device'] if rows else ''}; us per launch, least - greatest of {a.rounds} rounds "
                "(tools/time_moving_time.py).\n\n"
                "| B | boxes | static gradient | moving gradient | moving eval | gradient / static | gradient / eval | "
                "optimizer, us per evaluation (evaluations) |\n|---|---|---|---|---|---|---|---|\n")
        for B in sorted({q["B"] for q in rows}):
            s = cell("static_gradient", B, 0)
            for nbox in sorted({q["boxes"] for q in rows if q["boxes"]}):
                g, e, p = (cell(k, B, nbox) for k in ("moving_gradient", "moving_eval", "moving_optimize"))
                f.write(f"| {B} | {nbox} | {s['us_min']:.2f} - {s['us_max']:.2f} | {g['us_min']:.2f} - {g['us_max']:.2f} | "
                        f"{e['us_min']:.2f} - {e['us_max']:.2f} | {g['us_min'] / s['us_min']:.2f} | "
                        f"{g['us_min'] / e['us_min']:.2f} | {p['us_min'] / p['evals_mean']:.2f} ({p['evals_mean']:.1f}) |\n")


if __name__ == "__main__":
    main()
