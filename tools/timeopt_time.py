#!/usr/bin/env python3
"""Device time of the segment-time entry points (include/gtop_time.h) beside the evaluation they differentiate, on the
same inputs: gtop_time_gradient_device, one gtop_optimize_times_device of exactly 20 evaluations, and gtop_eval_device,
at B trajectories of m = 6 segments on a random map.

ONE of the three per process (--what), so that each is a run of its own; --lib names the library to load (the
evaluation of an older build is timed by pointing it there: the evaluation needs include/gtop.h alone).  Device times
are spans of the device's own clock between two one-lane stamp kernels (gtop_device_clock_stamp) around `reps`
back-to-back launches, never host timers: the least of five spans per round, and the rounds' least and greatest of
that.  The optimizer is held to 20 evaluations by stop tolerances of zero on rows that do not converge sooner; the
evaluations it used are read back and printed (a row that stops early would show).  It appends one JSON line per batch
size to <out>/timeopt_time.jsonl and reads nothing but what it generates from a seed.

usage: tools/timeopt_time.py --what gradient|optimize|eval [--lib PATH] [--batches 1024,16384] [--rounds 3]
                             [--out profiles/timeopt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, EVALS = 6, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=("gradient", "optimize", "eval"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--batches", default="1024,16384")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeopt"))
    a = ap.parse_args()
    if a.lib:
        os.environ["GTOP_HIP_LIB"] = os.path.abspath(a.lib)

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
    for B in (int(v) for v in a.batches.split(",")):
        b = problem.make_trajectories(B, M, mp, seed=8)
        x, Df, T = (torch.tensor(np.ascontiguousarray(v), device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T))
        cost = torch.zeros(B, dtype=torch.float64, device=dev)
        extra = {}
        if a.what == "eval":
            grad = torch.zeros(B, 9 * (M - 1), dtype=torch.float64, device=dev)
            fn, reps = (lambda: ctx.eval_device(x, Df, T, cost=cost, grad=grad)), 50
        elif a.what == "gradient":
            gT = torch.zeros(B, M, dtype=torch.float64, device=dev)
            fn, reps = (lambda: gtop.time_gradient_device(ctx, x, Df, T, cost=cost, gT=gT)), 50
        else:
            T_out = torch.zeros(B, M, dtype=torch.float64, device=dev)
            info = torch.zeros(B, 8, dtype=torch.float64, device=dev)
            o = gtop.GtopTimeOpt(rho=1.0, t_min=0.05, t_max=60.0, first_move=0.02, ftol_rel=0.0, xtol_abs=0.0,
                                 max_evals=EVALS)
            fn, reps = (lambda: gtop.optimize_times_device(ctx, o, x, Df, T, T_out=T_out, info=info)), 10
        us = [span(fn, reps) for _ in range(a.rounds)]
        if a.what == "optimize":
            ev = info[:, 2]
            extra = dict(evals_min=float(ev.min()), evals_mean=float(ev.mean()), evals_max=float(ev.max()))
        row = dict(what=a.what, lib=os.path.relpath(gtop.library_path(), ROOT), B=B, m=M, us_min=min(us), us_max=max(us),
                   rounds=us, reps=reps, device=torch.cuda.get_device_properties(0).name, **extra)
        print(json.dumps(row), flush=True)
        with open(os.path.join(a.out, "timeopt_time.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
