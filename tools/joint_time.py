#!/usr/bin/env python3
"""Device time of the joint entry points (include/gtop_joint.h) beside what the same information costs without them,
on the same rows of a random map: gtop_joint_gradient_device (`joint`) against a consistent-mode gtop_eval_device plus
gtop_time_gradient_device (`pair`: cost, d cost / d x and d cost / d T from two kernels, each with its own lookups), and
one round of gtop_optimize_joint_device (`round`: the joint pass at the trial point plus the MMA update over 10 m - 9
variables), taken as the difference of two calls of 5 and 25 evaluations divided by 20, with the 5-evaluation call's
time beside it (pack, initialisation, closing pass, finish and report included).

ONE of the three per process (--what), so that each is a run of its own.  Device times are spans of the device's own
clock between two one-lane stamp kernels (gtop_device_clock_stamp) around `reps` back-to-back calls, never host timers:
the least of five spans per round, and the rounds' least and greatest of that.  It appends one JSON line per shape to
<out>/joint_time.jsonl, reads nothing but what it generates from a seed, and --report turns the lines into
<out>/joint_time.md.

usage: tools/joint_time.py --what joint|pair|round [--shapes 1024x6,16384x6,8192x13] [--rounds 3] [--out profiles/joint]
       tools/joint_time.py --report [--out profiles/joint]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_LO, E_HI = 5, 25


def report(out):
    rows = [json.loads(ln) for ln in open(os.path.join(out, "joint_time.jsonl")) if ln.strip()]
    last = {}
    for r in rows:
        last[(r["what"], r["B"], r["m"])] = r
    shapes = sorted({(B, m) for (_, B, m) in last}, key=lambda s: (s[1], s[0]))
    device = rows[-1]["device"] if rows else "?"
    lines = [f"# Joint pass and joint optimizer: device time ({device})", "",
             "`tools/joint_time.py`; microseconds by the device clock, least of five spans, least .. greatest of the rounds.",
             "", "| rows x segments | joint pass | eval (consistent) + time gradient | pair / joint | one optimizer round | "
             f"optimizer call of {E_LO} evaluations |", "|---|---|---|---|---|---|"]
    for B, m in shapes:
        j, p, r = (last.get((w, B, m)) for w in ("joint", "pair", "round"))
        cell = lambda v: "-" if v is None else f"{v['us_min']:.1f} .. {v['us_max']:.1f}"
        ratio = "-" if j is None or p is None else f"{p['us_min'] / j['us_min']:.2f}"
        call = "-" if r is None else f"{r['call_lo_us']:.1f}"
        lines.append(f"| {B} x {m} | {cell(j)} | {cell(p)} | {ratio} | {cell(r)} | {call} |")
    with open(os.path.join(out, "joint_time.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("joint", "pair", "round"))
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--shapes", default="1024x6,16384x6,8192x13")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint"))
    a = ap.parse_args()
    if a.report:
        return report(a.out)
    if not a.what:
        ap.error("--what or --report")

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
    for B, m in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        b = problem.make_trajectories(B, m, mp, seed=8, step_len=(0.5, 1.2) if m > 6 else (1.0, 2.0))
        x, Df, T = (torch.tensor(np.ascontiguousarray(v), device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T))
        n = 9 * (m - 1)
        cost = torch.zeros(B, dtype=torch.float64, device=dev)
        gx = torch.zeros(B, n, dtype=torch.float64, device=dev)
        gT = torch.zeros(B, m, dtype=torch.float64, device=dev)
        extra = {}
        if a.what == "joint":
            fn = lambda: gtop.joint_gradient_device(ctx, x, Df, T, cost=cost, gx=gx, gT=gT)
            us = [span(fn, 50) for _ in range(a.rounds)]
        elif a.what == "pair":
            ctx.set_gradient_mode(True)
            cost2 = torch.zeros(B, dtype=torch.float64, device=dev)

            def fn():
                ctx.eval_device(x, Df, T, cost=cost, grad=gx)
                gtop.time_gradient_device(ctx, x, Df, T, cost=cost2, gT=gT)
            us = [span(fn, 50) for _ in range(a.rounds)]
        else:
            lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
            lbt, ubt = (torch.tensor(np.ascontiguousarray(v), device=dev) for v in (lb, ub))
            work = torch.zeros(gtop.joint_workspace_bytes(B, m), dtype=torch.uint8, device=dev)
            T_out = torch.zeros(B, m, dtype=torch.float64, device=dev)
            info = torch.zeros(B, 8, dtype=torch.float64, device=dev)
            xw = x.clone()

            def call(evals):
                o = gtop.GtopJointOpt(rho=1.0, t_min=0.05, t_max=60.0, max_evals=evals)

                def fn():
                    xw.copy_(x)
                    gtop.optimize_joint_device(ctx, o, xw, Df, T, lbt, ubt, T_out=T_out, info=info, work=work)
                return fn
            us, lo_all = [], []
            for _ in range(a.rounds):
                lo, hi = span(call(E_LO), 5), span(call(E_HI), 5)
                lo_all.append(lo)
                us.append((hi - lo) / (E_HI - E_LO))
            extra = dict(call_lo_us=min(lo_all), evals_lo=E_LO, evals_hi=E_HI, evals_used_mean=float(info[:, 1].mean()))
        row = dict(what=a.what, lib=os.path.relpath(gtop.library_path(), ROOT), B=B, m=m, us_min=min(us), us_max=max(us),
                   rounds=us, device=torch.cuda.get_device_properties(0).name, **extra)
        print(json.dumps(row), flush=True)
        with open(os.path.join(a.out, "joint_time.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
