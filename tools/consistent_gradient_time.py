#!/usr/bin/env python3
"""Device time of evaluations and of the optimizer in the two gradient modes (gtop_set_gradient_mode), the default mode
against a PARENT build of the library measured in the same run, and what the consistent gradient buys the optimizer.

Times: B = 1 024 and 16 384 trajectories of 6 segments on the bench scene (200^3 map), fp64 and fp32 evaluations in
both modes, and the optimizer at 16 384 x 50 evaluations in both modes.  Spans of the device's own clock between two
one-lane stamp kernels around the launches (gtop_device_clock_stamp, as bench.py uses them), never host timers.  One
child process per library and round, parent build and this build alternating.  The table shows every round, so that
"this build, reference mode" can be judged against the spread the parent build shows against itself.

Mode comparison: the bench scene, B = 4 096, m = 6, stop rule ftol_rel = 1e-4 / max_evals = 100; per mode the median
and quartiles of the final cost and of the evaluations at the stop, and the share of rows that pass gtop_validate_batch
with margin d0 / 2.  The final COST is the same function in both modes, so the figures compare.

usage: tools/consistent_gradient_time.py [--parent-lib build_var/libgtop_parent.so] [--rounds 3]
                                         [--out profiles/consistent_gradient]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1024, 16384)
TAG = "CONSISTENT_TIME_JSON "


def _scene():
    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import problem

    mp = problem.make_map(200, density=0.02, seed=0)
    ctx = gtop.GtopContext(0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    ctx.set_params()
    return gtop, problem, mp, ctx


def child_times(reference_only):
    import time

    import torch

    gtop, problem, mp, ctx = _scene()
    dev = torch.device("cuda:0")
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

    modes = (("reference", False),) if reference_only else (("reference", False), ("consistent", True))
    out = {}
    for B in BATCHES:
        b = problem.make_trajectories(B, 6, mp, seed=1)
        b = problem.permute(b, problem.spatial_order(b.waypoints, mp.origin, mp.map_size))
        for name, td in (("fp64", torch.float64), ("fp32", torch.float32)):
            x, Df, T = (torch.tensor(a, dtype=td, device=dev) for a in (b.x, b.Df.reshape(-1, 18), b.T))
            cost = torch.empty(B, dtype=td, device=dev)
            grad = torch.empty_like(x)
            for mode, flag in modes:
                if not reference_only:
                    ctx.set_gradient_mode(flag)
                out[f"eval B={B} {name} {mode}"] = span(lambda: ctx.eval_device(x, Df, T, cost=cost, grad=grad), 20)
        if B == 16384:
            x, Df, T = (torch.tensor(a, device=dev) for a in (b.x, b.Df.reshape(-1, 18), b.T))
            lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
            lbt, ubt = torch.tensor(lb, device=dev), torch.tensor(ub, device=dev)
            xo = x.clone()

            def opt():
                xo.copy_(x)
                ctx.optimize_device(xo, Df, T, lbt, ubt, 50)
            for mode, flag in modes:
                if not reference_only:
                    ctx.set_gradient_mode(flag)
                out[f"optimize B={B} x 50 {mode}"] = span(opt, 2)
    print(TAG + json.dumps(out), flush=True)


def child_compare():
    import numpy as np

    gtop, problem, mp, ctx = _scene()
    B = 4096
    b = problem.make_trajectories(B, 6, mp, seed=1)
    b = problem.permute(b, problem.spatial_order(b.waypoints, mp.origin, mp.map_size))
    lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
    ctx.set_problem(b.T, b.Df)
    c_start, _ = ctx.eval_batch(b.x)
    limits = gtop.GtopLimits(margin=0.5 * ctx.params["d0"])

    def q(v):
        return [float(t) for t in np.percentile(v, (25, 50, 75))]

    _, ok, _ = ctx.validate_batch(b.x, limits, cost=c_start)
    out = {"start": dict(cost_q=q(c_start), pass_share=float(ok.mean()))}
    for mode, flag in (("reference", False), ("consistent", True)):
        ctx.set_gradient_mode(flag)
        xs, costs, nev, _ = ctx.optimize_batch_ex(b.x, lb, ub, 100, ftol_rel=1e-4)
        _, ok, _ = ctx.validate_batch(xs, limits, cost=costs)
        out[mode] = dict(cost_q=q(costs), nevals_q=q(nev), pass_share=float(ok.mean()),
                         rows_lower_than_other=None)
        out[mode]["costs"] = costs.tolist()
    cr, cc = np.array(out["reference"].pop("costs")), np.array(out["consistent"].pop("costs"))
    out["reference"]["rows_lower_than_other"] = float(np.mean(cr < cc))
    out["consistent"]["rows_lower_than_other"] = float(np.mean(cc < cr))
    print(TAG + json.dumps(out), flush=True)


def _run_child(what, parent_lib=None):
    env = dict(os.environ)
    if parent_lib:
        env["GTOP_HIP_LIB"] = os.path.realpath(parent_lib)
    else:
        env.pop("GTOP_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], env=env, capture_output=True,
                       text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
    if p.returncode != 0 or not line:
        sys.exit(f"child {what} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(line[0][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_var", "libgtop_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistent_gradient"))
    ap.add_argument("--child", choices=("times", "times-reference", "compare"))
    a = ap.parse_args()
    if a.child:
        return child_compare() if a.child == "compare" else child_times(a.child == "times-reference")
    if not os.path.exists(a.parent_lib):
        sys.exit(f"no parent build at {a.parent_lib}: make -C grad_traj_optimization_amd/csrc lib OUT=... on the parent commit")
    os.makedirs(a.out, exist_ok=True)
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):                                   # alternating, one fresh process each
        runs["parent"].append(_run_child("times-reference", a.parent_lib))
        runs["this"].append(_run_child("times"))
    with open(os.path.join(a.out, "consistent_gradient_time.json"), "w") as f:
        json.dump(dict(runs=runs, rounds=a.rounds), f, indent=1)
    fmt = lambda vs: " / ".join(f"{v:.1f}" for v in vs)
    lines = ["| workload | parent build, rounds (us) | this build, reference mode, rounds (us) | min this / min parent |"
             " parent's own spread | consistent mode, rounds (us) | consistent / reference (min) |",
             "|---|---|---|---|---|---|---|"]
    for k in runs["parent"][0]:
        par = [r[k] for r in runs["parent"]]
        ref = [r[k] for r in runs["this"]]
        con = [r[k.replace("reference", "consistent")] for r in runs["this"]]
        lines.append(f"| {k.replace(' reference', '')} | {fmt(par)} | {fmt(ref)} | {min(ref) / min(par):.3f} | "
                     f"{(max(par) / min(par) - 1) * 100:.1f} % | {fmt(con)} | {min(con) / min(ref):.3f} |")
    table = "\n".join(lines)
    with open(os.path.join(a.out, "consistent_gradient_time.md"), "w") as f:
        f.write("m = 6, bench scene (200^3 map); device-clock us per call, %d alternating rounds (parent build, this "
                "build), every round shown\n\n%s\n" % (a.rounds, table))
    print(table)

    cmp_ = _run_child("compare")
    with open(os.path.join(a.out, "mode_comparison.json"), "w") as f:
        json.dump(cmp_, f, indent=1)
    lines = ["| | final cost: quartile 1 / median / quartile 3 | evaluations at stop: q1 / median / q3 | "
             "rows passing validation (margin d0/2) | rows ending lower than in the other mode |", "|---|---|---|---|---|"]
    s = cmp_["start"]
    lines.append(f"| start point | {fmt(s['cost_q'])} | | {s['pass_share'] * 100:.1f} % | |")
    for mode in ("reference", "consistent"):
        r = cmp_[mode]
        lines.append(f"| {mode} gradient | {fmt(r['cost_q'])} | {fmt(r['nevals_q'])} | {r['pass_share'] * 100:.1f} % | "
                     f"{r['rows_lower_than_other'] * 100:.1f} % |")
    table = "\n".join(lines)
    with open(os.path.join(a.out, "mode_comparison.md"), "w") as f:
        f.write("bench scene (200^3 map), B = 4096, m = 6, fp64, stop rule ftol_rel = 1e-4 / max_evals = 100\n\n%s\n" % table)
    print(table)


if __name__ == "__main__":
    main()
