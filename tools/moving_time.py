#!/usr/bin/env python3
"""Device time of fp64 evaluations and of the optimizer with the moving-obstacle cost (gtop_set_moving_cost) off and on,
with constant-velocity and with polynomial box lists (gtop_set_moving_box_polynomials), against the same rows of a
PARENT build of the library measured in the same run.

B = 1 024 and 16 384 trajectories of 6 segments on the 200^3 map; mode off, and on with 1, 8 and 32 boxes — spread
over the map, and the worst case: every box aimed at a waypoint of the batch at the moment its trajectory is there —
and the optimizer at 16 384 x 50 evaluations off / on.  The polynomial rows are the same boxes with an acceleration of
up to 1 m/s^2 (0.2 in z), as quadratics in t.  Times are spans of the device's own clock between two one-lane
stamp kernels around the launches (gtop_device_clock_stamp, as bench.py uses them), never host timers.  One child
process per library and round, parent build and this build alternating; the table takes each row's minimum.

The bar: every mode-off and constant-velocity row of this build within the larger of 2 % and twice the row's own
spread over rounds (of the parent build) of the parent's row; the exit status is non-zero when a row misses it.  The
polynomial rows have no bar: they are reported as a ratio to their constant-velocity row.

usage: tools/moving_time.py [--parent-lib build_var/libgtop_parent.so] [--rounds 3] [--out profiles/box_polynomials]
(a parent build without the moving-obstacle cost: --parent-mode off, its mode-off rows only)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1024, 16384)
BOXES = (1, 8, 32)


def child(mode):
    """mode: "off" = the mode-off rows only, "constvel" = those and the constant-velocity rows, "all" = the polynomial
    rows too."""
    off_only, with_poly = mode == "off", mode == "all"
    import time

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import problem

    mp = problem.make_map(200, density=0.02, seed=0)
    ctx = gtop.GtopContext(0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    ctx.set_params()
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

    def boxes(b, t0, nbox, kind, rng):
        """(p0, vel, scale), and the moment each box is where it is aimed (0: p0 itself)"""
        if kind == "spread":
            return (rng.uniform(mp.origin, mp.origin + mp.map_size, (nbox, 3)), rng.uniform(-1.0, 1.0, (nbox, 3)),
                    rng.uniform(1.0, 2.0, (nbox, 3))), np.zeros(nbox)
        j = rng.integers(0, len(b.x), nbox)                    # "near": aimed at the batch's own waypoints
        w = rng.integers(0, b.m + 1, nbox)
        vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * np.array([1.0, 1.0, 0.2])
        when = np.array([t0[jj] + b.T[jj][:ww].sum() for jj, ww in zip(j, w)])
        return (b.waypoints[j, w] - vel * when[:, None], vel, rng.uniform(1.0, 2.0, (nbox, 3))), when

    def polynomials(bx, when, rng_acc):
        """The same boxes with an acceleration a around `when`: c(t) = c(when) + v (t - when) + a (t - when)^2 / 2 in
        powers of t, v the box's velocity at `when`."""
        p0, vel, scale = bx
        acc = rng_acc.uniform(-1.0, 1.0, p0.shape) * np.array([1.0, 1.0, 0.2])
        when = when[:, None]
        coef = np.zeros((p0.shape[0], 3, 6))
        coef[:, :, 0] = p0 + 0.5 * acc * when * when
        coef[:, :, 1] = vel - acc * when
        coef[:, :, 2] = 0.5 * acc
        return coef, scale

    out = {}
    for B in BATCHES:
        b = problem.make_trajectories(B, 6, mp, seed=1)
        b = problem.permute(b, problem.spatial_order(b.waypoints, mp.origin, mp.map_size))
        rng = np.random.default_rng(B)
        rng_acc = np.random.default_rng(B + 1)                  # (a stream of its own: the constant-velocity rows keep theirs)
        t0 = rng.uniform(0.0, 5.0, B)
        x, Df, T = (torch.tensor(a, device=dev) for a in (b.x, b.Df.reshape(-1, 18), b.T))
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        grad = torch.empty_like(x)
        ev = lambda: ctx.eval_device(x, Df, T, cost=cost, grad=grad)
        out[f"eval B={B} off"] = span(ev, 20)
        if not off_only:
            ctx.set_start_times(t0)
            for kind in ("spread", "near"):
                for nbox in BOXES:
                    bx, when = boxes(b, t0, nbox, kind, rng)
                    ctx.set_moving_boxes(*bx)
                    ctx.set_moving_cost(True)
                    out[f"eval B={B} on {nbox} boxes {kind}"] = span(ev, 20)
                    if with_poly:
                        ctx.set_moving_box_polynomials(*polynomials(bx, when, rng_acc))
                        out[f"eval B={B} on {nbox} polynomial boxes {kind}"] = span(ev, 20)
                    ctx.set_moving_cost(False)
        if B == 16384:
            lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
            lbt, ubt = torch.tensor(lb, device=dev), torch.tensor(ub, device=dev)
            xo = x.clone()

            def opt():
                xo.copy_(x)
                ctx.optimize_device(xo, Df, T, lbt, ubt, 50)
            out[f"optimize B={B} x 50 off"] = span(opt, 2)
            if not off_only:
                for kind in ("spread", "near"):
                    bx, when = boxes(b, t0, 8, kind, rng)
                    ctx.set_moving_boxes(*bx)
                    ctx.set_moving_cost(True)
                    out[f"optimize B={B} x 50 on 8 boxes {kind}"] = span(opt, 2)
                    if with_poly:
                        ctx.set_moving_box_polynomials(*polynomials(bx, when, rng_acc))
                        out[f"optimize B={B} x 50 on 8 polynomial boxes {kind}"] = span(opt, 2)
                    ctx.set_moving_cost(False)
    print("MOVING_TIME_JSON " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_var", "libgtop_parent.so"))
    ap.add_argument("--parent-mode", choices=("constvel", "off"), default="constvel")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_polynomials"))
    ap.add_argument("--child", choices=("all", "constvel", "off"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not os.path.exists(a.parent_lib):
        sys.exit(f"no parent build at {a.parent_lib}: make -C grad_traj_optimization_amd/csrc lib OUT=... on the parent commit")
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):                                   # alternating, one fresh process each
        for who in ("parent", "this"):
            env = dict(os.environ)
            if who == "parent":
                env["GTOP_HIP_LIB"] = os.path.realpath(a.parent_lib)
            else:
                env.pop("GTOP_HIP_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", a.parent_mode if who == "parent" else "all"],
                               env=env, capture_output=True, text=True, timeout=300)   # (each child under its own limit)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("MOVING_TIME_JSON ")]
            if p.returncode != 0 or not line:   # (nothing more is started on the device after a child that failed)
                sys.exit(f"{who} child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[who].append(json.loads(line[0].split(" ", 1)[1]))
    best = {who: {k: min(r[k] for r in rs) for k in rs[0]} for who, rs in runs.items()}
    spread = {who: {k: max(r[k] for r in rs) / min(r[k] for r in rs) - 1 for k in rs[0]} for who, rs in runs.items()}
    missed = []
    lines = ["| workload | us (device clock) | x parent's same row | allowed | x parent's mode-off | x its constant-velocity row | spread over rounds |",
             "|---|---|---|---|---|---|---|"]
    for k, v in best["this"].items():
        base = k.split(" off")[0].split(" on ")[0] + " off"
        vs_off = f"{v / best['parent'][base]:.2f}"
        if " polynomial" in k:                                  # no bar: against the same boxes at constant velocity
            same = allowed = "-"
            vs_cv = f"{v / best['this'][k.replace(' polynomial', '')]:.2f}"
        elif k in best["parent"]:
            ratio, margin = v / best["parent"][k], max(0.02, 2 * spread["parent"][k])
            same, allowed, vs_cv = f"{ratio:.3f}", f"{1 + margin:.3f}", "-"
            if ratio > 1 + margin:
                missed.append(k)
                same += " MISSED"
        else:
            same = allowed = vs_cv = "-"
        lines.append(f"| {k} | {v:.1f} | {same} | {allowed} | {vs_off} | {vs_cv} | {spread['this'][k] * 100:.1f} % |")
    for k, v in best["parent"].items():
        lines.append(f"| parent build: {k} | {v:.1f} | 1.000 | - | - | - | {spread['parent'][k] * 100:.1f} % |")
    table = "\n".join(lines)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "moving_time.json"), "w") as f:
        json.dump(dict(runs=runs, best_us=best, rounds=a.rounds, missed=missed), f, indent=1)
    with open(os.path.join(a.out, "moving_time.md"), "w") as f:
        f.write("fp64, m = 6, 200^3 map; minimum over %d alternating rounds; box-skip hit rate: not collected\n"
                "allowed = 1 + the larger of 2 %% and twice the spread of the parent build's row over the rounds; rows "
                "that miss it: %s\n\n%s\n" % (a.rounds, ", ".join(missed) if missed else "none", table))
    print(table)
    if missed:
        sys.exit("rows over the bar: " + ", ".join(missed))


if __name__ == "__main__":
    main()
