#!/usr/bin/env python3
"""Device time of the continuous-time kinematic certificate (gtop_certify_kinematics_device) beside the clearance
certificate (gtop_certify_trajectories_device) on the same OPTIMISED trajectories: the report's own workload, B = 1 024
rows of 6 segments on the 200^3 map (tools/certify_time.py's rows and method).

  (a) the clearance certificate at the default options and margin 0.3,
  (b) the kinematic certificate with both limits off (level 0 alone: 64 intervals per segment), with and without seg,
  (c) the kinematic certificate against max_vel / max_acc at the default options, with the mean refinements per row and
      the share of each verdict.

Times are spans of the device's own clock between two one-lane stamp kernels (gtop_device_clock_stamp) around `reps`
back-to-back launches, never host timers; the least of five spans per round, and the rounds' least and greatest of that.
It writes kinematics_time.{md,json}.

usage: tools/kinematics_time.py [--rounds 3] [--max-vel 3.0] [--max-acc 6.0] [--out profiles/kinematics]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M, DT, MARGIN, EVALS, REPS = 1024, 6, 0.01, 0.3, 20, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-vel", type=float, default=3.0)
    ap.add_argument("--max-acc", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinematics"))
    a = ap.parse_args()

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

    def span(fn):
        """us per call of fn over REPS back-to-back calls, by the device clock; sustained clocks first."""
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.05:
            fn()
            torch.cuda.synchronize()
        best = None
        for _ in range(5):
            stamps.copy_(init)
            ctx.clock_stamp(stamps)
            for _ in range(REPS):
                fn()
            ctx.clock_stamp(stamps)
            torch.cuda.synchronize()
            st = stamps.tolist()
            us = (st[1] - st[0]) / hz * 1e6 / REPS
            best = us if best is None else min(best, us)
        return best

    b = problem.make_trajectories(B, M, mp, seed=1)
    ctx.set_problem(b.T, b.Df)
    lb, ub = ctx.default_bounds(b.waypoints)
    x, _ = ctx.optimize_batch(b.x, lb, ub, EVALS)
    coeff_h, _ = ctx.trajectory_stats(x, DT)
    coeff, T = torch.tensor(coeff_h, device=dev), torch.tensor(b.T, device=dev)
    cert = torch.empty(B, 8, dtype=torch.float64, device=dev)
    kin = torch.empty(B, 11, dtype=torch.float64, device=dev)
    seg = torch.empty(B, M, 10, dtype=torch.float64, device=dev)
    clear, off = gtop.GtopCertifyOpts(margin=MARGIN), gtop.GtopKinOpts()
    lim = gtop.GtopKinOpts(a.max_vel, a.max_acc)
    rows = {
        "clearance certificate, margin 0.3": lambda: gtop.certify_device(ctx, coeff, T, clear, cert=cert),
        "kinematic certificate, limits off, kin + seg": lambda: gtop.certify_kinematics_device(ctx, coeff, T, off, kin=kin, seg=seg),
        "kinematic certificate, limits off, kin only": lambda: gtop.certify_kinematics_device(ctx, coeff, T, off, kin=kin, want_seg=False),
        f"kinematic certificate, max_vel {a.max_vel} max_acc {a.max_acc}, kin + seg":
            lambda: gtop.certify_kinematics_device(ctx, coeff, T, lim, kin=kin, seg=seg),
    }
    times = {name: [] for name in rows}
    for _ in range(a.rounds):           # the rows alternate within a round
        for name, fn in rows.items():
            times[name].append(span(fn))
    gtop.certify_device(ctx, coeff, T, clear, cert=cert)
    gtop.certify_kinematics_device(ctx, coeff, T, lim, kin=kin, seg=seg)
    torch.cuda.synchronize()
    c, k = cert.cpu().numpy(), kin.cpu().numpy()
    out = {"workload": f"B={B} x {M} segments, 200^3 map, {EVALS} optimizer evaluations, {REPS} launches per span",
           "us_per_launch": {n: {"min": min(t), "max": max(t), "rounds": t} for n, t in times.items()},
           "clearance": {"mean_refinements": float(c[:, 6].mean()),
                         "verdicts_unsafe_undecided_safe": np.bincount((c[:, 0] + 1).astype(int), minlength=3).tolist()},
           "kinematic": {"max_vel": a.max_vel, "max_acc": a.max_acc, "mean_refinements": float(k[:, 9].mean()),
                         "verdicts_exceeds_undecided_within": np.bincount((k[:, 0] + 1).astype(int), minlength=3).tolist(),
                         "median_ub_v": float(np.median(k[:, 1])), "median_ub_a": float(np.median(k[:, 4]))}}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "kinematics_time.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, "kinematics_time.md"), "w") as f:
        f.write(f"{out['workload']}\n\n| launch | us, least of the rounds | greatest |\n|---|---|---|\n")
        for n, t in out["us_per_launch"].items():
            f.write(f"| {n} | {t['min']:.1f} | {t['max']:.1f} |\n")
        f.write(f"\nclearance: {out['clearance']}\nkinematic: {out['kinematic']}\n")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
