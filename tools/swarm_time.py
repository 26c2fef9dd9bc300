#!/usr/bin/env python3
"""Device time of the swarm entry points (include/gtop_swarm.h) at B robots of m = 6 segments on 256 grid samples, in a
random map: gtop_swarm_gradient_device (joint form), gtop_optimize_swarm_device at 1 sweep x 50 evaluations, and the
yardstick for what the swarm rounds add, gtop_optimize_device_ex in its two-launch form at 50 evaluations on the same
rows.

ONE of the three per process (--what), so that each is a run of its own — and a run under `rocprofv3 --kernel-trace
--stats -- python tools/swarm_time.py --what gradient ...` gives the kernels' own times.  Times are HIP events around
one call on the stream, the median of 20 calls after warm-up (the least and the greatest beside it).  The share of the
pairs that interact is printed with the gradient: the pair kernel skips the force arithmetic where no lane of a
wavefront has an active term.  It appends one JSON line per batch size to <out>/swarm_time.jsonl and reads nothing but
what it generates from a seed.

usage: tools/swarm_time.py --what gradient|optimize|baseline [--lib PATH] [--batches 64,256,1024] [--radius 1.0]
                           [--out profiles/swarm]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, SAMPLES, EVALS, CALLS = 6, 256, 50, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=("gradient", "optimize", "baseline"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swarm"))
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
    ctx.set_params()
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(us)), float(min(us)), float(max(us))

    os.makedirs(a.out, exist_ok=True)
    for B in (int(v) for v in a.batches.split(",")):
        b = problem.make_trajectories(B, M, mp, seed=100 + B)
        lb, ub = gtop.GtopContext.default_bounds(b.waypoints)
        x0 = torch.tensor(b.x, device=dev)
        Df, T = torch.tensor(b.Df.reshape(-1, 18), device=dev), torch.tensor(b.T, device=dev)
        lbt, ubt = torch.tensor(lb, device=dev), torch.tensor(ub, device=dev)
        dt = float(b.T.sum(axis=1).max()) / (SAMPLES - 1)
        opts = gtop.GtopSwarmOpts(t_lo=0.0, dt=dt, n_samples=SAMPLES, w=20.0, radius=a.radius, hold_ends=True)
        work = torch.zeros(gtop.swarm_workspace_bytes(B, M, SAMPLES), device=dev, dtype=torch.uint8)
        rec = dict(what=a.what, B=B, m=M, samples=SAMPLES, radius=a.radius)
        if a.what == "gradient":
            coeff = ctx.coefficients_device(x0, Df, T)
            S, g, act = (torch.empty(B, device=dev, dtype=torch.float64), torch.empty((B, 9 * (M - 1)), device=dev, dtype=torch.float64),
                         torch.empty(B, device=dev, dtype=torch.float64))
            med, lo, hi = timed(lambda: gtop.swarm_gradient_device(ctx, opts, coeff, T, S=S, grad=g, active=act, work=work))
            rec.update(us=med, us_min=lo, us_max=hi, pair_samples=B * (B - 1) * SAMPLES,
                       active_share=float(act.sum().item()) / max(B * (B - 1) * SAMPLES, 1))
        else:
            x, mc = x0.clone(), torch.empty(B, device=dev, dtype=torch.float64)
            if a.what == "optimize":
                stop = gtop.GtopSwarmStop(1, EVALS)

                def call():
                    x.copy_(x0)
                    gtop.optimize_swarm_device(ctx, opts, stop, x, Df, T, lbt, ubt, min_cost=mc, work=work)
            else:
                ctx.set_optimizer_fusion(0)   # the two-launch form: what the swarm rounds are added to

                def call():
                    x.copy_(x0)
                    ctx.optimize_device(x, Df, T, lbt, ubt, EVALS, min_cost=mc)
            med, lo, hi = timed(call)
            rec.update(us=med, us_min=lo, us_max=hi, evals=EVALS, min_cost_mean=float(mc.mean().item()))
        print(json.dumps(rec))
        with open(os.path.join(a.out, "swarm_time.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
