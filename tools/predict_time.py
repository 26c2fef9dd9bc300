#!/usr/bin/env python3
"""Device time of the prediction fit (include/gtop_prediction.h): gtop_fit_predictions_device and
gtop_refresh_box_predictions_device, both modes, at N objects with full histories of H samples (wrapped rings), and
beside each figure the host entry gtop_fit_predictions on one core.

Device times are spans of the device's own clock between two one-lane stamp kernels (gtop_device_clock_stamp) around
`reps` back-to-back launches, never host timers: the least of five spans per round, and the rounds' least and greatest
of that.  The refresh is timed at N <= GTOP_MOVING_COST_MAX_BOXES only where it also writes the cost bodies' rows;
larger lists write the query buffer alone.  The host entry is the least of three calls by the host's clock.  A kernel
that runs less than ~10 us is a statement about launch rate, not about the kernel; the bytes a launch reads (N H 32)
over the time is printed for scale.  It writes predict_time.{md,json}.

usage: tools/predict_time.py [--rounds 3] [--out profiles/prediction] [--small]   (--small: a rehearsal of two sizes)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, HS, REPS = (5, 32, 1024, 16384), (20, 64, 256), 20


def histories(np, N, H, seed):
    """Full rings of H samples on smooth curves with 1 cm of noise, times advancing by about 50 ms."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 50.0, (N, 1)) + np.cumsum(rng.uniform(0.03, 0.07, (N, H)), axis=1)
    a = rng.normal(size=(N, 1, 3, 3))
    u = (t - t[:, :1])[:, :, None]
    q = a[:, :, :, 0] + a[:, :, :, 1] * u + 0.3 * a[:, :, :, 2] * u * u + 0.01 * rng.normal(size=(N, H, 3))
    hist = np.concatenate([q, t[:, :, None]], axis=2)
    head = rng.integers(0, H, N).astype(np.int32)
    hist = np.stack([np.roll(hist[n], int(head[n]), axis=0) for n in range(N)])
    return np.ascontiguousarray(hist), np.full(N, H, dtype=np.int32), head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prediction"))
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import prediction as gp

    ctx = gtop.GtopContext(0)
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

    rows = []
    sizes = [(5, 20), (1024, 64)] if a.small else [(N, H) for N in NS for H in HS]
    for N, H in sizes:
        hist, count, head = histories(np, N, H, seed=N + H)
        h, c, hd = torch.tensor(hist, device=dev), torch.tensor(count, device=dev), torch.tensor(head, device=dev)
        coef = torch.zeros(N, 18, dtype=torch.float64, device=dev)
        t_range = torch.zeros(N, 2, dtype=torch.float64, device=dev)
        info = torch.zeros(N, 12, dtype=torch.float64, device=dev)
        scale = torch.ones(N, 3, dtype=torch.float64, device=dev)
        ctx.set_moving_box_polynomials(np.zeros((N, 3, 6)), np.ones((N, 3)), np.tile([0.0, 1.0], (N, 1)))
        for mode, name in ((gp.PREDICT_POLYFIT, "polyfit"), (gp.PREDICT_CONST_VEL, "const_vel")):
            o = gp.GtopPredictOpts(mode=mode, horizon=1.0, inflate=1.0)
            calls = {
                "fit": lambda: gp.fit_predictions_device(ctx, h, c, o, hd, coef, t_range, info),
                "refresh": lambda: gp.refresh_box_predictions_device(ctx, h, c, o, hd, scale=scale, info=info),
            }
            us = {k: [] for k in calls}
            for _ in range(a.rounds):       # the two entries alternate within a round
                for k, fn in calls.items():
                    us[k].append(span(fn))
            fitted = int((info[:, 0] <= gp.PRED_LOWERED).sum())
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                gp.fit_predictions(hist, count, o, head=head, want_local=False)
                host.append((time.perf_counter() - t0) * 1e6)
            row = dict(N=N, H=H, mode=name, fitted=fitted, host_us=min(host),
                       read_GBps=N * H * 32 / (min(us["fit"]) * 1e-6) / 1e9,
                       **{f"{k}_us": {"min": min(v), "max": max(v), "rounds": v} for k, v in us.items()})
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "method": f"device-clock spans around {REPS} back-to-back launches, least of 5 spans, "
           f"{a.rounds} rounds; host entry: least of 3 calls on one core", "rows": rows}
    os.makedirs(a.out, exist_ok=True)
    stem = "predict_time_small" if a.small else "predict_time"
    with open(os.path.join(a.out, stem + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, stem + ".md"), "w") as f:
        f.write(f"{out['device']}; fp64; {out['method']}.  us per launch, least of the rounds (greatest).\n\n"
                "| N | H | mode | fit_predictions_device | refresh_box_predictions_device | host entry, one core | "
                "histories read, GB/s |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['N']} | {r['H']} | {r['mode']} | {r['fit_us']['min']:.1f} ({r['fit_us']['max']:.1f}) | "
                    f"{r['refresh_us']['min']:.1f} ({r['refresh_us']['max']:.1f}) | {r['host_us']:.0f} | "
                    f"{r['read_GBps']:.1f} |\n")
    ctx.close()


if __name__ == "__main__":
    main()
