#!/usr/bin/env python3
"""Device time of the per-segment report (gtop_validate_segments_device) beside the whole-trajectory report
(gtop_validate_trajectories_device) on the same inputs, and of the segment-time reallocation
(gtop_reallocate_times_device) on its own.  No threshold is set for any of them: the tool writes down what comes out.

Device-clock spans between two one-lane stamp kernels (gtop_device_clock_stamp, as bench.py times its region) around
back-to-back launches; the two reports alternate span by span in one process, so that a drift of the clocks or another
tenant of the machine touches both; minimum and median of the spans.  B = 1 024 and 16 384 trajectories of 6 segments,
8 moving boxes, dt_sample = 0.01; 200^3 map, random-walk waypoints.  Before timing, the laws between the two reports
(tests/segments_twin.py, check_laws) are checked on the first rows of each batch.

usage: tools/segment_time.py [--out profiles/segment_report]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1024, 6), (16384, 6))
NBOX, DT, SPANS = 8, 0.01, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_report"))
    a = ap.parse_args()

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import problem
    from tests import segments_twin as st

    dev = torch.device("cuda:0")
    ctx = gtop.GtopContext(0)
    hz = ctx.clock_hz()
    init = torch.tensor([2 ** 63 - 1, 0], dtype=torch.int64, device=dev)
    stamps = init.clone()

    def one_span(fn, reps):
        stamps.copy_(init)
        ctx.clock_stamp(stamps)
        for _ in range(reps):
            fn()
        ctx.clock_stamp(stamps)
        torch.cuda.synchronize()
        s = stamps.tolist()
        return (s[1] - s[0]) / hz * 1e6 / reps

    def spans(fns, reps):
        """us per call of each fn: SPANS spans each, alternating; sustained clocks first."""
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.2:
            for fn in fns:
                fn()
            torch.cuda.synchronize()
        got = [[] for _ in fns]
        for _ in range(SPANS):
            for k, fn in enumerate(fns):
                got[k].append(one_span(fn, reps))
        return [dict(min_us=float(np.min(g)), median_us=float(np.median(g)), max_us=float(np.max(g))) for g in got]

    mp = problem.make_map(200, density=0.02, seed=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    ctx.set_params()
    rows = []
    for B, m in SHAPES:
        b = problem.make_trajectories(B, m, mp, seed=1)
        rng = np.random.default_rng(3)
        j, w = rng.integers(0, B, NBOX), rng.integers(0, m + 1, NBOX)
        ctx.set_moving_boxes(b.waypoints[j, w] + rng.uniform(-0.3, 0.3, (NBOX, 3)),
                             rng.uniform(-2.0, 2.0, (NBOX, 3)) * (1.0, 1.0, 0.2), rng.uniform(1.0, 2.0, (NBOX, 3)))
        x, Df, T = (torch.tensor(v, device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T))
        coeff = ctx.coefficients_device(x, Df, T)
        lim = gtop.GtopLimits(margin=0.3, use_boxes=True)
        R = torch.empty(B, 12, dtype=torch.float64, device=dev)
        S = torch.empty(B, m, 10, dtype=torch.float64, device=dev)
        T_out = torch.empty(B, m, dtype=torch.float64, device=dev)
        ctx.validate_device(coeff, T, lim, dt_sample=DT, report=R)
        ctx.validate_segments_device(coeff, T, lim, dt_sample=DT, seg_report=S)
        torch.cuda.synchronize()
        Rh, Sh = R.cpu().numpy(), S.cpu().numpy()
        for i in range(min(B, 256)):
            assert st.check_laws(Sh[i], Rh[i]) == [], i
        samples = float(Rh[:, 0].sum())
        limits = gtop.GtopRetime(mode=1, max_vel=float(np.median(Sh[:, :, 6].max(axis=1))), scale_x=True, max_ratio=2.0)
        length = gtop.GtopRetime(mode=0)
        xs = x.clone()
        reps = 20 if B <= 1024 else 5
        t_rep, t_seg = spans([lambda: ctx.validate_device(coeff, T, lim, dt_sample=DT, report=R),
                              lambda: ctx.validate_segments_device(coeff, T, lim, dt_sample=DT, seg_report=S)], reps)
        t_lim, t_len = spans([lambda: ctx.reallocate_times_device(limits, x=xs, T=T, seg_report=S, T_out=T_out),
                              lambda: ctx.reallocate_times_device(length, x=x, Df=Df, T_out=T_out)], 20)
        rows.append(dict(B=B, m=m, boxes=NBOX, dt_sample=DT, samples=samples, report=t_rep, segment_report=t_seg,
                         reallocate_limits=t_lim, reallocate_length=t_len))
        print(rows[-1], flush=True)
    name = torch.cuda.get_device_name(0)
    ctx.close()

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "segment_time.json"), "w") as f:
        json.dump(dict(device=name, date=time.strftime("%Y-%m-%d"), spans=SPANS, rows=rows), f, indent=1)
    with open(os.path.join(a.out, "segment_time.md"), "w") as f:
        f.write(f"{name}, {time.strftime('%Y-%m-%d')}; fp64; device-clock spans (gtop_device_clock_stamp around back-to-back "
                f"launches), {SPANS} spans per entry, the two reports alternating span by span in one process: minimum "
                f"(median) in us per launch; 200^3 map, random-walk waypoints, {NBOX} moving boxes, dt_sample = {DT}; the "
                "laws between the two reports checked on the first 256 rows before timing\n\n")
        f.write("| B x m | samples | whole report (W = 4 / 2 / 1 by the batch) | segment report (W = 1) | segment / whole | "
                "reallocate LIMITS + scale_x | reallocate LENGTH |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            cell = lambda t: f"{t['min_us']:.1f} ({t['median_us']:.1f})"
            f.write(f"| {r['B']} x {r['m']} | {r['samples']:.0f} | {cell(r['report'])} | {cell(r['segment_report'])} | "
                    f"{r['segment_report']['min_us'] / r['report']['min_us']:.2f} | {cell(r['reallocate_limits'])} | "
                    f"{cell(r['reallocate_length'])} |\n")


if __name__ == "__main__":
    main()
