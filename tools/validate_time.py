#!/usr/bin/env python3
"""Device time of the fused trajectory report (gtop_validate_trajectories_device) against the composition it replaces,
made only of entry points a PARENT build of the library has too: gtop_sample_trajectories_device (every sample to
HBM), gtop_edt_query_device over all of them (distance and gradient back to HBM), and a torch amin per trajectory.

B = 1 024 and 16 384 trajectories of 6 segments on the 200^3 map with 0, 8 and 32 boxes.  The composition's per-sample
times (t0[b] + eval_t) are prepared outside the timed span; its sample buffer is B x (largest sample count) x 3, so it
also queries the padding of the shorter rows (filled once, outside the span, with points that cannot lower the minimum;
the share of padding is printed beside the table).  A caller's other choice is a compaction pass: (a') times sampling,
a gather of the real samples into a dense list (torch index_select, indices prepared outside the span) and the query
over that list, WITHOUT any per-trajectory reduction — a lower bound of that route, given for comparison; the
condition the fused report is held to is the one on (a).  Times are spans
of the device's own clock between two one-lane stamp kernels (gtop_device_clock_stamp), never host timers.  One child
process per library and round, the parent build and this build alternating; each row's minimum is taken, and the
parent's own spread over the rounds is the yardstick for the two kernels whose ISA the shared headers touched
(the 2^20-query time of edt_query_kernel and the 1 024-trajectory time of eval_trajectories_kernel).

The tool also runs the headline benchmark (`bench.py --gpus 1 --steps 2000 --warmup 100`) on both builds, alternating,
and writes that line under the table.  It writes validate_time.{md,json} only; notes kept by hand go into a file beside
them (profiles/validate/NOTES.md), which a re-run leaves alone.

usage: tools/validate_time.py [--parent-lib build_var/libgtop_parent.so] [--rounds 2] [--bench-rounds 2]
                              [--out profiles/validate]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1024, 16384)
BOXES = (0, 8, 32)
DT = 0.01


def child(fused):
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
    L, h = ctx._L, ctx._h
    dev = torch.device("cuda:0")
    hz = ctx.clock_hz()
    init = torch.tensor([2 ** 63 - 1, 0], dtype=torch.int64, device=dev)
    stamps = init.clone()
    vp = C.c_void_p

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

    out = {}
    stream = torch.cuda.current_stream(dev).cuda_stream
    for B in BATCHES:
        b = problem.make_trajectories(B, 6, mp, seed=1)
        ctx.set_problem(b.T, b.Df)
        coeff_h, stats_h = ctx.trajectory_stats(b.x, DT)
        counts = stats_h[:, 8].astype(np.int64)
        cap = int(counts.max())
        rng = np.random.default_rng(B)
        t0 = rng.uniform(0.0, 5.0, B)
        coeff = torch.tensor(coeff_h, device=dev)
        T = torch.tensor(b.T, device=dev)
        stats = torch.empty(B, 9, dtype=torch.float64, device=dev)
        samples = torch.zeros(B, cap, 3, dtype=torch.float64, device=dev)
        # t0[b] + eval_t per stored sample (eval_t accumulated as the kernel does), -1 behind a row's count
        acc = np.zeros(cap)
        for k in range(1, cap):
            acc[k] = acc[k - 1] + DT
        tau_h = t0[:, None] + acc[None, :]
        tau_h[np.arange(cap)[None, :] >= counts[:, None]] = -1.0
        tau = torch.tensor(tau_h, device=dev)
        static = torch.full_like(tau, -1.0)
        dist = torch.empty(B * cap, dtype=torch.float64, device=dev)
        grad = torch.empty(B * cap, 3, dtype=torch.float64, device=dev)
        pad = torch.tensor(np.arange(cap)[None, :] >= counts[:, None], device=dev)
        clearance = torch.empty(B, dtype=torch.float64, device=dev)
        # the compacted route: the real samples' rows in the padded buffer, their times, a dense position list
        keep = torch.nonzero(~pad.reshape(-1)).reshape(-1)
        nreal = int(keep.numel())
        cpos = torch.empty(nreal, 3, dtype=torch.float64, device=dev)
        ctau, cstatic = tau.reshape(-1)[keep].contiguous(), torch.full((nreal,), -1.0, dtype=torch.float64, device=dev)
        out[f"padding share B={B}"] = 1.0 - nreal / float(B * cap)
        report = torch.empty(B, 12, dtype=torch.float64, device=dev)
        ctx.set_start_times(t0)

        def sample():
            rc = L.gtop_sample_trajectories_device(h, B, 6, vp(coeff.data_ptr()), vp(T.data_ptr()), 6, DT,
                                                   vp(stats.data_ptr()), vp(samples.data_ptr()), cap, vp(stream))
            assert rc == 0

        # the padding behind a row's count, which the sampling kernel never writes: the row's own first point, looked up
        # static only — no smaller than that sample's real distance, so a plain amin over the padded row is the clearance
        sample()
        torch.cuda.synchronize()
        samples[pad] = samples[:, :1, :].expand(B, cap, 3)[pad]
        if B == 1024:
            out["sampling 1024 trajectories (eval_trajectories_kernel)"] = span(sample, 20)
        for nbox in BOXES:
            ctx.set_moving_boxes(rng.uniform(mp.origin, mp.origin + mp.map_size, (nbox, 3)),
                                 rng.uniform(-1.0, 1.0, (nbox, 3)), rng.uniform(1.0, 2.0, (nbox, 3)))
            times = tau if nbox else static

            def composed():
                sample()
                rc = L.gtop_edt_query_device(h, B * cap, vp(samples.data_ptr()), vp(times.data_ptr()),
                                             vp(dist.data_ptr()), vp(grad.data_ptr()), vp(stream))
                assert rc == 0
                torch.amin(dist.view(B, cap), dim=1, out=clearance)

            ctimes = ctau if nbox else cstatic

            def compacted():
                sample()
                torch.index_select(samples.view(B * cap, 3), 0, keep, out=cpos)
                rc = L.gtop_edt_query_device(h, nreal, vp(cpos.data_ptr()), vp(ctimes.data_ptr()), vp(dist.data_ptr()),
                                             vp(grad.data_ptr()), vp(stream))
                assert rc == 0

            reps = 20 if B == 1024 else 5
            out[f"composed B={B} boxes={nbox}"] = span(composed, reps)
            out[f"compacted B={B} boxes={nbox}"] = span(compacted, reps)
            if fused:
                lim = gtop.GtopLimits(margin=0.3, use_boxes=nbox > 0)
                fn = lambda: ctx.validate_device(coeff, T, lim, dt_sample=DT, report=report)
                out[f"fused B={B} boxes={nbox}"] = span(fn, reps)
                composed()
                fn()
                torch.cuda.synchronize()
                assert torch.equal(report[:, 1], clearance), "the fused clearance differs from the composition's"
                assert torch.equal(report[:, 0], stats[:, 8])
    # the 2^20-query time of the kernel that now shares its lookup with the report
    N = 1 << 20
    rng = np.random.default_rng(0)
    pos = torch.tensor(rng.uniform(mp.origin + 0.5, mp.origin + mp.map_size - 0.5, size=(N, 3)), device=dev)
    tq = torch.tensor(rng.uniform(0.0, 3.0, size=N), device=dev)
    ctx.set_moving_boxes(rng.uniform(mp.origin, mp.origin + mp.map_size, size=(32, 3)), rng.uniform(-1, 1, size=(32, 3)),
                         rng.uniform(0.3, 1.5, size=(32, 3)))
    dq = torch.empty(N, dtype=torch.float64, device=dev)
    gq = torch.empty(N, 3, dtype=torch.float64, device=dev)
    for name, t in (("32 boxes", tq), ("static only", -torch.ones_like(tq))):
        fn = lambda: L.gtop_edt_query_device(h, N, vp(pos.data_ptr()), vp(t.data_ptr()), vp(dq.data_ptr()),
                                             vp(gq.data_ptr()), vp(stream))
        out[f"edt_query 2^20 queries, {name} (edt_query_kernel)"] = span(fn, 10)
    print("VALIDATE_TIME_JSON " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_var", "libgtop_parent.so"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate"))
    ap.add_argument("--bench-rounds", type=int, default=2, help="alternating bench.py runs per build (0 = none)")
    ap.add_argument("--child", choices=("fused", "composed"))
    a = ap.parse_args()
    if a.child:
        return child(a.child == "fused")
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "composed" if who == "parent" else "fused"],
                               env=env, capture_output=True, text=True, timeout=500)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("VALIDATE_TIME_JSON ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{who} child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[who].append(json.loads(line[0].split(" ", 1)[1]))
            print(f"{who}: done", flush=True)
    best = {who: {k: min(r[k] for r in rs) for k in rs[0]} for who, rs in runs.items()}
    spread = {who: {k: max(r[k] for r in rs) / min(r[k] for r in rs) - 1 for k in rs[0]} for who, rs in runs.items()}
    bench = {"parent": [], "this": []}
    for _ in range(a.bench_rounds):
        for who in ("parent", "this"):
            env = dict(os.environ)
            if who == "parent":
                env["GTOP_HIP_LIB"] = os.path.realpath(a.parent_lib)
            else:
                env.pop("GTOP_HIP_LIB", None)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "100"],
                               env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
            res = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{") and '"value"' in ln]
            if p.returncode != 0 or not res:
                sys.exit(f"bench.py on the {who} build failed ({p.returncode}):\n{p.stderr[-2000:]}")
            bench[who].append(res[-1]["value"])
    bench_line = None
    if a.bench_rounds:
        fm = lambda v: " / ".join(f"{x / 1e6:.2f}" for x in v)
        pv, tv = bench["parent"], bench["this"]
        bench_line = (f"`bench.py --gpus 1 --steps 2000 --warmup 100`, {a.bench_rounds} alternating runs per build (parent first), "
                      f"M evals/s: parent {fm(pv)}; this build {fm(tv)}; means {sum(tv) / len(tv) / (sum(pv) / len(pv)):.4f} of the "
                      f"parent's; the parent's own runs differ by {(max(pv) / min(pv) - 1) * 100:.2f} %, this build's by "
                      f"{(max(tv) / min(tv) - 1) * 100:.2f} %")
    lines = ["| size | (a) composed, parent build, us | (a) composed, this build, us | (b) fused, us | (b) / (a) parent | (b) <= (a) "
             "| (a') compacted, no reduction, parent build, us | (b) / (a') |",
             "|---|---|---|---|---|---|---|---|"]
    ratios, failed = {}, []
    for B in BATCHES:
        for nbox in BOXES:
            ka, kb = f"composed B={B} boxes={nbox}", f"fused B={B} boxes={nbox}"
            pa, ta, fb = best["parent"][ka], best["this"][ka], best["this"][kb]
            ok = fb <= pa and fb <= ta
            ratios[f"B={B} boxes={nbox}"] = fb / pa
            if not ok:
                failed.append(f"B={B} boxes={nbox}")
            pc = best["parent"][f"compacted B={B} boxes={nbox}"]
            lines.append(f"| B = {B}, {nbox} boxes | {pa:.1f} | {ta:.1f} | {fb:.1f} | {fb / pa:.3f} | {'yes' if ok else 'NO'} "
                         f"| {pc:.1f} | {fb / pc:.3f} |")
    lines += ["", "| existing kernel (shared header) | parent build, us | this build, us | this / parent | parent's spread over rounds | inside it |",
              "|---|---|---|---|---|---|"]
    for k in best["parent"]:
        if "kernel)" not in k:
            continue
        pa, th, sp = best["parent"][k], best["this"][k], spread["parent"][k]
        lines.append(f"| {k} | {pa:.1f} | {th:.1f} | {th / pa:.3f} | {sp * 100:.1f} % | {'yes' if th / pa - 1 <= sp else 'NO'} |")
    table = "\n".join(lines)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "validate_time.json"), "w") as f:
        json.dump(dict(runs=runs, best_us=best, fused_over_composed=ratios, rows_failing=failed, rounds=a.rounds,
                       bench_evals_per_s=bench, bench_line=bench_line), f, indent=1)
    with open(os.path.join(a.out, "validate_time.md"), "w") as f:
        f.write("fp64, m = 6, 200^3 map, dt_sample = 0.01; device-clock spans, minimum over %d alternating rounds of one "
                "fresh process per library; box-skip hit rate: not collected\n\n%s\n\nrows where the fused report is not at "
                "least as fast as the composition (a): %s\n" % (a.rounds, table, ", ".join(failed) if failed else "none"))
        f.write("\n(a) queries a rectangular B x (largest sample count) buffer: %s of its lookups are padding behind the shorter "
                "rows' counts, which the fused report never does.  (a') gathers the real samples into a dense list first and "
                "queries only those; it is timed WITHOUT any per-trajectory reduction, so it is a lower bound of that route.\n"
                % ", ".join(f"{best['parent'][f'padding share B={B}'] * 100:.1f} % at B = {B}" for B in BATCHES))
        if bench_line:
            f.write("\nbench.py A/B in the same call: %s\n" % bench_line)
    print(table)


if __name__ == "__main__":
    main()
