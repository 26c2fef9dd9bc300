#!/usr/bin/env python3
"""Diagnostic: time of gtop_separation_device (its three kernels) and of gtop_select_distinct_device.

usage: tools/separation_time.py [--kernels DIR] [--samples N] [--segments M] [B ...]        (default B: 1024 4096)

Without --kernels: HIP-event time of the whole separation call and of the selection at K = 8, the median of 20 calls
after warm-up, per B.  The three kernels sit inside one entry point, where events cannot be placed between them; so
with --kernels DIR the tool, before it touches the GPU itself, runs one fresh child of itself per B under
`rocprofv3 --kernel-trace --stats` writing into DIR/B<B>, and prints each kernel's average time from the child's
kernel statistics, beside the pair kernel's issue bound: pair-samples x fp64 instructions per pair-sample (10.25 in
the built kernel: tools/kernel_resources.py or the ISA) over 4 SIMDs x 256 CUs x one wave64 instruction per 4 cycles
at the clock the run reports."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.getcwd())

FP64_PER_PAIR_SAMPLE = 10.25     # 3 sub, 3 mul, 2 add, min, max; + 16 quieting v_max per 64 pair-samples (one unrolled chunk)
TILE, CHUNK = 64, 8


def pair_samples(B, n):
    """What the pair kernel computes: whole 64 x 64 tiles of the upper triangle, diagonal tiles included, on the
    samples rounded up to the chunk."""
    tiles = (B + TILE - 1) // TILE
    return tiles * (tiles + 1) // 2 * TILE * TILE * ((n + CHUNK - 1) // CHUNK * CHUNK)


def run(Bs, n, m, repeats=20):
    import numpy as np
    import torch
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import separation as gs
    ctx = gtop.GtopContext(0)
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    print(f"device {props.name}, {props.multi_processor_count} CUs", flush=True)
    for B in Bs:
        rng = np.random.default_rng(B)
        coeff = torch.tensor(rng.uniform(-1.0, 1.0, (B, m, 18)) * np.tile([3.0, 2.0, 1.0, 0.5, 0.25, 0.125], 3), device=dev)
        T = torch.tensor(rng.uniform(0.4, 1.1, (B, m)), device=dev)
        opts = gs.GtopSepOpts(t_lo=0.0, dt=0.6 * m / (n - 1), n_samples=n, radius=0.5, hold_ends=True)
        pmin, pmax = torch.empty(B, B, dtype=torch.float64, device=dev), torch.empty(B, B, dtype=torch.float64, device=dev)
        rows = torch.empty(B, 6, dtype=torch.float64, device=dev)
        work = torch.empty(gs.separation_workspace_bytes(B, n), dtype=torch.uint8, device=dev)
        cost = torch.tensor(rng.uniform(0.0, 1.0, B), device=dev)
        chosen, count = torch.empty(8, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)

        def sep():
            gs.separation_device(ctx, coeff, T, opts, pmin, pmax, rows, work=work)

        def sel():
            gs.select_distinct_device(ctx, None, cost, pmax, 1.0, 8, chosen=chosen, count=count)

        for name, fn in (("separation_device", sep), ("select_distinct_device K=8", sel)):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            times.sort()
            print(f"B={B} m={m} n_samples={n} {name}: median {times[len(times) // 2]:.1f} us, min {times[0]:.1f} us "
                  f"(HIP events, {repeats} calls)", flush=True)
        print(f"B={B} chosen {chosen.tolist()} count {count.item()} pair-samples {pair_samples(B, n):.4g}", flush=True)
    ctx.close()


def kernel_stats(directory):
    """{kernel name: (calls, average ns)} of a rocprofv3 --kernel-trace --stats run."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                if "sep_" in name:
                    out[name] = (int(row.get("Calls", 0)), float(row.get("AverageNs", "nan")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", metavar="DIR")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--segments", type=int, default=6)
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock of the issue bound")
    ap.add_argument("B", nargs="*", type=int)
    a = ap.parse_args()
    Bs = a.B or [1024, 4096]
    if not a.kernels:
        run(Bs, a.samples, a.segments)
        return
    for B in Bs:
        d = os.path.join(a.kernels, f"B{B}")
        os.makedirs(d, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--samples", str(a.samples), "--segments", str(a.segments), str(B)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            sys.exit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        stats = kernel_stats(d)
        if not stats:
            sys.exit(f"no kernel statistics under {d}")
        for name, (calls, avg) in sorted(stats.items()):
            short = re.search(r"sep_\w+", name).group(0)
            line = f"B={B} n_samples={a.samples} {short}: {avg / 1e3:.1f} us average of {calls} launches"
            if "sep_pairs" in name:
                bound = pair_samples(B, a.samples) * FP64_PER_PAIR_SAMPLE / 64 / (4 * 256) * 4 / (a.clock_ghz * 1e3)
                line += f"; issue bound at {a.clock_ghz} GHz {bound:.1f} us = {100 * bound / (avg / 1e3):.0f} % reached"
            print(line, flush=True)


if __name__ == "__main__":
    main()
