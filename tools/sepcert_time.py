#!/usr/bin/env python3
"""Diagnostic: time of gtop_certify_separation_device (its kernels: boxes when cull = 1, pairs, rows).

usage: tools/sepcert_time.py [--kernels DIR] [--segments M] [--min-sep D] [B ...]        (default B: 256 1024)

Without --kernels: HIP-event time of the whole call on random rows with cull = 0 and cull = 1, the median of 20 calls
after 5 warm-ups, per B; for scale, the sampled gtop_separation_device call at 256 samples on the same rows; and what
the certificate found (verdict counts, refinements, pairs certified by their boxes).  The kernels sit inside one entry
point, where events cannot be placed between them; so with --kernels DIR the tool, before it touches the GPU itself,
runs one fresh child of itself per B under `rocprofv3 --kernel-trace --stats` writing into DIR/B<B>, and prints each
kernel's average time and its share from the child's kernel statistics."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.getcwd())


def median_us(fn, repeats=20, warmup=5):
    import torch
    for _ in range(warmup):
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
    return times[len(times) // 2], times[0]


def run(Bs, m, min_sep, culls=(0, 1), sampled=True):
    import numpy as np
    import torch
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import separation as gs
    from grad_traj_optimization_amd import separation_certificate as gc
    ctx = gtop.GtopContext(0)
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    print(f"device {props.name}, {props.multi_processor_count} CUs", flush=True)
    for B in Bs:
        rng = np.random.default_rng(B)
        c = rng.uniform(-1.0, 1.0, (B, m, 18)) * np.tile([3.0, 2.0, 1.0, 0.5, 0.25, 0.125], 3)
        c[:, :, 0::6] += rng.uniform(-1.0, 1.0, (B, 1, 3)) * 2.0 * B ** (1.0 / 3.0)     # a swarm of constant density
        coeff = torch.tensor(c, device=dev)
        T = torch.tensor(rng.uniform(0.4, 1.1, (B, m)), device=dev)
        ctx.set_start_times(rng.uniform(0.0, 0.5, B))
        pairs = torch.empty(B, B, 8, dtype=torch.float64, device=dev)
        rows = torch.empty(B, 10, dtype=torch.float64, device=dev)
        work = torch.empty(gc.sepcert_workspace_bytes(B), dtype=torch.uint8, device=dev)
        for cull in culls:
            opts = gc.GtopSepCertOpts(min_sep=min_sep, max_depth=2, max_refine=64, cull=cull)
            med, least = median_us(lambda: gc.certify_separation_device(ctx, coeff, T, opts, pairs, rows, work=work))
            v = pairs[..., 0]
            off = ~torch.eye(B, dtype=torch.bool, device=dev)
            print(f"B={B} m={m} min_sep={min_sep} cull={cull} certify_separation_device: median {med:.1f} us, min "
                  f"{least:.1f} us (HIP events, 20 calls); pairs {B * (B - 1) // 2}: safe {int(((v == 1) & off).sum()) // 2} "
                  f"undecided {int(((v == 0) & off).sum()) // 2} unsafe {int(((v == -1) & off).sum()) // 2}, by boxes "
                  f"{int((pairs[..., 7] == -1).sum()) // 2}, refinements {int(pairs[..., 6].sum()) // 2}, pieces "
                  f"{int(pairs[..., 7].clamp(min=0).sum()) // 2}", flush=True)
        if sampled:
            n = 256
            sopts = gs.GtopSepOpts(t_lo=0.0, dt=(0.5 + 1.1 * m) / (n - 1), n_samples=n, radius=min_sep)
            pmin, pmax = (torch.empty(B, B, dtype=torch.float64, device=dev) for _ in range(2))
            srows = torch.empty(B, 6, dtype=torch.float64, device=dev)
            swork = torch.empty(gs.separation_workspace_bytes(B, n), dtype=torch.uint8, device=dev)
            med, least = median_us(lambda: gs.separation_device(ctx, coeff, T, sopts, pmin, pmax, srows, work=swork))
            print(f"B={B} m={m} n_samples={n} separation_device (sampled, for scale): median {med:.1f} us, min "
                  f"{least:.1f} us; pairs with pair_min < {min_sep}: {int((pmin < min_sep).sum()) // 2}", flush=True)
        ctx.set_start_times(None)
    ctx.close()


def kernel_stats(directory):
    """{kernel name: (calls, average ns, total ns)} of a rocprofv3 --kernel-trace --stats run."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                if "sepcert_" in name:
                    out[name] = (int(row.get("Calls", 0)), float(row.get("AverageNs", "nan")),
                                 float(row.get("TotalDurationNs", "nan")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", metavar="DIR")
    ap.add_argument("--segments", type=int, default=6)
    ap.add_argument("--min-sep", type=float, default=0.5)
    ap.add_argument("--cull", type=int, choices=(0, 1), help="one value of cull only, and no sampled call (the children)")
    ap.add_argument("B", nargs="*", type=int)
    a = ap.parse_args()
    Bs = a.B or [256, 1024]
    if not a.kernels:
        if a.cull is None:
            run(Bs, a.segments, a.min_sep)
        else:
            run(Bs, a.segments, a.min_sep, culls=(a.cull,), sampled=False)
        return
    for B in Bs:
        for cull in (0, 1):
            d = os.path.join(a.kernels, f"B{B}_cull{cull}")
            os.makedirs(d, exist_ok=True)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--segments", str(a.segments), "--min-sep", str(a.min_sep), "--cull",
                   str(cull), str(B)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            stats = kernel_stats(d)
            if not stats:
                sys.exit(f"no kernel statistics under {d}")
            total = sum(t for _, _, t in stats.values())
            for name, (calls, avg, tot) in sorted(stats.items()):
                short = re.search(r"sepcert_\w+", name).group(0)
                print(f"B={B} cull={cull} {short}: {avg / 1e3:.1f} us average of {calls} launches, "
                      f"{100 * tot / total:.1f} % of the call's kernel time", flush=True)


if __name__ == "__main__":
    main()
