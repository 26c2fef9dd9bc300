#!/usr/bin/env python3
"""Device time of the waypoint insertion (gtop_insert_waypoints_device) beside a hipMemcpyAsync device-to-device copy of
as many bytes as the launch writes, on the same device in the same process.  No threshold is set: the tool writes down
what comes out.

Device-clock spans between two one-lane stamp kernels (gtop_device_clock_stamp, as bench.py times its region) around
back-to-back launches; the forms and the copy alternate span by span, so that a drift of the clocks or another tenant of
the machine touches all of them; minimum and median of the spans.  16 384 trajectories of 6 segments and 8 192 of 40;
random-walk waypoints, per-row times.  The bytes of a launch are counted from the shapes: what it must read (x, T, the
cut segment's 18 coefficients, when, lb, ub) and what it writes (x_out, T_out, lb_out, ub_out, info).  Before timing,
the first rows are checked against the numpy twin (tests/insert_twin.py), bit for bit.

usage: tools/insert_time.py [--out profiles/insert_waypoints]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((16384, 6), (8192, 40))
SPANS, REPS = 9, 20
HBM_PEAK = 8.0e12          # bytes / s, the MI355X data sheet


def hip_runtime():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise SystemExit("no libamdhip64.so to call hipMemcpyAsync through")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insert_waypoints"))
    a = ap.parse_args()

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from grad_traj_optimization_amd import insert, problem
    from tests import insert_twin as it

    dev = torch.device("cuda:0")
    ctx = gtop.GtopContext(0)
    hz = ctx.clock_hz()
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    init = torch.tensor([2 ** 63 - 1, 0], dtype=torch.int64, device=dev)
    stamps = init.clone()

    def one_span(fn):
        stamps.copy_(init)
        ctx.clock_stamp(stamps)
        for _ in range(REPS):
            fn()
        ctx.clock_stamp(stamps)
        torch.cuda.synchronize()
        s = stamps.tolist()
        return (s[1] - s[0]) / hz * 1e6 / REPS

    def spans(fns):
        """us per call of each fn: SPANS spans each, alternating; sustained clocks first."""
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.2:
            for fn in fns:
                fn()
            torch.cuda.synchronize()
        got = [[] for _ in fns]
        for _ in range(SPANS):
            for k, fn in enumerate(fns):
                got[k].append(one_span(fn))
        return [dict(min_us=float(np.min(g)), median_us=float(np.median(g)), max_us=float(np.max(g))) for g in got]

    mp = problem.make_map(100, density=0.02, seed=0)
    rows = []
    for B, m in SHAPES:
        b = problem.make_trajectories(B, m, mp, seed=1)
        x, Df, T = (torch.tensor(v, device=dev) for v in (b.x, b.Df.reshape(-1, 18), b.T))
        coeff = ctx.coefficients_device(x, Df, T)
        lbh, ubh = ctx.default_bounds(b.waypoints)
        lb, ub = torch.tensor(lbh, device=dev), torch.tensor(ubh, device=dev)
        wh = np.random.default_rng(2).uniform(0.0, 1.0, B) * b.T.sum(axis=1)
        when = torch.tensor(wh, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        x_out, T_out, info = torch.empty(B, 9 * m, **f64), torch.empty(B, m + 1, **f64), torch.empty(B, 6, **f64)
        lb_out, ub_out = torch.empty(B, 9 * m, **f64), torch.empty(B, 9 * m, **f64)
        at, longest = gtop.GtopInsert(mode=0, min_fraction=0.1), gtop.GtopInsert(mode=1, min_fraction=0.1)
        outs = dict(x_out=x_out, T_out=T_out, info=info)
        with_bounds = dict(outs, lb=lb, ub=ub, lb_out=lb_out, ub_out=ub_out)
        # what is timed is right: the first rows against the twin
        insert.insert_waypoints_device(ctx, at, x, coeff, T, when=when, **with_bounds)
        torch.cuda.synchronize()
        k = 64
        want = it.insert_batch(m, b.x[:k], coeff[:k].cpu().numpy(), b.T[:k], when=wh[:k], lb=lbh[:k], ub=ubh[:k],
                               mode=it.AT_TIME, min_fraction=0.1)
        for name, t in (("x_out", x_out), ("T_out", T_out), ("lb_out", lb_out), ("ub_out", ub_out), ("info", info)):
            assert np.array_equal(t[:k].cpu().numpy().view(np.uint64), want[name].view(np.uint64)), name
        d = 8
        read = B * (9 * (m - 1) + m + 18 + 1) * d
        written = B * (9 * m + (m + 1) + 6) * d
        read_b, written_b = read + B * 18 * (m - 1) * d, written + B * 18 * m * d
        src, dst = torch.empty(written_b // d, **f64), torch.empty(written_b // d, **f64)
        src.normal_()
        stream = torch.cuda.current_stream().cuda_stream

        def copy():
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), written_b, 3, stream)     # 3: device to device
            assert rc == 0, rc

        t_at_b, t_long_b, t_at, t_copy = spans([
            lambda: insert.insert_waypoints_device(ctx, at, x, coeff, T, when=when, **with_bounds),
            lambda: insert.insert_waypoints_device(ctx, longest, x, coeff, T, **with_bounds),
            lambda: insert.insert_waypoints_device(ctx, at, x, coeff, T, when=when, **outs),
            copy])
        rows.append(dict(B=B, m=m, bytes_read_with_bounds=read_b, bytes_written_with_bounds=written_b, bytes_read=read,
                         bytes_written=written, at_time_bounds=t_at_b, longest_bounds=t_long_b, at_time=t_at,
                         copy_of_written_bytes=t_copy))
        print(rows[-1], flush=True)
    name = torch.cuda.get_device_name(0)
    ctx.close()

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time.json"), "w") as f:
        json.dump(dict(device=name, date=time.strftime("%Y-%m-%d"), spans=SPANS, reps=REPS, hbm_peak=HBM_PEAK, rows=rows),
                  f, indent=1)
    with open(os.path.join(a.out, "time.md"), "w") as f:
        f.write(f"{name}, {time.strftime('%Y-%m-%d')}; fp64; device-clock spans (gtop_device_clock_stamp around {REPS} "
                f"back-to-back launches), {SPANS} spans per entry, the three forms and the copy alternating span by span in "
                "one process: minimum (median) in us per launch.  Bytes = what the launch must read (x, T, 18 coefficients, "
                "when, lb, ub) + what it writes, from the shapes; 'at peak' = those bytes over the data sheet's 8 TB/s; "
                "the copy is one hipMemcpyAsync device-to-device of as many bytes as the launch with bounds WRITES (it "
                "reads as many again).  The first 64 rows of each batch checked against the numpy twin before timing.  "
                "A record, not a gate.\n\n")
        f.write("| B x m | AT_TIME + bounds | LONGEST + bounds | MB read + written | at peak, us | share of peak | "
                "AT_TIME, no bounds | MB | copy of the written bytes | MB copied |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            cell = lambda t: f"{t['min_us']:.1f} ({t['median_us']:.1f})"
            tot_b = r["bytes_read_with_bounds"] + r["bytes_written_with_bounds"]
            at_peak = tot_b / HBM_PEAK * 1e6
            f.write(f"| {r['B']} x {r['m']} | {cell(r['at_time_bounds'])} | {cell(r['longest_bounds'])} | {tot_b / 1e6:.1f} | "
                    f"{at_peak:.1f} | {at_peak / r['at_time_bounds']['min_us']:.2f} | {cell(r['at_time'])} | "
                    f"{(r['bytes_read'] + r['bytes_written']) / 1e6:.1f} | {cell(r['copy_of_written_bytes'])} | "
                    f"{r['bytes_written_with_bounds'] / 1e6:.1f} |\n")


if __name__ == "__main__":
    main()
