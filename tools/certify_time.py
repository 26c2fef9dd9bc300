#!/usr/bin/env python3
"""Device time of the continuous-time clearance certificate (gtop_certify_trajectories_device) beside the sampled
report (gtop_validate_trajectories_device) on the same OPTIMISED trajectories: B = 1 024 and 16 384 rows of 6 segments
on the 200^3 map, static field.

  (a) the sampled report at dt_sample = 0.01 from a PARENT build of the library,
  (b) the same from this build (the report's kernels include the shared lookup header this build added a helper to),
  (c) the certificate at the default options (max_depth 2, max_refine 256) and the report's margin, this build, with
      the mean refinements per row and the share of each verdict.

Times are spans of the device's own clock between two one-lane stamp kernels (gtop_device_clock_stamp), never host
timers.  One child process per library and round, the parent build and this build alternating; each row's minimum is
taken, and the parent's own spread of (a) over the rounds is the yardstick for (b).  (c) / (a) is recorded, not gated.
The tool also runs the headline benchmark on both builds, alternating, and writes that line under the table.  It writes
certify_time.{md,json}.

With --boxes the subject is the certificate against the moving boxes (gtop_certify_moving_device) instead: 0, 8 and 32
boxes of each kind of list fly through the map; the parent build gives the sampled report with the same boxes
(use_boxes, dt_sample = 0.01) and the static certificate, this build the static certificate and the moving one; the
static certificate of the two builds is compared inside the parent's own spread.  It writes certify_moving_time.{md,json}.

With --ab both builds run the same child, so that every launch of this build — the certificates included — stands beside
the parent's from the same call, each inside or outside the parent's own spread: certify_ab.{md,json} (with --boxes:
certify_moving_ab).  With --rows nothing is timed: one fresh child per library runs the three certificates (static,
moving, kinematic) on the rows of the device tests — every kind of field, both kinds of box list, a list longer than a
staging chunk, max_depth 0 .. 3, max_refine 0 / 1 / 256, limits on and off — and the two sets of output rows are
compared bit for bit: certify_rows.json, exit status 1 unless every row is equal.

usage: tools/certify_time.py [--parent-lib build_var/libgtop_parent.so] [--rounds 3] [--bench-rounds 2]
                             [--out profiles/certify] [--boxes] [--ab | --rows]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1024, 16384)
DT, MARGIN, EVALS = 0.01, 0.3, 20
BOX_COUNTS = (0, 8, 32)


def make_boxes(mp, n, poly, seed=7):
    """n boxes of 0.5 .. 1.5 m that fly through the map at up to 1 m/s; polynomial: with a second and third order term,
    every other one on a validity interval that ends at 3 s.  -> the arguments of the context's setter"""
    import numpy as np
    rng = np.random.default_rng(seed)
    lo, size = np.asarray(mp.origin, dtype=np.float64), np.asarray(mp.map_size, dtype=np.float64)
    p0 = lo + rng.uniform(0.1, 0.9, (n, 3)) * size
    vel = rng.uniform(-1.0, 1.0, (n, 3))
    scale = rng.uniform(0.5, 1.5, (n, 3))
    if not poly:
        return p0, vel, scale
    coef = np.zeros((n, 3, 6))
    coef[:, :, 0], coef[:, :, 1] = p0, vel
    coef[:, :, 2], coef[:, :, 3] = rng.uniform(-0.1, 0.1, (n, 3)), rng.uniform(-0.01, 0.01, (n, 3))
    t_range = np.tile([-np.inf, np.inf], (n, 1))
    t_range[::2] = (0.0, 3.0)
    return coef, scale, t_range


def child(certify, boxes=False):
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

    out = {}
    for B in BATCHES:
        b = problem.make_trajectories(B, 6, mp, seed=1)
        ctx.set_problem(b.T, b.Df)
        lb, ub = ctx.default_bounds(b.waypoints)
        x, _ = ctx.optimize_batch(b.x, lb, ub, EVALS)
        coeff_h, _ = ctx.trajectory_stats(x, DT)
        coeff = torch.tensor(coeff_h, device=dev)
        T = torch.tensor(b.T, device=dev)
        report = torch.empty(B, 12, dtype=torch.float64, device=dev)
        lim = gtop.GtopLimits(margin=MARGIN)
        reps = 20 if B == 1024 else 5
        if boxes:
            cert = torch.empty(B, 8, dtype=torch.float64, device=dev)
            static = gtop.GtopCertifyOpts(margin=MARGIN)
            out[f"certificate, static B={B}"] = span(lambda: gtop.certify_device(ctx, coeff, T, static, cert=cert), reps)
            with_boxes = gtop.GtopLimits(margin=MARGIN, use_boxes=True)
            for poly in (False, True):
                for n in BOX_COUNTS:
                    kind = f"{n} {'polynomial' if poly else 'constant-velocity'} boxes B={B}"
                    if poly:
                        ctx.set_moving_box_polynomials(*make_boxes(mp, n, True))
                    else:
                        ctx.set_moving_boxes(*make_boxes(mp, n, False))
                    if not certify:     # the parent build: the sampled report with the boxes
                        out[f"report, {kind}"] = span(
                            lambda: ctx.validate_device(coeff, T, with_boxes, dt_sample=DT, report=report), reps)
                        continue
                    mo = gtop.GtopCertifyMovingOpts(margin=MARGIN)
                    out[f"certificate, {kind}"] = span(lambda: gtop.certify_moving_device(ctx, coeff, T, mo, cert=cert), reps)
                    torch.cuda.synchronize()
                    c = cert.cpu().numpy()
                    out[f"mean refinements per row, {kind}"] = float(c[:, 6].mean())
                    out[f"share safe, {kind}"] = float((c[:, 0] == 1).mean())
                    assert np.all(c[:, 1] <= c[:, 2])
            ctx.set_moving_boxes(*make_boxes(mp, 0, False))
            continue
        out[f"report B={B}"] = span(lambda: ctx.validate_device(coeff, T, lim, dt_sample=DT, report=report), reps)
        if certify:
            cert = torch.empty(B, 8, dtype=torch.float64, device=dev)
            opts = gtop.GtopCertifyOpts(margin=MARGIN)
            out[f"certificate B={B}"] = span(lambda: gtop.certify_device(ctx, coeff, T, opts, cert=cert), reps)
            level0 = gtop.GtopCertifyOpts(margin=MARGIN, max_depth=0, max_refine=0)
            out[f"certificate, level 0 only B={B}"] = span(lambda: gtop.certify_device(ctx, coeff, T, level0, cert=cert), reps)
            gtop.certify_device(ctx, coeff, T, opts, cert=cert)
            torch.cuda.synchronize()
            c, r = cert.cpu().numpy(), report.cpu().numpy()
            out[f"mean refinements per row B={B}"] = float(c[:, 6].mean())
            out[f"rows that spend refinements B={B}"] = float((c[:, 6] > 0).mean())
            for name, v in (("unsafe", -1), ("undecided", 0), ("safe", 1)):
                out[f"share {name} B={B}"] = float((c[:, 0] == v).mean())
            out[f"share passing the sampled report B={B}"] = float(((r[:, 4] == 0) & (r[:, 6] == 0)).mean())
            out[f"rows the report passes and the certificate calls unsafe B={B}"] = int(
                ((r[:, 4] == 0) & (r[:, 6] == 0) & (c[:, 0] == -1)).sum())
            assert np.all(c[:, 1] <= c[:, 2])
    print("CERTIFY_TIME_JSON " + json.dumps(out), flush=True)


def child_rows(path):
    """The output rows of the three certificates on the device tests' inputs (tests/*_twin.py), into an .npz."""
    import itertools

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import grad_traj_optimization_amd as gtop
    from oracle import oracle
    from tests import certify_moving_twin as cm
    from tests import certify_twin as ct
    from tests import kinematics_twin as kt

    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda:0")
    host = lambda t: t.cpu().numpy()          # (waits for the launch: the context's setters below do not)
    out = {}
    sweep = list(itertools.product(range(4), (0, 1, 256)))
    perm = np.random.default_rng(2).permutation(65) % 5
    for kind, margin in zip(ct.FIELDS, (0.2, 0.2, 0.0, 0.3)):
        field, mp = ct.make_field(oracle, kind)
        ctx = gtop.GtopContext(0)
        ctx.set_sdf(field.val, ct.GRID, mp.origin, ct.RES, mp.map_size)
        c5, T5, _ = ct.make_rows(oracle, mp, 5, 3, 31)
        batches = [(dev(c5[perm]), dev(T5[perm]), margin)]
        for k, m, B, seed, mg, _, _ in ct.CASES.values():
            if k == kind:
                batches.append((*map(dev, ct.make_rows(oracle, mp, B, m, seed)[:2]), mg))
        for i, (c, T, mg) in enumerate(batches):
            for depth, refine in sweep:
                out[f"static/{kind}/{i}/{depth}/{refine}"] = host(gtop.certify_device(ctx, c, T, gtop.GtopCertifyOpts(mg, depth, refine)))
            if kind not in ("esdf", "signed"):
                continue
            ctx.set_start_times(np.linspace(0.0, 3.0, c.shape[0]))
            for poly in (False, True):
                few = cm.shared_boxes(mp, poly)
                rng = np.random.default_rng(9)
                shift = rng.uniform(-1.0, 1.0, (70, 3))
                pick = np.arange(70) % 3
                if poly:                                   # 70 boxes: past a staging chunk of either kind
                    coef = few.coef[pick].copy()
                    coef[:, :, 0] += shift
                    many = cm.Boxes.polynomial(coef, few.scale[pick], few.t_range[pick])
                else:
                    many = cm.Boxes.const_vel(few.p0[pick] + shift, few.vel[pick], few.scale[pick])
                for name, boxes, options in (("few", few, sweep), ("many", many, ((2, 16), (3, 1), (0, 0)))):
                    boxes.set_on(ctx)
                    for depth, refine in options:
                        out[f"moving/{kind}/{i}/{poly}/{name}/{depth}/{refine}"] = host(gtop.certify_moving_device(
                            ctx, c, T, gtop.GtopCertifyMovingOpts(mg, depth, refine)))
            ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
            ctx.set_start_times(None)
        ctx.close()
    ctx = gtop.GtopContext(0)
    ctx.set_sdf(np.full((24, 24, 24), 10.0), (24, 24, 24), (-6.0, -6.0, -6.0), 0.5)
    for B, m, seed in kt.BATCHES:
        coeff, T = kt.random_rows(B, m, seed)
        mv, ma, _ = kt.batch_limits(coeff, T)
        c, T = dev(coeff), dev(T)
        small = B <= 3 and m <= 7
        for (v, a), (depth, refine) in itertools.product(((0.0, 0.0), (mv, 0.0), (0.0, ma), (mv, ma)),
                                                         sweep if small else ((2, 256), (3, 1), (0, 0))):
            for per_axis in (False, True):
                kin, seg = gtop.certify_kinematics_device(ctx, c, T, gtop.GtopKinOpts(v, a, per_axis, depth, refine))
                key = f"kin/{B}/{m}/{v > 0}/{a > 0}/{per_axis}/{depth}/{refine}"
                out[key], out[key + "/seg"] = host(kin), host(seg)
    ctx.close()
    np.savez_compressed(path, **out)
    print("CERTIFY_ROWS_JSON " + json.dumps(dict(arrays=len(out), rows=int(sum(len(v.reshape(-1, v.shape[-1])) for v in out.values())))),
          flush=True)


def compare_rows(a):
    """--rows: one child per library, the parent first; every output row of the two compared bit for bit."""
    import numpy as np
    os.makedirs(a.out, exist_ok=True)
    files, counts = {}, {}
    for who in ("parent", "this"):
        files[who] = os.path.join(a.out, f"certify_rows_{who}.npz")
        line = run_child(who, a.parent_lib, [os.path.abspath(__file__), "--child", "rows", "--dump", files[who]],
                         "CERTIFY_ROWS_JSON ", 900)
        counts[who] = json.loads(line.split(" ", 1)[1])
        print(f"{who}: {counts[who]}", flush=True)
    pa, th = np.load(files["parent"]), np.load(files["this"])
    bits = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    differ = [k for k in pa.files if k not in th.files or pa[k].shape != th[k].shape or not np.array_equal(bits(pa[k]), bits(th[k]))]
    differ += [k for k in th.files if k not in pa.files]
    res = dict(counts, differing=differ, by_kind={p: sum(k.startswith(p) for k in pa.files) for p in ("static", "moving", "kin")})
    with open(os.path.join(a.out, "certify_rows.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 1 if differ else 0


def run_child(who, parent_lib, args, prefix, timeout):
    env = dict(os.environ)
    if who == "parent":
        env["GTOP_HIP_LIB"] = os.path.realpath(parent_lib)
    else:
        env.pop("GTOP_HIP_LIB", None)
    p = subprocess.run([sys.executable, *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(prefix)]
    if p.returncode != 0 or not line:
        sys.exit(f"{who} child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return line[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_var", "libgtop_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify"))
    ap.add_argument("--bench-rounds", type=int, default=2, help="alternating bench.py runs per build (0 = none)")
    ap.add_argument("--child", choices=("certify", "report", "rows"))
    ap.add_argument("--dump", help="(--child rows) the .npz to write")
    ap.add_argument("--boxes", action="store_true", help="the certificate against the moving boxes (see above)")
    ap.add_argument("--ab", action="store_true", help="both builds run every launch (see above)")
    ap.add_argument("--rows", action="store_true", help="compare the two builds' output rows bit for bit (see above)")
    a = ap.parse_args()
    if a.child == "rows":
        return child_rows(a.dump)
    if a.child:
        return child(a.child == "certify", a.boxes)
    if not os.path.exists(a.parent_lib):
        sys.exit(f"no parent build at {a.parent_lib}: make -C grad_traj_optimization_amd/csrc lib OUT=... on the parent commit")
    if a.rows:
        return compare_rows(a)
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):                                   # alternating, one fresh process each
        for who in ("parent", "this"):
            line = run_child(who, a.parent_lib, [os.path.abspath(__file__), "--child", "report" if who == "parent" and not a.ab else "certify",
                                                 *(["--boxes"] if a.boxes else [])], "CERTIFY_TIME_JSON ", 400)
            runs[who].append(json.loads(line.split(" ", 1)[1]))
            print(f"{who}: done", flush=True)
    timed = lambda k: k.startswith(("report", "certificate"))
    best = {who: {k: min(r[k] for r in rs) for k in rs[0] if timed(k)} for who, rs in runs.items()}
    spread = {k: max(r[k] for r in runs["parent"]) / min(r[k] for r in runs["parent"]) - 1 for k in best["parent"]}
    facts = {k: v for k, v in runs["this"][0].items() if not timed(k)}
    bench = {"parent": [], "this": []}
    for _ in range(a.bench_rounds):
        for who in ("parent", "this"):
            line = run_child(who, a.parent_lib, [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "100"],
                             "{", 300)
            bench[who].append(json.loads(line)["value"])
    bench_line = None
    if a.bench_rounds:
        fm = lambda v: " / ".join(f"{x / 1e6:.2f}" for x in v)
        pv, tv = bench["parent"], bench["this"]
        bench_line = (f"`bench.py --gpus 1 --steps 2000 --warmup 100`, {a.bench_rounds} alternating runs per build (parent first), "
                      f"M evals/s: parent {fm(pv)}; this build {fm(tv)}; means {sum(tv) / len(tv) / (sum(pv) / len(pv)):.4f} of the "
                      f"parent's; the parent's own runs differ by {(max(pv) / min(pv) - 1) * 100:.2f} %, this build's by "
                      f"{(max(tv) / min(tv) - 1) * 100:.2f} %")
    if a.ab:
        return write_ab(a, runs, best, spread, bench, bench_line)
    if a.boxes:
        return write_moving(a, runs, best, spread, facts, bench, bench_line)
    lines = ["| B | (a) report, parent build, us | (b) report, this build, us | (b) / (a) | parent's spread of (a) | inside it "
             "| (c) certificate, us | (c) / (a) | level 0 only, us | mean refinements per row |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    failed = []
    for B in BATCHES:
        pa, tb, sp = best["parent"][f"report B={B}"], best["this"][f"report B={B}"], spread[f"report B={B}"]
        c, c0 = best["this"][f"certificate B={B}"], best["this"][f"certificate, level 0 only B={B}"]
        ok = tb / pa - 1 <= sp
        if not ok:
            failed.append(f"B={B}")
        lines.append(f"| {B} | {pa:.1f} | {tb:.1f} | {tb / pa:.3f} | {sp * 100:.1f} % | {'yes' if ok else 'NO'} | {c:.1f} | {c / pa:.2f} "
                     f"| {c0:.1f} | {facts[f'mean refinements per row B={B}']:.2f} |")
    table = "\n".join(lines)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "certify_time.json"), "w") as f:
        json.dump(dict(runs=runs, best_us=best, parent_spread=spread, facts=facts, report_outside_parent_spread=failed,
                       rounds=a.rounds, bench_evals_per_s=bench, bench_line=bench_line), f, indent=1)
    with open(os.path.join(a.out, "certify_time.md"), "w") as f:
        f.write("fp64, m = 6, 200^3 map, static field, rows optimised for %d evaluations, margin %.1f, dt_sample = %.2f, "
                "certificate at max_depth 2 / max_refine 256; device-clock spans, minimum over %d alternating rounds of one "
                "fresh process per library\n\n%s\n\nsizes where (b) lies outside the parent's own spread of (a): %s\n\n"
                % (EVALS, MARGIN, DT, a.rounds, table, ", ".join(failed) if failed else "none"))
        for k, v in facts.items():
            f.write(f"- {k}: {v:.4g}\n")
        if bench_line:
            f.write("\nbench.py A/B in the same call: %s\n" % bench_line)
    print(table)
    print(json.dumps(facts))
    if bench_line:
        print(bench_line)


def write_ab(a, runs, best, spread, bench, bench_line):
    """certify[_moving]_ab.{md,json}: every launch, the parent build's least beside this build's, and the parent's spread."""
    lines = ["| launch | parent build, us | this build, us | ratio | parent's spread | inside it |", "|---|---|---|---|---|---|"]
    outside = []
    for k, pa in best["parent"].items():
        tb, sp = best["this"][k], spread[k]
        if tb / pa - 1 > sp:
            outside.append(k)
        lines.append(f"| {k} | {pa:.1f} | {tb:.1f} | {tb / pa:.4f} | {sp * 100:.2f} % | {'NO' if k in outside else 'yes'} |")
    table = "\n".join(lines)
    name = os.path.join(a.out, "certify_moving_ab" if a.boxes else "certify_ab")
    os.makedirs(a.out, exist_ok=True)
    with open(name + ".json", "w") as f:
        json.dump(dict(runs=runs, best_us=best, parent_spread=spread, outside_parent_spread=outside, rounds=a.rounds,
                       bench_evals_per_s=bench, bench_line=bench_line), f, indent=1)
    with open(name + ".md", "w") as f:
        f.write("least of %d alternating rounds of one fresh process per library, the parent first; device-clock spans\n\n%s\n"
                % (a.rounds, table))
        if bench_line:
            f.write("\nbench.py A/B in the same call: %s\n" % bench_line)
    print(table)
    if bench_line:
        print(bench_line)


def write_moving(a, runs, best, spread, facts, bench, bench_line):
    """certify_moving_time.{md,json}: per batch and list, the parent's sampled report beside this build's certificate."""
    lines = ["| B | list | report with boxes, parent build, us | moving certificate, this build, us | ratio "
             "| mean refinements per row | share SAFE |", "|---|---|---|---|---|---|---|"]
    static, failed = [], []
    for B in BATCHES:
        k = f"certificate, static B={B}"
        pa, tb, sp = best["parent"][k], best["this"][k], spread[k]
        ok = tb / pa - 1 <= sp
        if not ok:
            failed.append(f"B={B}")
        static.append(f"- static certificate B={B}: parent {pa:.1f} us, this build {tb:.1f} us, ratio {tb / pa:.3f}; the "
                      f"parent's own spread {sp * 100:.1f} %: {'inside' if ok else 'OUTSIDE'}")
        for poly in ("constant-velocity", "polynomial"):
            for n in BOX_COUNTS:
                kind = f"{n} {poly} boxes B={B}"
                r, c = best["parent"][f"report, {kind}"], best["this"][f"certificate, {kind}"]
                lines.append(f"| {B} | {n} {poly} | {r:.1f} | {c:.1f} | {c / r:.2f} | "
                             f"{facts[f'mean refinements per row, {kind}']:.2f} | {facts[f'share safe, {kind}']:.3f} |")
    table = "\n".join(lines)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "certify_moving_time.json"), "w") as f:
        json.dump(dict(runs=runs, best_us=best, parent_spread=spread, facts=facts, static_outside_parent_spread=failed,
                       rounds=a.rounds, bench_evals_per_s=bench, bench_line=bench_line), f, indent=1)
    with open(os.path.join(a.out, "certify_moving_time.md"), "w") as f:
        f.write("fp64, m = 6, 200^3 map, rows optimised for %d evaluations, margin %.1f, start time 0, report at dt_sample = "
                "%.2f, certificates at max_depth 2 / max_refine 256; device-clock spans, minimum over %d alternating rounds "
                "of one fresh process per library\n\n%s\n\n%s\n" % (EVALS, MARGIN, DT, a.rounds, table, "\n".join(static)))
        if bench_line:
            f.write("\nbench.py A/B in the same call: %s\n" % bench_line)
    print(table)
    print("\n".join(static))
    if bench_line:
        print(bench_line)


if __name__ == "__main__":
    sys.exit(main())
