"""bench.py's own contract: a plain run times the steps and prints the headline (the checks and the other figures come
with --full), and --dump-outputs writes what the timed path computed in its last step."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module(monkeypatch):
    # importing bench.py sets an environment default for the GPU runtime: undone after the test
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return importlib.import_module("bench")


def _bench(args, timeout=600):
    out = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # exactly ONE JSON line
    return json.loads(lines[0])


def test_dump_outputs_writes_each_array_in_its_own_width(tmp_path, monkeypatch):
    bench = _bench_module(monkeypatch)
    c = np.linspace(1.0, 2.0, 7)
    g = np.arange(21, dtype=np.float32).reshape(7, 3)
    assert bench.dump_outputs(str(tmp_path / "d"), {"cost": c, "grad": g}) is None
    c2, g2 = np.load(tmp_path / "d" / "cost.npy"), np.load(tmp_path / "d" / "grad.npy")
    assert c2.dtype == np.float64 and g2.dtype == np.float32
    assert np.array_equal(c2, c) and np.array_equal(g2, g)


def test_dump_outputs_samples_the_same_rows_of_every_array_under_the_limit(tmp_path, monkeypatch):
    bench = _bench_module(monkeypatch)
    n = 1000
    c = np.arange(n, dtype=np.float64)
    g = np.repeat(c[:, None], 9, axis=1)
    limit = (c.nbytes + g.nbytes) // 4
    rows = bench.dump_outputs(str(tmp_path / "a"), {"cost": c, "grad": g}, limit=limit)
    again = bench.dump_outputs(str(tmp_path / "b"), {"cost": c, "grad": g}, limit=limit)
    assert rows is not None and np.array_equal(rows, again)             # fixed seed: the same sample every run
    assert len(rows) == len(set(rows.tolist())) and np.all(np.diff(rows) > 0)
    c2, g2 = np.load(tmp_path / "a" / "cost.npy"), np.load(tmp_path / "a" / "grad.npy")
    assert c2.nbytes + g2.nbytes <= limit
    assert np.array_equal(c2, rows.astype(np.float64)) and np.array_equal(g2[:, 4], c2)


def test_bench_lists_its_options():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
    bad = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--steps" in bad.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path, dtype, gtop):
    """A plain run: exactly --steps timed steps, the headline fields, none of --full's checks or figures; its dumped
    outputs are the batch's costs and gradients, bit for bit those of a direct evaluation of the same inputs."""
    import torch
    from grad_traj_optimization_amd import problem
    grid, B, m = 100, 512, 6
    r = _bench(["--gpus", "1", "--steps", "30", "--warmup", "3", "--grid", str(grid), "--batch", str(B),
                "--dtype", dtype, "--dump-outputs", str(tmp_path)])
    assert r["steps"] == 30 and r["warmup"] == 3 and r["dtype"] == dtype and r["higher_is_better"] is True
    assert r["unit"] == "evals/s" and r["metric"] == "cost+grad evals/sec (batched trajectories)"
    assert r["ms_per_step"] > 0 and abs(r["value"] - B / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    assert "extras" not in r and "cpu_baseline" not in r and r["parity"] is None
    assert r["roofline"]["launch_us"]["probe"] is None and r["roofline"]["frac"] > 0
    cost, grad = np.load(tmp_path / "cost.npy"), np.load(tmp_path / "grad.npy")
    want = np.float64 if dtype == "f64" else np.float32
    assert cost.dtype == want and grad.dtype == want and cost.shape == (B,) and grad.shape == (B, 9 * (m - 1))

    # the bench's inputs, rebuilt from its seeds, through one direct launch
    td = torch.float64 if dtype == "f64" else torch.float32
    mp = problem.make_map(grid, density=0.02, seed=0)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    b = problem.make_trajectories(B, m, mp, seed=1)
    b = problem.permute(b, problem.spatial_order(b.waypoints, mp.origin, mp.map_size))
    dev = torch.device("cuda:0")
    c, g = ctx.eval_device(torch.tensor(b.x, dtype=td, device=dev), torch.tensor(b.Df.reshape(-1, 18), dtype=td, device=dev),
                           torch.tensor(b.T, dtype=td, device=dev))
    torch.cuda.synchronize()
    assert np.array_equal(cost, c.cpu().numpy()) and np.array_equal(grad, g.cpu().numpy())
    ctx.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_full_run_keeps_the_checks_and_the_other_figures():
    r = _bench(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--cpu-seconds", "1"])
    assert r["parity"]["ok"] and r["steps"] == 20
    assert r["roofline"]["launch_us"]["probe"] > 0 and r["roofline"]["gpu_vs_probe"] > 0
    assert "error" not in r["extras"] and len(r["extras"]["workloads"]) == 4 and "optimizer" in r["extras"]
    assert "error" not in r["cpu_baseline"] and r["cpu_baseline"]["value"] > 0
