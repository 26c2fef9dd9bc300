"""The launch rule of the evaluation kernels (csrc/gtop_launch_rule.cpp: gtop_eval_plan, gtop_eval_plan_moving) on the
CPU: plain C++ that a host compiler builds without any HIP header, pinned plan by plan against a table generated from
the rule as it stood before it was cut out of csrc/gtop_kernels.hip (tests/golden/launch_rule.txt; the dumper is
tests/cpp/launch_rule_dump.cpp).  The GPU test of the switch points is tests/test_gpu_wave.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grad_traj_optimization_amd", "csrc")


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    """csrc/gtop_launch_rule.cpp + the dumper through g++ with csrc/ as the only include path: that it builds is the
    test that the rule is host-only."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("launch_rule") / "launch_rule_dump")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + CSRC, os.path.join(CSRC, "gtop_launch_rule.cpp"),
                          os.path.join(ROOT, "tests", "cpp", "launch_rule_dump.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def test_every_plan_is_the_recorded_one(dumper):
    """(spl, nt, is_long, nw) or "refused" for B across every switch point x m in 1 .. 70, 118, 119, 227, 228 x fp64 /
    fp32 x pinned 0, 3, 6, 10, 30 and an illegal value x evaluation / optimizer loop, and the moving-term rule over the
    same: line for line the golden table (its first line says where it comes from)."""
    out = subprocess.run([dumper], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "launch_rule.txt")).read().splitlines()[1:]
    assert len(got) == len(want) and len(got) > 200
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 2} of tests/golden/launch_rule.txt: expected {w!r}, got {g!r}"


def test_accepted_plans_keep_what_the_launchers_rely_on(dumper):
    """For every plan the rule accepts: gtop_wave_lds_bytes <= 160 KiB, nt * m <= the geometry's segment slots unless the
    body walks the segments in chunks, and gtop_eval_plan_moving accepts only nw == 1 with spl 3 or 6 (the geometries
    that have a moving-term body).  The dumper prints one line per violation."""
    out = subprocess.run([dumper, "--check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "", out.stdout[:2000] + out.stderr
