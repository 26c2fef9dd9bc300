"""Access to the distance-field builder's launch plan (csrc/gtop_esdf_plan.{h,cpp}) from the tests: the host-only plan
and the dumper tests/cpp/esdf_plan_dump.cpp through g++ with csrc/ as the only include path — the same statement the
library's launcher reads, with or without a GPU.  tests/test_esdf_plan.py pins the plan itself; the GPU tests assert,
shape by shape, the plan cell they are there for."""
import atexit
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grad_traj_optimization_amd", "csrc")

_exe = None


def dumper():
    """Path of the built dumper (built once per process; that it builds is the test that the plan is host-only)."""
    global _exe
    if _exe is None:
        tmp = tempfile.mkdtemp(prefix="esdf_plan_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        exe = os.path.join(tmp, "esdf_plan_dump")
        out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                              os.path.join(CSRC, "gtop_esdf_plan.cpp"),
                              os.path.join(ROOT, "tests", "cpp", "esdf_plan_dump.cpp"), "-o", exe],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        _exe = exe
    return _exe


def _parse(line):
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


def plans(grids):
    """The plan of every (nx, ny, nz) of `grids`: a list of dicts of ints (GtopEsdfPlan's fields)."""
    grids = [tuple(int(v) for v in g) for g in grids]
    out = subprocess.run([dumper(), "plan"] + [str(v) for g in grids for v in g], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [_parse(l) for l in out.stdout.splitlines()]
    assert [(p["nx"], p["ny"], p["nz"]) for p in got] == grids
    return got


def plan(grid):
    return plans([grid])[0]


def constants():
    out = subprocess.run([dumper(), "consts"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return _parse(out.stdout)


def cell(p):
    """The plan cell a grid lands in — what selects the kernels and how they loop: (z sweep variant: 1 .. 8 chunks in
    scalar masks or "lds", z sweep strided, esdf_rows_kernel runs, voxels per lane of the y sweep, of the x sweep, slab
    tables possible)."""
    return ("lds" if p["z_lds"] else p["z_chunks"], bool(p["z_strided"]), bool(p["rows_kernel"]), p["y_vox"], p["x_vox"],
            bool(p["slab_tables"]))
