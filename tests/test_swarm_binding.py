"""The surface of include/gtop_swarm.h without a GPU: every symbol the header declares is exported and bound, the
binding's table and structures are the header's, the entry points refuse a null context, gtop_swarm_workspace_bytes is a
pure function, and gtop.h and the five other companion headers are untouched.  (What the options refuse on a live
context: tests/test_gpu_swarm.py — a context needs a device.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_swarm_workspace_bytes", "gtop_swarm_gradient_device", "gtop_swarm_gradient_batch",
         "gtop_optimize_swarm_device", "gtop_optimize_swarm")
ERR_INVALID = 1


def header_body():
    text = open(os.path.join(ROOT, "include", "gtop_swarm.h")).read()
    return text[text.index("#ifndef GTOP_SWARM_H_"):]


def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import swarm as gs
    L = gs.swarm_library()
    assert L.gtop_swarm_abi_version() == 1 == gs.SWARM_ABI_VERSION == gtop.SWARM_ABI_VERSION == gs.swarm_abi_version()
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_swarm_abi_version"} <= exported
    assert not [n for n in exported if "swarm" in n and n.startswith("gtop_group")]   # the groups do not forward
    for name in ("SWARM_ABI_VERSION", "SWARM_ENTRY_POINTS", "GtopSwarmOpts", "GtopSwarmStop", "swarm_workspace_bytes",
                 "swarm_gradient_device", "swarm_gradient_batch", "optimize_swarm_device", "optimize_swarm",
                 "swarm_library", "swarm_abi_version", "swarm"):
        assert hasattr(gtop, name) and name in gtop.__all__, name


def struct_fields(body, name):
    start = body.rindex("typedef struct {", 0, body.index(f"}} {name};"))
    struct = re.sub(r"/\*.*?\*/", "", body[start:body.index(f"}} {name};")], flags=re.S)
    fields = []
    for ctype, names in re.findall(r"^\s*(int32_t|double) ([\w, \[\]]+);", struct, flags=re.M):
        for n in names.split(","):
            n = n.strip()
            t = {"int32_t": C.c_int32, "double": C.c_double}[ctype]
            k = re.fullmatch(r"(\w+)\[(\d+)\]", n)
            fields.append((k.group(1), t * int(k.group(2))) if k else (n, t))
    return fields


def test_binding_table_covers_the_header(gtop):
    from grad_traj_optimization_amd import swarm as gs
    body = header_body()
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gs.SWARM_ENTRY_POINTS) == set(NAMES) | {"gtop_swarm_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gs.SWARM_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # the structures as the header lays them out
    assert gs.GtopSwarmOpts._fields_ == struct_fields(body, "gtop_swarm_opts") and len(gs.GtopSwarmOpts._fields_) == 7
    assert gs.GtopSwarmStop._fields_ == struct_fields(body, "gtop_swarm_stop") and len(gs.GtopSwarmStop._fields_) == 3
    assert C.sizeof(gs.GtopSwarmOpts) == 48 and C.sizeof(gs.GtopSwarmStop) == 16
    assert re.search(r"^#define GTOP_SWARM_ABI_VERSION 1\b", body, flags=re.M)
    o, s = gs.GtopSwarmOpts(), gs.GtopSwarmStop()
    assert list(o.reserved) == [0, 0] == list(s.reserved) and o.w >= 0 and o.radius > 0 and o.dt > 0
    assert 1 <= o.n_samples <= gs.SEP_MAX_SAMPLES and s.sweeps >= 1 and s.evals_per_sweep >= 1
    # the header states the arithmetic the twin follows
    text = open(os.path.join(ROOT, "include", "gtop_swarm.h")).read()
    for line in ("e  = R2 - d2", "ACTIVE iff e > 0", "h_v0 = (((G_1 + (-6 / T2) G_3) + (8 / T3) G_4) + (-3 / T4) G_5)",
                 "K = ((-6 w) dt)", "produces the same bits"):
        assert line in text, line


def test_entry_points_refuse_a_null_context(gtop):
    from grad_traj_optimization_amd import swarm as gs
    L = gs.swarm_library()
    o, s = gs.GtopSwarmOpts(n_samples=4), gs.GtopSwarmStop()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    dp = C.cast(buf, C.POINTER(C.c_double))
    assert L.gtop_swarm_gradient_device(None, C.byref(o), 1, 2, p, None, p, 2, p, p, None, p, 1 << 20, None) == ERR_INVALID
    assert L.gtop_swarm_gradient_batch(None, C.byref(o), 1, dp, None, dp, dp, None) == ERR_INVALID
    assert L.gtop_optimize_swarm_device(None, C.byref(o), C.byref(s), 1, 2, p, p, p, 2, p, p, p, None, p, 1 << 20,
                                        None) == ERR_INVALID
    assert L.gtop_optimize_swarm(None, C.byref(o), C.byref(s), 1, dp, dp, dp, dp, None) == ERR_INVALID
    assert all(v == 0.0 for v in buf)


def test_workspace_bytes_is_a_pure_function(gtop):
    from grad_traj_optimization_amd import swarm as gs
    wb = gs.swarm_workspace_bytes
    assert wb(0, 2, 1) == 0 == wb(0, 227, 65536)
    assert wb(1, 2, 1) > 0 and wb(1, 2, 1) == wb(1, 2, 1)
    # monotone in each argument, and room for what the header names: two position sets, four sums per sample and row,
    # the coefficient scratch
    for B, m, n in ((1, 2, 1), (64, 6, 256), (65, 7, 257), (4096, 227, 65536)):
        assert wb(B, m, n) >= 8 * (10 * B * n + 18 * B * m)
    last = 0
    for B in (1, 2, 63, 64, 65, 130, 1024, 4096):
        assert wb(B, 6, 256) >= last
        last = wb(B, 6, 256)
    assert [wb(65, 6, n) for n in (1, 7, 8, 9, 64, 257)] == sorted(wb(65, 6, n) for n in (1, 7, 8, 9, 64, 257))
    assert [wb(65, m, 64) for m in (2, 3, 6, 7, 227)] == sorted(wb(65, m, 64) for m in (2, 3, 6, 7, 227))
    L = gs.swarm_library()
    n = C.c_size_t(12345)
    for B, m, ns in ((-1, 6, 8), (4097, 6, 8), (1, 1, 8), (1, 228, 8), (1, 6, 0), (1, 6, 65537)):
        assert L.gtop_swarm_workspace_bytes(B, m, ns, C.byref(n)) == ERR_INVALID and n.value == 12345
        with pytest.raises(ValueError):
            wb(B, m, ns)
    assert L.gtop_swarm_workspace_bytes(1, 6, 8, None) == ERR_INVALID


def test_the_other_headers_are_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert not [n for n in _abi.ENTRY_POINTS if "swarm" in n]
    for other in ("gtop.h", "gtop_kinematics.h", "gtop_separation.h", "gtop_separation_certificate.h",
                  "gtop_prediction.h", "gtop_time.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "gtop_swarm" not in text and "GTOP_SWARM" not in text, other
    from grad_traj_optimization_amd import kinematics, prediction, separation, separation_certificate, timeopt
    assert (kinematics.KIN_ABI_VERSION, separation.SEP_ABI_VERSION, separation_certificate.SEPCERT_ABI_VERSION,
            prediction.PRED_ABI_VERSION, timeopt.TIME_ABI_VERSION) == (1, 1, 1, 1, 1)
