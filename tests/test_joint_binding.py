"""The surface of include/gtop_joint.h without a GPU: every symbol the header declares is exported and bound, the
binding's table and structure are the header's, the workspace size is monotone and refuses bad shapes, the entry points
refuse a null context, and gtop.h and the seven other companion headers are untouched.  (What the options structure
refuses on a live context: tests/test_gpu_joint.py — a context needs a device.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import joint_twin as jt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_joint_gradient_device", "gtop_joint_gradient_batch", "gtop_joint_workspace_bytes",
         "gtop_optimize_joint_device", "gtop_optimize_joint")
ERR_INVALID = 1


def header_body():
    text = open(os.path.join(ROOT, "include", "gtop_joint.h")).read()
    return text[text.index("#ifndef GTOP_JOINT_H_"):]


def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import joint as gj
    L = gj.joint_library()
    assert L.gtop_joint_abi_version() == 1 == gj.JOINT_ABI_VERSION == gtop.JOINT_ABI_VERSION == gj.joint_abi_version()
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_joint_abi_version"} <= exported
    for name in ("joint_gradient_device", "joint_gradient_batch", "optimize_joint_device", "optimize_joint",
                 "joint_workspace_bytes", "GtopJointOpt", "JOINT_INFO", "JOINT_ENTRY_POINTS", "joint_abi_version",
                 "joint_library", "joint"):
        assert hasattr(gtop, name) and name in gtop.__all__, name
    assert len(gj.JOINT_INFO) == 8 == jt.INFO


def test_binding_table_covers_the_header(gtop):
    from grad_traj_optimization_amd import joint as gj
    body = header_body()
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gj.JOINT_ENTRY_POINTS) == set(NAMES) | {"gtop_joint_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gj.JOINT_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # the structure as the header lays it out: five doubles, two 32-bit words
    struct = body[body.index("typedef struct {"):body.index("} gtop_jointopt;")]
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"^\s*(int32_t|double) ([\w, ]+);", struct, flags=re.M):
        fields += [(n.strip(), {"int32_t": C.c_int32, "double": C.c_double}[ctype]) for n in names.split(",")]
    assert gj.GtopJointOpt._fields_ == fields and len(fields) == 7
    assert C.sizeof(gj.GtopJointOpt) == 48
    for macro, value in (("GTOP_JOINT_ABI_VERSION", 1), ("GTOP_JOINT_INFO", 8)):
        assert re.search(rf"^#define {macro} {value}\b", body, flags=re.M), macro
    o = gj.GtopJointOpt()
    assert o.reserved == 0 and o.max_evals >= 1 and 0.0301 <= o.t_min <= o.t_max and o.rho >= 0
    # the header states the table the twin follows, and says what it does not differentiate
    text = open(os.path.join(ROOT, "include", "gtop_joint.h")).read()
    assert "c4    15/T^4     8/T^3     3/(2T^2)   -15/T^4     7/T^3    -1/T^2" in text and "gtop_set_moving_cost" in text


def test_workspace_bytes_is_monotone_and_refuses_bad_shapes(gtop):
    from grad_traj_optimization_amd import joint as gj
    L = gj.joint_library()
    assert gj.joint_workspace_bytes(0, 2) == 0
    last = 0
    for B in (1, 2, 3, 64, 65, 1024):
        row = [gj.joint_workspace_bytes(B, m) for m in (2, 3, 6, 7, 13, 118, 227)]
        assert all(a < b for a, b in zip(row, row[1:])) and row[0] > last and all(v % 8 == 0 for v in row)
        last = row[0]
        # the six n_z-vectors, the packed bounds, f | g, the scalars and the counters
        for m, v in zip((2, 3, 6, 7, 13, 118, 227), row):
            assert v >= 8 * B * (9 * (10 * m - 9) + 6) + 4 * 5 * B
    n = C.c_size_t(77)
    for B, m in ((-1, 6), (4, 1), (4, 228), (4, 0), (4, -3)):
        assert L.gtop_joint_workspace_bytes(B, m, C.byref(n)) == ERR_INVALID and n.value == 77
        with pytest.raises(ValueError):
            gj.joint_workspace_bytes(B, m)
    assert L.gtop_joint_workspace_bytes(4, 6, None) == ERR_INVALID


def test_entry_points_refuse_a_null_context(gtop):
    from grad_traj_optimization_amd import joint as gj
    L = gj.joint_library()
    o = gj.GtopJointOpt()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    dp = C.cast(buf, C.POINTER(C.c_double))
    assert L.gtop_joint_gradient_device(None, 1, 2, p, p, p, 2, p, p, p, None, None) == ERR_INVALID
    assert L.gtop_joint_gradient_batch(None, 1, dp, dp, dp, dp, None) == ERR_INVALID
    assert L.gtop_optimize_joint_device(None, C.byref(o), 1, 2, p, p, p, 2, p, p, None, p, p, p, 1 << 20, None) == ERR_INVALID
    assert L.gtop_optimize_joint(None, C.byref(o), 1, dp, dp, dp, None, dp, dp) == ERR_INVALID
    assert all(v == 0.0 for v in buf)


def test_the_other_headers_are_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert not [n for n in _abi.ENTRY_POINTS if "joint" in n]
    for other in ("gtop.h", "gtop_kinematics.h", "gtop_separation.h", "gtop_separation_certificate.h", "gtop_prediction.h",
                  "gtop_time.h", "gtop_time_moving.h", "gtop_swarm.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "gtop_joint" not in text and "GTOP_JOINT" not in text and "gtop_optimize_joint" not in text, other
    from grad_traj_optimization_amd import (kinematics, prediction, separation, separation_certificate, swarm, timeopt,
                                            timeopt_moving)
    assert (kinematics.KIN_ABI_VERSION, separation.SEP_ABI_VERSION, separation_certificate.SEPCERT_ABI_VERSION,
            prediction.PRED_ABI_VERSION, timeopt.TIME_ABI_VERSION, timeopt_moving.TIME_MOVING_ABI_VERSION,
            swarm.SWARM_ABI_VERSION) == (1, 1, 1, 1, 1, 1, 1)
