"""The surface of include/gtop_time.h without a GPU: every symbol the header declares is exported and bound, the
binding's table and structure are the header's, the entry points refuse a null context, and gtop.h and the four other
companion headers are untouched.  (What the options structure refuses on a live context: tests/test_gpu_time.py — a
context needs a device.)"""
import ctypes as C
import os
import re
import subprocess

from tests import time_twin as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_time_gradient_device", "gtop_time_gradient_batch", "gtop_optimize_times_device", "gtop_optimize_times")
ERR_INVALID = 1


def header_body():
    text = open(os.path.join(ROOT, "include", "gtop_time.h")).read()
    return text[text.index("#ifndef GTOP_TIME_H_"):]


def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import timeopt as gt
    L = gt.time_library()
    assert L.gtop_time_abi_version() == 1 == gt.TIME_ABI_VERSION == gtop.TIME_ABI_VERSION == gt.time_abi_version()
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_time_abi_version"} <= exported
    for name in ("time_gradient_device", "time_gradient_batch", "optimize_times_device", "optimize_times", "GtopTimeOpt",
                 "TIMEOPT_INFO", "TIME_PARTS", "TIME_ENTRY_POINTS", "time_abi_version", "time_library", "timeopt"):
        assert hasattr(gtop, name) and name in gtop.__all__, name
    assert len(gt.TIMEOPT_INFO) == 8 == tt.INFO and len(gt.TIME_PARTS) == 4 == tt.PARTS
    assert (gt.FTOL_REACHED, gt.XTOL_REACHED, gt.MAXEVAL_REACHED) == (tt.FTOL, tt.XTOL, tt.MAXEVAL) == (3, 4, 5)


def test_binding_table_covers_the_header(gtop):
    from grad_traj_optimization_amd import timeopt as gt
    body = header_body()
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gt.TIME_ENTRY_POINTS) == set(NAMES) | {"gtop_time_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gt.TIME_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # the structure as the header lays it out: six doubles, two 32-bit words
    struct = body[body.index("typedef struct {"):body.index("} gtop_timeopt;")]
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"^\s*(int32_t|double) ([\w, ]+);", struct, flags=re.M):
        fields += [(n.strip(), {"int32_t": C.c_int32, "double": C.c_double}[ctype]) for n in names.split(",")]
    assert gt.GtopTimeOpt._fields_ == fields and len(fields) == 8
    assert C.sizeof(gt.GtopTimeOpt) == 56
    for macro, value in (("GTOP_TIME_ABI_VERSION", 1), ("GTOP_TIME_PARTS", 4), ("GTOP_TIMEOPT_INFO", 8)):
        assert re.search(rf"^#define {macro} {value}\b", body, flags=re.M), macro
    o = gt.GtopTimeOpt()
    assert o.reserved == 0 and o.max_evals >= 1 and 0.0301 <= o.t_min <= o.t_max and o.first_move > 0 and o.rho >= 0
    # the header states the rule the twin follows, and says what it does not differentiate
    text = open(os.path.join(ROOT, "include", "gtop_time.h")).read()
    assert "accept if F' <= F + 1e-4 sum_s g_s (T'_s - T_s)" in text and "gtop_set_moving_cost" in text


def test_entry_points_refuse_a_null_context(gtop):
    from grad_traj_optimization_amd import timeopt as gt
    L = gt.time_library()
    o = gt.GtopTimeOpt()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    dp = C.cast(buf, C.POINTER(C.c_double))
    assert L.gtop_time_gradient_device(None, 1, 2, p, p, p, 2, p, p, None, None) == ERR_INVALID
    assert L.gtop_time_gradient_batch(None, 1, dp, dp, dp, None) == ERR_INVALID
    assert L.gtop_optimize_times_device(None, C.byref(o), 1, 2, p, p, p, 2, None, p, p, None) == ERR_INVALID
    assert L.gtop_optimize_times(None, C.byref(o), 1, dp, None, dp, dp) == ERR_INVALID
    assert all(v == 0.0 for v in buf)


def test_the_other_headers_are_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert not [n for n in _abi.ENTRY_POINTS if "time_gradient" in n or "optimize_times" in n]
    for other in ("gtop.h", "gtop_kinematics.h", "gtop_separation.h", "gtop_separation_certificate.h",
                  "gtop_prediction.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "gtop_time" not in text and "GTOP_TIME" not in text and "gtop_optimize_times" not in text, other
    from grad_traj_optimization_amd import kinematics, prediction, separation, separation_certificate
    assert (kinematics.KIN_ABI_VERSION, separation.SEP_ABI_VERSION, separation_certificate.SEPCERT_ABI_VERSION,
            prediction.PRED_ABI_VERSION) == (1, 1, 1, 1)
