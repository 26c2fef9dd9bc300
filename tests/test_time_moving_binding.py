"""The surface of include/gtop_time_moving.h without a GPU: every symbol the header declares is exported and bound,
the binding's table is the header's, GTOP_TIME_MOVING_PARTS is 6, the entry points refuse a null context, and gtop.h,
the six other companion headers — gtop_time.h with its four entry points and its words about gtop_set_moving_cost
among them — are untouched."""
import ctypes as C
import os
import re
import subprocess

from tests import time_moving_twin as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_time_gradient_moving_device", "gtop_time_gradient_moving_batch", "gtop_optimize_times_moving_device",
         "gtop_optimize_times_moving")
TIME_NAMES = ("gtop_time_gradient_device", "gtop_time_gradient_batch", "gtop_optimize_times_device", "gtop_optimize_times")
ERR_INVALID = 1


def header_body():
    text = open(os.path.join(ROOT, "include", "gtop_time_moving.h")).read()
    return text[text.index("#ifndef GTOP_TIME_MOVING_H_"):]


def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import timeopt_moving as gm
    L = gm.time_moving_library()
    assert (L.gtop_time_moving_abi_version() == 1 == gm.TIME_MOVING_ABI_VERSION == gtop.TIME_MOVING_ABI_VERSION
            == gm.time_moving_abi_version())
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_time_moving_abi_version"} <= exported
    for name in ("time_gradient_moving_device", "time_gradient_moving_batch", "optimize_times_moving_device",
                 "optimize_times_moving", "TIME_MOVING_PARTS", "TIME_MOVING_ENTRY_POINTS", "time_moving_abi_version",
                 "time_moving_library", "timeopt_moving"):
        assert hasattr(gtop, name) and name in gtop.__all__, name
    assert len(gm.TIME_MOVING_PARTS) == 6 == tm.PARTS
    assert gm.TIME_MOVING_PARTS[:4] == gtop.TIME_PARTS and tm.INFO == len(gtop.TIMEOPT_INFO)


def test_binding_table_covers_the_header(gtop):
    from grad_traj_optimization_amd import timeopt as gt
    from grad_traj_optimization_amd import timeopt_moving as gm
    body = header_body()
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gm.TIME_MOVING_ENTRY_POINTS) == set(NAMES) | {"gtop_time_moving_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gm.TIME_MOVING_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # a table of its own, apart from gtop.h's and gtop_time.h's
    assert not set(gm.TIME_MOVING_ENTRY_POINTS) & set(gt.TIME_ENTRY_POINTS)
    for macro, value in (("GTOP_TIME_MOVING_ABI_VERSION", 1), ("GTOP_TIME_MOVING_PARTS", 6)):
        assert re.search(rf"^#define {macro} {value}\b", body, flags=re.M), macro
    # gtop_timeopt is reused, not restated; the header states the derivative and the sums the twin follows
    assert '#include "gtop_time.h"' in body and "typedef struct" not in body
    text = open(os.path.join(ROOT, "include", "gtop_time_moving.h")).read()
    for words in ("R_{m-1} = 0, R_s = R_{s+1} + q_{s+1}", "gT[b][s] = ([2] + [3]) + [5]", "gt0[b] = R_0 + q_0",
                  "pt < bmin: +c'_k", "pt > bmax: -c'_k", "the static value wins a tie"):
        assert words in text, words


def test_entry_points_refuse_a_null_context(gtop):
    from grad_traj_optimization_amd import timeopt_moving as gm
    L = gm.time_moving_library()
    o = gtop.GtopTimeOpt()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    dp = C.cast(buf, C.POINTER(C.c_double))
    assert L.gtop_time_gradient_moving_device(None, 1, 2, p, p, p, 2, p, p, None, None, None) == ERR_INVALID
    assert L.gtop_time_gradient_moving_batch(None, 1, dp, dp, dp, None, None) == ERR_INVALID
    assert L.gtop_optimize_times_moving_device(None, C.byref(o), 1, 2, p, p, p, 2, None, p, p, None) == ERR_INVALID
    assert L.gtop_optimize_times_moving(None, C.byref(o), 1, dp, None, dp, dp) == ERR_INVALID
    assert all(v == 0.0 for v in buf)


def test_the_other_headers_are_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    from grad_traj_optimization_amd import timeopt as gt
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert not [n for n in _abi.ENTRY_POINTS if "time_gradient" in n or "optimize_times" in n]
    for other in ("gtop.h", "gtop_kinematics.h", "gtop_separation.h", "gtop_separation_certificate.h",
                  "gtop_prediction.h", "gtop_time.h", "gtop_swarm.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "time_moving" not in text and "TIME_MOVING" not in text and "gt0" not in text, other
    # gtop_time.h: its four entry points, its version, and what it says about the moving-obstacle cost
    text = open(os.path.join(ROOT, "include", "gtop_time.h")).read()
    body = text[text.index("#ifndef GTOP_TIME_H_"):]
    assert set(re.findall(r"^int (gtop_\w+)\(", body, flags=re.M)) == set(TIME_NAMES) | {"gtop_time_abi_version"}
    assert set(gt.TIME_ENTRY_POINTS) == set(TIME_NAMES) | {"gtop_time_abi_version"} and gt.time_abi_version() == 1
    assert ("While\n * gtop_set_moving_cost is switched on every entry point of this header returns\n * GTOP_ERR_STATE and "
            "launches nothing.") in text
    from grad_traj_optimization_amd import kinematics, prediction, separation, separation_certificate, swarm
    assert (kinematics.KIN_ABI_VERSION, separation.SEP_ABI_VERSION, separation_certificate.SEPCERT_ABI_VERSION,
            prediction.PRED_ABI_VERSION, gt.TIME_ABI_VERSION, swarm.SWARM_ABI_VERSION) == (1, 1, 1, 1, 1, 1)


def test_the_new_kernels_use_no_scratch_memory(tmp_path):
    """The build-time check of tests/test_consistent_gradient.py on csrc/gtop_time_moving.hip and on the static
    kernels that share its pass (csrc/gtop_time_pass.h): no kernel uses scratch memory or spills a vector register."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    for source, kernels in (("gtop_time_moving.hip", 5), ("gtop_time.hip", 2)):
        rows, _ = kr.analyse(asm_out=str(tmp_path / (source + ".s")), source=source)
        assert len(rows) == kernels, [r["kernel"] for r in rows]
        bad = [r for r in rows if r["scratch"] or r["vgpr_spill"]]
        assert not bad, bad
