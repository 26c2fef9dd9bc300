"""The surface of include/gtop_prediction.h without a GPU: every symbol the header declares is exported and bound, the
binding's table and structure are the header's, the host entry refuses what the header says it refuses and leaves
unfitted rows alone, and gtop.h is untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import predict_twin as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_fit_predictions_device", "gtop_refresh_box_predictions_device", "gtop_fit_predictions")
ERR_INVALID = 1


def header_body():
    text = open(os.path.join(ROOT, "include", "gtop_prediction.h")).read()
    return text[text.index("#ifndef GTOP_PREDICTION_H_"):]


def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import prediction as gp
    L = gp.pred_library()
    assert L.gtop_pred_abi_version() == 1 == gp.PRED_ABI_VERSION == gtop.PRED_ABI_VERSION == gp.pred_abi_version()
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_pred_abi_version"} <= exported
    for name in ("GtopPredictOpts", "PRED_INFO", "PRED_ABI_VERSION", "PRED_ENTRY_POINTS", "fit_predictions_device",
                 "fit_predictions", "refresh_box_predictions_device", "pred_abi_version", "prediction"):
        assert hasattr(gtop, name) and name in gtop.__all__, name
    assert len(gp.PRED_INFO) == 12 == pt.INFO and gp.PRED_LOCAL == 20 == pt.LOCAL


def test_binding_table_covers_the_header(gtop):
    from grad_traj_optimization_amd import prediction as gp
    body = header_body()
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gp.PRED_ENTRY_POINTS) == set(NAMES) | {"gtop_pred_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gp.PRED_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # the structure as the header lays it out: two 32-bit words, three doubles, two 32-bit words
    struct = body[body.index("typedef struct {"):body.index("} gtop_predict_opts;")]
    fields = re.findall(r"^\s*(int32_t|double) (\w+);", struct, flags=re.M)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n.rstrip("_"), c) for n, c in gp.GtopPredictOpts._fields_] == [(n, ctype[c]) for c, n in fields]
    assert C.sizeof(gp.GtopPredictOpts) == 40
    for macro, value in (("GTOP_PRED_ABI_VERSION", 1), ("GTOP_PREDICT_POLYFIT", 0), ("GTOP_PREDICT_CONST_VEL", 1),
                         ("GTOP_PRED_INFO", 12), ("GTOP_PRED_LOCAL", 20), ("GTOP_PRED_OK", 0), ("GTOP_PRED_LOWERED", 1),
                         ("GTOP_PRED_EMPTY", 2), ("GTOP_PRED_BAD", 3)):
        assert re.search(rf"^#define {macro} {value}\b", body, flags=re.M), macro
    assert (gp.PREDICT_POLYFIT, gp.PREDICT_CONST_VEL) == (pt.POLYFIT, pt.CONST_VEL) == (0, 1)
    assert (gp.PRED_OK, gp.PRED_LOWERED, gp.PRED_EMPTY, gp.PRED_BAD) == (pt.OK, pt.LOWERED, pt.EMPTY, pt.BAD)
    o = gp.GtopPredictOpts()                                # the reference's defaults
    assert (o.mode, o.degree, o.lambda_, o.horizon, o.inflate, o.regularise_horizon, o.reserved) == (0, 5, 1.0, 0.0, 0.0, 0, 0)


def test_host_entry_refusals(gtop):
    from grad_traj_optimization_amd import prediction as gp
    hist, count, head = pt.make_batch(3, 7)
    for bad in (dict(mode=2), dict(mode=-1), dict(degree=0), dict(degree=6), dict(lambda_=-1.0), dict(lambda_=np.nan),
                dict(lambda_=np.inf), dict(horizon=-0.5), dict(horizon=np.nan), dict(inflate=-1.0), dict(inflate=np.inf),
                dict(inflate=np.nan), dict(regularise_horizon=2), dict(regularise_horizon=1, horizon=np.inf), dict(reserved=1)):
        with pytest.raises(gtop.GtopError) as e:
            gp.fit_predictions(hist, count, gp.GtopPredictOpts(**bad), head=head)
        assert e.value.code == ERR_INVALID, bad
    gp.fit_predictions(hist, count, gp.GtopPredictOpts(horizon=np.inf), head=head)          # allowed
    gp.fit_predictions(hist, count, gp.GtopPredictOpts(lambda_=0.0, degree=1), head=head)
    L = gp.pred_library()
    o = gp.GtopPredictOpts()
    out = [np.zeros((3, 18)), np.zeros((3, 2)), np.zeros((3, 12))]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h, c = hist.ctypes.data_as(dp), count.ctypes.data_as(ip)
    po = [a.ctypes.data_as(dp) for a in out]
    assert L.gtop_fit_predictions(3, 7, h, c, None, C.byref(o), *po, None) == 0
    assert L.gtop_fit_predictions(3, 7, h, c, None, None, *po, None) == ERR_INVALID
    assert L.gtop_fit_predictions(-1, 7, h, c, None, C.byref(o), *po, None) == ERR_INVALID
    assert L.gtop_fit_predictions(3, 0, h, c, None, C.byref(o), *po, None) == ERR_INVALID
    assert L.gtop_fit_predictions(3, 7, None, c, None, C.byref(o), *po, None) == ERR_INVALID
    assert L.gtop_fit_predictions(3, 7, h, None, None, C.byref(o), *po, None) == ERR_INVALID
    for missing in range(3):
        args = list(po)
        args[missing] = None
        assert L.gtop_fit_predictions(3, 7, h, c, None, C.byref(o), *args, None) == ERR_INVALID
    assert L.gtop_fit_predictions(0, 7, None, None, None, C.byref(o), None, None, None, None) == 0
    with pytest.raises(ValueError):
        gp.fit_predictions(hist[:, :, :3], count, o)
    with pytest.raises(ValueError):
        gp.fit_predictions(hist, count[:2], o)
    with pytest.raises(ValueError):
        gp.fit_predictions(hist, count, o, head=head[:2])


def test_unfitted_rows_are_left_alone(gtop):
    """EMPTY and BAD write the info row only: status, count, zeros."""
    from grad_traj_optimization_amd import prediction as gp
    hist, count, head = pt.make_batch(12, 7)
    coef, t_range, info, local = gp.fit_predictions(hist, count, gp.GtopPredictOpts(), head=head, fill=-3.5)
    status = info[:, 0]
    assert set(status.astype(int)) == {pt.OK, pt.LOWERED, pt.EMPTY, pt.BAD}
    left = status >= pt.EMPTY
    assert np.all(coef[left] == -3.5) and np.all(t_range[left] == -3.5) and np.all(local[left] == -3.5)
    assert np.all(info[left, 2:] == 0.0) and np.all(info[:, 10:] == 0.0)
    assert not np.any(coef[~left] == -3.5) and np.all(np.isfinite(coef[~left]))
    kinds = dict(zip(pt.KINDS, range(12)))
    assert status[kinds["empty"]] == pt.EMPTY and info[kinds["empty"], 1] == 0
    for kind in ("nan", "flat", "over", "negative", "inf_time"):
        assert status[kinds[kind]] == pt.BAD, kind
    assert info[kinds["over"], 1] == 7 and info[kinds["negative"], 1] == 0           # the count, clamped
    none = gp.fit_predictions(hist, count, gp.GtopPredictOpts(), head=head, want_local=False)
    assert none[3] is None and np.array_equal(none[2], info)


def test_the_surface_of_gtop_h_is_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert not [n for n in _abi.ENTRY_POINTS if "pred_" in n or "predictions" in n]
    text = open(os.path.join(ROOT, "include", "gtop.h")).read()
    assert "gtop_pred" not in text and "GTOP_PRED" not in text and "gtop_fit_predictions" not in text
    for other in ("gtop_kinematics.h", "gtop_separation.h", "gtop_separation_certificate.h"):
        assert "gtop_pred" not in open(os.path.join(ROOT, "include", other)).read()
