"""The continuous-time kinematic certificate (include/gtop_kinematics.h: gtop_certify_kinematics_device,
gtop_certify_kinematics_batch, gtop_select_best_kin_certified_device) over a GtopContext.

The sampled reports (GtopContext.validate_device, validate_segments_device) give the maxima of the velocity and the
acceleration over the getTraj samples; the certificate bounds ‖v‖, ‖a‖, max|v_k| and max|a_k| over whole time
intervals, so "WITHIN" speaks about every time of the curve.  Its per-segment rows carry the certified upper bounds in
the columns GtopContext.reallocate_times_device(LIMITS) reads: passed as its seg_report, the segments are stretched by
certified figures.

The companion header has its own table and its own version, apart from _abi.ENTRY_POINTS and ABI_VERSION (which speak
of include/gtop.h alone): the table is bound onto load_library()'s handle at first use.

Functions of a context, not methods of it: the device forms are built on the context's own argument helpers
(GtopContext._trajectory, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import GtopLimits, library_path, load_library
from ._lib import _f64, _p, _stream, _th
from .certify import CERT_REPORT, REQUIRE_NOT_UNSAFE, REQUIRE_SAFE

# the columns of a certificate row and of a per-segment row (GTOP_KIN_REPORT, GTOP_KIN_SEG)
KIN_REPORT = ("verdict", "ub_v", "lo_v", "lo_v_t", "ub_a", "lo_a", "lo_a_t", "first_violation_t", "n_undecided",
              "n_refinements", "time_sum")
KIN_SEG = ("verdict", "n_refinements", "lo_vel_norm", "lo_acc_norm", "lo_vel_axis", "lo_acc_axis", "ub_vel_norm",
           "ub_acc_norm", "ub_vel_axis", "ub_acc_axis")
EXCEEDS, UNDECIDED, WITHIN = -1, 0, 1
# the version of include/gtop_kinematics.h this module speaks: gtop_kin_abi_version() of the in-tree build
KIN_ABI_VERSION = 1


class GtopKinOpts(C.Structure):
    """gtop_kin_opts of include/gtop_kinematics.h: the limits (<= 0 or NaN: off), whether they apply to the norms or
    (per_axis) to the largest |component|, the levels of refinement below a segment's 64 intervals (0 .. 3), the
    refinements a trajectory may spend, and a reserved word that must be 0."""
    _fields_ = [("max_vel", C.c_double), ("max_acc", C.c_double), ("per_axis", C.c_int32), ("max_depth", C.c_int32),
                ("max_refine", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, max_vel=0.0, max_acc=0.0, per_axis=False, max_depth=2, max_refine=256, reserved=0):
        super().__init__(float(max_vel), float(max_acc), int(bool(per_axis)), int(max_depth), int(max_refine),
                         int(reserved))


_i, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
_kin, _limits = C.POINTER(GtopKinOpts), C.POINTER(GtopLimits)
# Every entry point of include/gtop_kinematics.h: name -> (the header version that introduced it; restype; argtypes)
KIN_ENTRY_POINTS = {
    "gtop_kin_abi_version": (1, _i, []),
    "gtop_certify_kinematics_device": (1, _i, [_vp, _i, _i, _vp, _vp, _i, _kin, _vp, _vp, _vp]),
    "gtop_certify_kinematics_batch": (1, _i, [_vp, _i, _dp, _kin, _dp, _dp]),
    "gtop_select_best_kin_certified_device": (1, _i, [_vp, _i, _vp, _vp, _vp, _vp, _limits, _i, _vp, _vp, _vp]),
}

_bound = None


def kin_library():
    """load_library()'s handle with KIN_ENTRY_POINTS bound onto it.  Raises where the library has no kinematic
    certificate: an older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_kin_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_kin_abi_version: it was built before include/gtop_kinematics.h "
                          "and has no kinematic certificate (GTOP_HIP_LIB names an older build?)")
    L.gtop_kin_abi_version.restype = C.c_int
    have = L.gtop_kin_abi_version()
    for name, (since, restype, argtypes) in KIN_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def certify_kinematics_device(ctx, coeff, T, opts, kin=None, seg=None, want_seg=True, stream=None):
    """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> (kin (B, 11), seg (B, m, 10) or None), the
    columns of KIN_REPORT and KIN_SEG; asynchronous, capturable (pass `kin` / `seg` to write into buffers of the
    caller's; want_seg False and no `seg`: the per-segment rows are not formed).  opts: a GtopKinOpts."""
    L = kin_library()
    traj = ctx._trajectory(coeff, T)
    kin, pkin = ctx._out("kin", kin, (traj[0], len(KIN_REPORT)), coeff)
    pseg = None
    if seg is not None or want_seg:
        seg, pseg = ctx._out("seg", seg, (*traj[:2], len(KIN_SEG)), coeff)
    ctx._chk(L.gtop_certify_kinematics_device(ctx._h, *traj, C.byref(opts), pkin, pseg, _stream(stream, coeff)))
    return kin, seg


def select_best_kin_certified_device(ctx, report, cert, kin, cost, limits, require=REQUIRE_SAFE, want_pass=True,
                                     best=None, stream=None):
    """report (B, 12), cert (B, 8) or None, kin (B, 11), cost (B,) torch fp64 CUDA tensors -> (pass (B,) uint8 or None,
    best (2,) int32): select_best_certified_device's rule (cert None: GtopContext.select_best_device's), and the row's
    kinematic verdict must be WITHIN (REQUIRE_SAFE) or must not be EXCEEDS (REQUIRE_NOT_UNSAFE); asynchronous,
    capturable."""
    L = kin_library()
    B = cost.numel()
    preport = ctx._dev("report", report, B * len(ctx.TRAJ_REPORT))
    pcert = None if cert is None else ctx._dev("cert", cert, B * len(CERT_REPORT))
    pkin, pcost = ctx._dev("kin", kin, B * len(KIN_REPORT)), ctx._dev("cost", cost, B)
    ok, pok = ctx._out("pass", None, (B,), report, _th().uint8) if want_pass else (None, None)
    best, pbest = ctx._out("best", best, (2,), report, _th().int32)
    ctx._chk(L.gtop_select_best_kin_certified_device(ctx._h, B, preport, pcert, pkin, pcost, C.byref(limits),
                                                     int(require), pok, pbest, _stream(stream, report)))
    return ok, best


def certify_kinematics_batch(ctx, x, opts, want_seg=True):
    """(kin (B, 11), seg (B, m, 10) or None) of the first B rows of the context's problem at free variables x (B, n),
    host arrays."""
    L = kin_library()
    x = _f64(x)
    B = x.shape[0]
    kin = np.empty((B, len(KIN_REPORT)))
    seg = np.empty((B, getattr(ctx, "m", 0), len(KIN_SEG))) if want_seg else None   # (no problem: the library refuses)
    ctx._chk(L.gtop_certify_kinematics_batch(ctx._h, B, _p(x), C.byref(opts), _p(kin), None if seg is None else _p(seg)))
    return kin, seg


__all__ = ["KIN_REPORT", "KIN_SEG", "EXCEEDS", "UNDECIDED", "WITHIN", "REQUIRE_SAFE", "REQUIRE_NOT_UNSAFE",
           "KIN_ENTRY_POINTS", "KIN_ABI_VERSION", "GtopKinOpts", "kin_library", "certify_kinematics_device",
           "certify_kinematics_batch", "select_best_kin_certified_device"]
