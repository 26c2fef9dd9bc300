"""Waypoint derivatives and segment times together (include/gtop_joint.h: gtop_joint_gradient_device,
gtop_joint_gradient_batch, gtop_optimize_joint_device, gtop_optimize_joint, gtop_joint_workspace_bytes) over a
GtopContext.

joint_gradient_device returns the cost, its derivative with respect to every free waypoint value (gx) and with respect
to every segment time (gT) from ONE pass over the trajectory: cost, gT and parts carry time_gradient_device's bits, gx is
the consistent gradient without its + 1e-5.  optimize_joint_device minimises cost + rho sum(T) over z = [x | T] inside
lb <= x <= ub and max(t_min, T_lo) <= T <= t_max with the batched MMA loop, max_evals rounds of {joint pass, MMA update}
on the caller's stream, its whole state in a workspace of the caller's: "min-jerk start, joint optimise, report /
certify" stays on the device and can be captured as one graph.  With the moving-obstacle cost on these entry points
refuse; alternate optimize_device_ex and optimize_times_moving_device there.

The companion header has its own table and its own version, apart from _abi.ENTRY_POINTS and ABI_VERSION (which speak
of include/gtop.h alone): the table is bound onto load_library()'s handle at first use.

Functions of a context, not methods of it: the device forms are built on the context's own argument helpers
(GtopContext._problem, _bounded_problem, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import library_path, load_library
from ._lib import _f64, _p, _stream
from .timeopt import TIME_PARTS

# the columns of an info row (GTOP_JOINT_INFO)
JOINT_INFO = ("code", "evals", "F_start", "F", "cost", "time_sum", "free_gradient_x", "free_gradient_T")
# the version of include/gtop_joint.h this module speaks: gtop_joint_abi_version() of the in-tree build
JOINT_ABI_VERSION = 1


class GtopJointOpt(C.Structure):
    """gtop_jointopt of include/gtop_joint.h: rho >= 0, the weight of sum(T); the bounds 0.0301 <= t_min <= t_max of
    every segment time; the MMA loop's stop rules ftol_rel, xtol_rel (0: off) and max_evals, per row; a reserved word
    that must be 0."""
    _fields_ = [("rho", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double), ("ftol_rel", C.c_double),
                ("xtol_rel", C.c_double), ("max_evals", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, rho=0.0, t_min=0.05, t_max=60.0, ftol_rel=0.0, xtol_rel=0.0, max_evals=40, reserved=0):
        super().__init__(float(rho), float(t_min), float(t_max), float(ftol_rel), float(xtol_rel), int(max_evals),
                         int(reserved))


_i, _vp, _dp, _sz = C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t
_opt = C.POINTER(GtopJointOpt)
# Every entry point of include/gtop_joint.h: name -> (the header version that introduced it; restype; argtypes)
JOINT_ENTRY_POINTS = {
    "gtop_joint_abi_version": (1, _i, []),
    "gtop_joint_gradient_device": (1, _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gtop_joint_gradient_batch": (1, _i, [_vp, _i, _dp, _dp, _dp, _dp, _dp]),
    "gtop_joint_workspace_bytes": (1, _i, [_i, _i, C.POINTER(_sz)]),
    "gtop_optimize_joint_device": (1, _i, [_vp, _opt, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gtop_optimize_joint": (1, _i, [_vp, _opt, _i, _dp, _dp, _dp, _dp, _dp, _dp]),
}

_bound = None


def _th():
    import torch
    return torch


def joint_library():
    """load_library()'s handle with JOINT_ENTRY_POINTS bound onto it.  Raises where the library has no joint pass: an
    older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_joint_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_joint_abi_version: it was built before include/gtop_joint.h "
                          "and has no joint gradient (GTOP_HIP_LIB names an older build?)")
    L.gtop_joint_abi_version.restype = C.c_int
    have = L.gtop_joint_abi_version()
    for name, (since, restype, argtypes) in JOINT_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def joint_abi_version():
    """gtop_joint_abi_version() of the library in use."""
    return joint_library().gtop_joint_abi_version()


def joint_workspace_bytes(B, m):
    """The bytes of workspace optimize_joint_device needs for B rows of m segments (pure: no context, no GPU)."""
    n = _sz(0)
    if joint_library().gtop_joint_workspace_bytes(int(B), int(m), C.byref(n)) != 0:
        raise ValueError(f"joint_workspace_bytes: need B >= 0 and 2 <= m <= 227, got B = {B}, m = {m}")
    return int(n.value)


def joint_gradient_device(ctx, x, Df, T, cost=None, gx=None, gT=None, parts=None, want_parts=False, stream=None):
    """torch fp64 CUDA tensors x (B, 9 (m - 1)), Df (18 B elements), T (B, m) or (m,) -> (cost (B,), gx (B, 9 (m - 1)),
    gT (B, m), parts (B, m, 4) or None): the callback's cost, its derivative with respect to every free waypoint value
    and every segment time, and (given, or want_parts) the columns of TIME_PARTS per segment.  One launch;
    asynchronous, capturable when every output is the caller's."""
    L = joint_library()
    prob = ctx._problem(x, Df, T)
    B, m = prob[:2]
    cost, pcost = ctx._out("cost", cost, (B,), x)
    gx, pgx = ctx._out("gx", gx, (B, 9 * (m - 1)), x)
    gT, pg = ctx._out("gT", gT, (B, m), x)
    pparts = None
    if parts is not None or want_parts:
        parts, pparts = ctx._out("parts", parts, (B, m, len(TIME_PARTS)), x)
    ctx._chk(L.gtop_joint_gradient_device(ctx._h, *prob, pcost, pgx, pg, pparts, _stream(stream, x)))
    return cost, gx, gT, parts


def optimize_joint_device(ctx, opts, x, Df, T, lb, ub, T_lo=None, T_out=None, info=None, work=None, stream=None):
    """torch fp64 CUDA tensors, the optimizer's run of arguments, T_lo (B, m) or None; x is overwritten with every
    row's result.  Returns (x, T_out (B, m), info (B, 8)): per row the best point of the MMA loop on cost + opts.rho
    sum(T) over lb <= x <= ub and max(t_min, T_lo) <= T <= t_max, and the columns of JOINT_INFO.  T_out may not be T.
    Asynchronous; capturable when the outputs and `work` (a uint8 tensor of at least joint_workspace_bytes(B, m) bytes)
    are the caller's.  opts: a GtopJointOpt."""
    L = joint_library()
    args = ctx._bounded_problem(x, Df, T, lb, ub)
    B, m = args[:2]
    plo = None if T_lo is None else ctx._dev("T_lo", T_lo, B * m)
    T_out, pout = ctx._out("T_out", T_out, (B, m), x)
    info, pinfo = ctx._out("info", info, (B, len(JOINT_INFO)), x)
    if work is None:
        need = joint_workspace_bytes(B, m) if B >= 0 and 2 <= m <= 227 else 0   # (else: refused below)
        work = ctx._new((max(need, 1),), x, _th().uint8)
    pwork = ctx._dev("work", work, work.numel(), _th().uint8)
    ctx._chk(L.gtop_optimize_joint_device(ctx._h, C.byref(opts), *args, plo, pout, pinfo, pwork, work.numel(),
                                          _stream(stream, x)))
    return x, T_out, info


def joint_gradient_batch(ctx, x, want_parts=True):
    """(cost (B,), gx (B, n), gT (B, m), parts (B, m, 4) or None) of the first B rows of the context's problem at free
    variables x (B, n), host arrays."""
    L = joint_library()
    x = _f64(x)
    B, m = x.shape[0], getattr(ctx, "m", 0)   # (no problem: the library refuses)
    cost, gx, gT = np.empty(B), np.empty(x.shape), np.empty((B, m))
    parts = np.empty((B, m, len(TIME_PARTS))) if want_parts else None
    ctx._chk(L.gtop_joint_gradient_batch(ctx._h, B, _p(x), _p(cost), _p(gx), _p(gT),
                                         None if parts is None else _p(parts)))
    return cost, gx, gT, parts


def optimize_joint(ctx, opts, x0, lb, ub, T_lo=None):
    """Host arrays; (x (B, n), T_out (B, m), info (B, 8)) of the first B rows of the context's problem; T_lo (B, m) or
    None."""
    L = joint_library()
    x = _f64(x0).copy()
    B, m = x.shape[0], getattr(ctx, "m", 0)
    lb, ub = _f64(lb), _f64(ub)
    if not (lb.shape == x.shape == ub.shape):
        raise ValueError(f"lb, ub: expected the shape of x0, {x.shape}")
    plo = None
    if T_lo is not None:
        T_lo = _f64(T_lo)
        if T_lo.shape != (B, m):
            raise ValueError(f"T_lo: expected shape {(B, m)}, got {T_lo.shape}")
        plo = _p(T_lo)
    T_out, info = np.empty((B, m)), np.empty((B, len(JOINT_INFO)))
    ctx._chk(L.gtop_optimize_joint(ctx._h, C.byref(opts), B, _p(x), _p(lb), _p(ub), plo, _p(T_out), _p(info)))
    return x, T_out, info


__all__ = ["JOINT_INFO", "JOINT_ABI_VERSION", "JOINT_ENTRY_POINTS", "GtopJointOpt", "joint_library", "joint_abi_version",
           "joint_workspace_bytes", "joint_gradient_device", "joint_gradient_batch", "optimize_joint_device",
           "optimize_joint"]
