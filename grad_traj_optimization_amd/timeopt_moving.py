"""The segment times as variables under the moving-obstacle cost (include/gtop_time_moving.h:
gtop_time_gradient_moving_device, gtop_time_gradient_moving_batch, gtop_optimize_times_moving_device,
gtop_optimize_times_moving) over a GtopContext.

timeopt's entry points refuse while set_moving_cost is on: under absolute sample times a segment time moves the
lookups of every later segment.  These form that derivative — the time derivative of the box-lowered lookup, chained
through the prefix sum of T — and run timeopt's optimizer on it, so that "optimise x, optimise T, optimise x, report /
certify" stays on the device with boxes set: slowing down to let a box pass, or speeding up to get through before it
arrives, changes no waypoint.  With the mode off, or on without boxes, they return what timeopt's return.

The options structure is timeopt's GtopTimeOpt, the info row TIMEOPT_INFO.  The companion header has its own table and
its own version, apart from _abi.ENTRY_POINTS and timeopt.TIME_ENTRY_POINTS: the table is bound onto load_library()'s
handle at first use.  Functions of a context, built on its own argument helpers, as timeopt's are."""
import ctypes as C

import numpy as np

from ._abi import library_path, load_library
from ._lib import _f64, _p, _stream
from .timeopt import TIMEOPT_INFO, GtopTimeOpt

# the columns of a parts row (GTOP_TIME_MOVING_PARTS): timeopt.TIME_PARTS, then q_s — what the segment's cost gains per
# second of delay of its start — and R_s, the sum of q over the later segments
TIME_MOVING_PARTS = ("smooth", "collision", "d_smooth", "d_collision", "d_start", "later_segments")
# the version of include/gtop_time_moving.h this module speaks
TIME_MOVING_ABI_VERSION = 1

_i, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
_opt = C.POINTER(GtopTimeOpt)
# Every entry point of include/gtop_time_moving.h: name -> (the header version that introduced it; restype; argtypes)
TIME_MOVING_ENTRY_POINTS = {
    "gtop_time_moving_abi_version": (1, _i, []),
    "gtop_time_gradient_moving_device": (1, _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gtop_time_gradient_moving_batch": (1, _i, [_vp, _i, _dp, _dp, _dp, _dp, _dp]),
    "gtop_optimize_times_moving_device": (1, _i, [_vp, _opt, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "gtop_optimize_times_moving": (1, _i, [_vp, _opt, _i, _dp, _dp, _dp, _dp]),
}

_bound = None


def time_moving_library():
    """load_library()'s handle with TIME_MOVING_ENTRY_POINTS bound onto it.  Raises where the library has no
    segment-time gradient under the moving-obstacle cost: an older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_time_moving_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_time_moving_abi_version: it was built before "
                          "include/gtop_time_moving.h (GTOP_HIP_LIB names an older build?)")
    L.gtop_time_moving_abi_version.restype = C.c_int
    have = L.gtop_time_moving_abi_version()
    for name, (since, restype, argtypes) in TIME_MOVING_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def time_moving_abi_version():
    """gtop_time_moving_abi_version() of the library in use."""
    return time_moving_library().gtop_time_moving_abi_version()


def time_gradient_moving_device(ctx, x, Df, T, cost=None, gT=None, gt0=None, parts=None, want_gt0=True,
                                want_parts=False, stream=None):
    """torch fp64 CUDA tensors x (B, 9 (m - 1)), Df (18 B elements), T (B, m) or (m,) -> (cost (B,), gT (B, m), gt0
    (B,) or None, parts (B, m, 6) or None): the cost eval_device returns for the context's state — its boxes and start
    times included when the moving cost is in force —, its derivative with respect to every segment time and (given,
    or want_gt0) to the row's start time, and (given, or want_parts) the columns of TIME_MOVING_PARTS per segment.
    One launch; asynchronous, capturable when every output is the caller's."""
    L = time_moving_library()
    prob = ctx._problem(x, Df, T)
    B, m = prob[:2]
    cost, pcost = ctx._out("cost", cost, (B,), x)
    gT, pg = ctx._out("gT", gT, (B, m), x)
    pgt0 = pparts = None
    if gt0 is not None or want_gt0:
        gt0, pgt0 = ctx._out("gt0", gt0, (B,), x)
    if parts is not None or want_parts:
        parts, pparts = ctx._out("parts", parts, (B, m, len(TIME_MOVING_PARTS)), x)
    ctx._chk(L.gtop_time_gradient_moving_device(ctx._h, *prob, pcost, pg, pgt0, pparts, _stream(stream, x)))
    return cost, gT, gt0, parts


def optimize_times_moving_device(ctx, opts, x, Df, T, T_lo=None, T_out=None, info=None, stream=None):
    """timeopt.optimize_times_device with the pass above as its evaluation: (T_out (B, m), info (B, 8)).  T_out may
    not be T.  One launch; asynchronous, capturable when both outputs are the caller's.  opts: a GtopTimeOpt."""
    L = time_moving_library()
    prob = ctx._problem(x, Df, T)
    B, m = prob[:2]
    plo = None if T_lo is None else ctx._dev("T_lo", T_lo, B * m)
    T_out, pout = ctx._out("T_out", T_out, (B, m), x)
    info, pinfo = ctx._out("info", info, (B, len(TIMEOPT_INFO)), x)
    ctx._chk(L.gtop_optimize_times_moving_device(ctx._h, C.byref(opts), *prob, plo, pout, pinfo, _stream(stream, x)))
    return T_out, info


def time_gradient_moving_batch(ctx, x, want_parts=True):
    """(cost (B,), gT (B, m), gt0 (B,), parts (B, m, 6) or None) of the first B rows of the context's problem at free
    variables x (B, n), host arrays."""
    L = time_moving_library()
    x = _f64(x)
    B, m = x.shape[0], getattr(ctx, "m", 0)   # (no problem: the library refuses)
    cost, gT, gt0 = np.empty(B), np.empty((B, m)), np.empty(B)
    parts = np.empty((B, m, len(TIME_MOVING_PARTS))) if want_parts else None
    ctx._chk(L.gtop_time_gradient_moving_batch(ctx._h, B, _p(x), _p(cost), _p(gT), _p(gt0),
                                               None if parts is None else _p(parts)))
    return cost, gT, gt0, parts


def optimize_times_moving(ctx, opts, x, T_lo=None):
    """(T_out (B, m), info (B, 8)) of the first B rows of the context's problem at free variables x (B, n), host
    arrays; T_lo (B, m) or None."""
    L = time_moving_library()
    x = _f64(x)
    B, m = x.shape[0], getattr(ctx, "m", 0)
    plo = None
    if T_lo is not None:
        T_lo = _f64(T_lo)
        if T_lo.shape != (B, m):
            raise ValueError(f"T_lo: expected shape {(B, m)}, got {T_lo.shape}")
        plo = _p(T_lo)
    T_out, info = np.empty((B, m)), np.empty((B, len(TIMEOPT_INFO)))
    ctx._chk(L.gtop_optimize_times_moving(ctx._h, C.byref(opts), B, _p(x), plo, _p(T_out), _p(info)))
    return T_out, info


__all__ = ["TIME_MOVING_PARTS", "TIME_MOVING_ABI_VERSION", "TIME_MOVING_ENTRY_POINTS", "time_moving_library",
           "time_moving_abi_version", "time_gradient_moving_device", "time_gradient_moving_batch",
           "optimize_times_moving_device", "optimize_times_moving"]
