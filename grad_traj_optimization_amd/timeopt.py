"""The segment times as variables (include/gtop_time.h: gtop_time_gradient_device, gtop_time_gradient_batch,
gtop_optimize_times_device, gtop_optimize_times) over a GtopContext.

Everything else the library optimises is a function of the free waypoint derivatives x at fixed segment times T.
time_gradient_device returns the derivative of the same cost with respect to every T_s — with the waypoint values held
in x and Df a segment depends on its own time alone —, and optimize_times_device minimises cost + rho sum(T) over the
segment times by a projected gradient descent with backtracking, one wavefront per trajectory, in one launch.  Its
output is a legal T for every entry point that takes the problem triple, so "optimise x, optimise T, optimise x, report
/ certify" stays on the device and can be captured as one graph; the output of reallocate_times_device(LIMITS) is a
legal T_lo ("never faster than the limits allow").

The companion header has its own table and its own version, apart from _abi.ENTRY_POINTS and ABI_VERSION (which speak
of include/gtop.h alone): the table is bound onto load_library()'s handle at first use.

Functions of a context, not methods of it: the device forms are built on the context's own argument helpers
(GtopContext._problem, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import library_path, load_library
from ._lib import _f64, _p, _stream

# the columns of an info row (GTOP_TIMEOPT_INFO) and of a parts row (GTOP_TIME_PARTS)
TIMEOPT_INFO = ("code", "accepted", "evals", "F_start", "F", "cost", "free_gradient", "time_sum")
TIME_PARTS = ("smooth", "collision", "d_smooth", "d_collision")
# the version of include/gtop_time.h this module speaks: gtop_time_abi_version() of the in-tree build
TIME_ABI_VERSION = 1
FTOL_REACHED, XTOL_REACHED, MAXEVAL_REACHED = 3, 4, 5


class GtopTimeOpt(C.Structure):
    """gtop_timeopt of include/gtop_time.h: rho >= 0, the weight of sum(T); the bounds 0.0301 <= t_min <= t_max of
    every segment time; first_move > 0, the seconds the first trial moves the segment of largest |gradient|; the stop
    rules ftol_rel (relative decrease of an accepted step), xtol_abs (largest move of a trial, seconds) and max_evals;
    a reserved word that must be 0."""
    _fields_ = [("rho", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double), ("first_move", C.c_double),
                ("ftol_rel", C.c_double), ("xtol_abs", C.c_double), ("max_evals", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, rho=0.0, t_min=0.05, t_max=60.0, first_move=0.05, ftol_rel=1e-6, xtol_abs=1e-9, max_evals=40,
                 reserved=0):
        super().__init__(float(rho), float(t_min), float(t_max), float(first_move), float(ftol_rel), float(xtol_abs),
                         int(max_evals), int(reserved))


_i, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
_opt = C.POINTER(GtopTimeOpt)
# Every entry point of include/gtop_time.h: name -> (the header version that introduced it; restype; argtypes)
TIME_ENTRY_POINTS = {
    "gtop_time_abi_version": (1, _i, []),
    "gtop_time_gradient_device": (1, _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "gtop_time_gradient_batch": (1, _i, [_vp, _i, _dp, _dp, _dp, _dp]),
    "gtop_optimize_times_device": (1, _i, [_vp, _opt, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "gtop_optimize_times": (1, _i, [_vp, _opt, _i, _dp, _dp, _dp, _dp]),
}

_bound = None


def time_library():
    """load_library()'s handle with TIME_ENTRY_POINTS bound onto it.  Raises where the library has no segment-time
    gradient: an older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_time_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_time_abi_version: it was built before include/gtop_time.h and "
                          "has no segment-time gradient (GTOP_HIP_LIB names an older build?)")
    L.gtop_time_abi_version.restype = C.c_int
    have = L.gtop_time_abi_version()
    for name, (since, restype, argtypes) in TIME_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def time_abi_version():
    """gtop_time_abi_version() of the library in use."""
    return time_library().gtop_time_abi_version()


def time_gradient_device(ctx, x, Df, T, cost=None, gT=None, parts=None, want_parts=False, stream=None):
    """torch fp64 CUDA tensors x (B, 9 (m - 1)), Df (18 B elements), T (B, m) or (m,) -> (cost (B,), gT (B, m), parts
    (B, m, 4) or None): the callback's cost, its derivative with respect to every segment time, and (given, or
    want_parts) the columns of TIME_PARTS per segment.  One launch; asynchronous, capturable when every output is the
    caller's."""
    L = time_library()
    prob = ctx._problem(x, Df, T)
    B, m = prob[:2]
    cost, pcost = ctx._out("cost", cost, (B,), x)
    gT, pg = ctx._out("gT", gT, (B, m), x)
    pparts = None
    if parts is not None or want_parts:
        parts, pparts = ctx._out("parts", parts, (B, m, len(TIME_PARTS)), x)
    ctx._chk(L.gtop_time_gradient_device(ctx._h, *prob, pcost, pg, pparts, _stream(stream, x)))
    return cost, gT, parts


def optimize_times_device(ctx, opts, x, Df, T, T_lo=None, T_out=None, info=None, stream=None):
    """The same problem triple, T_lo (B, m) or None -> (T_out (B, m), info (B, 8)): per row the minimiser of cost +
    opts.rho sum(T) over max(t_min, T_lo) <= T <= t_max found by the rule of include/gtop_time.h, and the columns of
    TIMEOPT_INFO.  T_out may not be T.  One launch; asynchronous, capturable when both outputs are the caller's.
    opts: a GtopTimeOpt."""
    L = time_library()
    prob = ctx._problem(x, Df, T)
    B, m = prob[:2]
    plo = None if T_lo is None else ctx._dev("T_lo", T_lo, B * m)
    T_out, pout = ctx._out("T_out", T_out, (B, m), x)
    info, pinfo = ctx._out("info", info, (B, len(TIMEOPT_INFO)), x)
    ctx._chk(L.gtop_optimize_times_device(ctx._h, C.byref(opts), *prob, plo, pout, pinfo, _stream(stream, x)))
    return T_out, info


def time_gradient_batch(ctx, x, want_parts=True):
    """(cost (B,), gT (B, m), parts (B, m, 4) or None) of the first B rows of the context's problem at free variables x
    (B, n), host arrays."""
    L = time_library()
    x = _f64(x)
    B, m = x.shape[0], getattr(ctx, "m", 0)   # (no problem: the library refuses)
    cost, gT = np.empty(B), np.empty((B, m))
    parts = np.empty((B, m, len(TIME_PARTS))) if want_parts else None
    ctx._chk(L.gtop_time_gradient_batch(ctx._h, B, _p(x), _p(cost), _p(gT), None if parts is None else _p(parts)))
    return cost, gT, parts


def optimize_times(ctx, opts, x, T_lo=None):
    """(T_out (B, m), info (B, 8)) of the first B rows of the context's problem at free variables x (B, n), host
    arrays; T_lo (B, m) or None."""
    L = time_library()
    x = _f64(x)
    B, m = x.shape[0], getattr(ctx, "m", 0)
    plo = None
    if T_lo is not None:
        T_lo = _f64(T_lo)
        if T_lo.shape != (B, m):
            raise ValueError(f"T_lo: expected shape {(B, m)}, got {T_lo.shape}")
        plo = _p(T_lo)
    T_out, info = np.empty((B, m)), np.empty((B, len(TIMEOPT_INFO)))
    ctx._chk(L.gtop_optimize_times(ctx._h, C.byref(opts), B, _p(x), plo, _p(T_out), _p(info)))
    return T_out, info


__all__ = ["TIMEOPT_INFO", "TIME_PARTS", "TIME_ABI_VERSION", "TIME_ENTRY_POINTS", "FTOL_REACHED", "XTOL_REACHED",
           "MAXEVAL_REACHED", "GtopTimeOpt", "time_library", "time_abi_version", "time_gradient_device",
           "time_gradient_batch", "optimize_times_device", "optimize_times"]
