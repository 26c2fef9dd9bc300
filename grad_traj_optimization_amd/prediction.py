"""Moving-obstacle predictions fitted from observation histories (include/gtop_prediction.h: gtop_fit_predictions_device,
gtop_refresh_box_predictions_device, gtop_fit_predictions) over a GtopContext.

set_moving_box_polynomials takes the reference's PolynomialPrediction; these produce it: the reference's predictPolyFit
(a regularised least-squares quintic through an object's recent (x, y, z, t) history) and predictConstVel (a line
through the last two observations), batched over objects.  fit_predictions_device leaves coef, t_range as the setter
takes them; refresh_box_predictions_device writes the same fit straight into the context's polynomial box list on the
caller's stream, so a loop of "new observations, new predictions, optimise with the moving cost, report, certify" stays
on the device and can be captured as one graph; fit_predictions is the host form (no context, no GPU), with the same
bits.

The companion header has its own table and its own version, apart from _abi.ENTRY_POINTS and ABI_VERSION (which speak
of include/gtop.h alone): the table is bound onto load_library()'s handle at first use.

Functions of a context, not methods of it: the device forms are built on the context's own argument helpers
(GtopContext._dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import GtopError, library_path, load_library
from ._lib import _f64, _p, _stream, _th

# the columns of an info row (GTOP_PRED_INFO)
PRED_INFO = ("status", "count", "degree", "t_start", "t_last", "t_end", "resmax_x", "resmax_y", "resmax_z", "rms",
             "pad0", "pad1")
PRED_LOCAL = 20
# the version of include/gtop_prediction.h this module speaks: gtop_pred_abi_version() of the in-tree build
PRED_ABI_VERSION = 1
PREDICT_POLYFIT, PREDICT_CONST_VEL = 0, 1
PRED_OK, PRED_LOWERED, PRED_EMPTY, PRED_BAD = 0, 1, 2, 3


class GtopPredictOpts(C.Structure):
    """gtop_predict_opts of include/gtop_prediction.h: mode (PREDICT_POLYFIT: the regularised least-squares fit of
    `degree` 1 .. 5 with weight `lambda_` on the integral of the squared second derivative; PREDICT_CONST_VEL: the line
    through the last two samples); horizon >= 0 (+inf allowed): the row is valid on [t_first, t_last + horizon], 0 being
    the reference's interval; regularise_horizon: the integral runs to t_last + horizon; inflate >= 0: the refresh adds
    inflate * resmax_k to a box's half extent; a reserved word that must be 0."""
    _fields_ = [("mode", C.c_int32), ("degree", C.c_int32), ("lambda_", C.c_double), ("horizon", C.c_double),
                ("inflate", C.c_double), ("regularise_horizon", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, mode=PREDICT_POLYFIT, degree=5, lambda_=1.0, horizon=0.0, regularise_horizon=False, inflate=0.0,
                 reserved=0):
        super().__init__(int(mode), int(degree), float(lambda_), float(horizon), float(inflate),
                         int(regularise_horizon), int(reserved))


_i, _vp, _dp, _i32p = C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
_opts = C.POINTER(GtopPredictOpts)
# Every entry point of include/gtop_prediction.h: name -> (the header version that introduced it; restype; argtypes)
PRED_ENTRY_POINTS = {
    "gtop_pred_abi_version": (1, _i, []),
    "gtop_fit_predictions_device": (1, _i, [_vp, _i, _i, _vp, _vp, _vp, _opts, _vp, _vp, _vp, _vp, _vp]),
    "gtop_refresh_box_predictions_device": (1, _i, [_vp, _i, _i, _vp, _vp, _vp, _opts, _vp, _vp, _vp]),
    "gtop_fit_predictions": (1, _i, [_i, _i, _dp, _i32p, _i32p, _opts, _dp, _dp, _dp, _dp]),
}

_bound = None


def pred_library():
    """load_library()'s handle with PRED_ENTRY_POINTS bound onto it.  Raises where the library has no prediction fit: an
    older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_pred_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_pred_abi_version: it was built before include/gtop_prediction.h "
                          "and fits no predictions (GTOP_HIP_LIB names an older build?)")
    L.gtop_pred_abi_version.restype = C.c_int
    have = L.gtop_pred_abi_version()
    for name, (since, restype, argtypes) in PRED_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def pred_abi_version():
    """gtop_pred_abi_version() of the library in use."""
    return pred_library().gtop_pred_abi_version()


def _histories(ctx, hist, count, head):
    """hist (N, H, 4) fp64, count (N,) int32, head (N,) int32 or None -> (N, H, their addresses)."""
    if hist.dim() != 3 or hist.shape[2] != 4:
        raise ValueError(f"hist: expected shape (N, H, 4), got {tuple(hist.shape)}")
    N, H = hist.shape[:2]
    i32 = _th().int32
    return (N, H, ctx._dev("hist", hist, N * H * 4), ctx._dev("count", count, N, i32),
            None if head is None else ctx._dev("head", head, N, i32))


def fit_predictions_device(ctx, hist, count, opts, head=None, coef=None, t_range=None, info=None, local=None,
                           want_local=False, stream=None):
    """torch CUDA tensors hist (N, H, 4) fp64 (x, y, z, t per slot), count (N,) int32, head (N,) int32 or None (each
    history a ring: sample i is slot (head + i) mod H, oldest first) -> (coef (N, 18), t_range (N, 2), info (N, 12),
    local (N, 20) or None): coef and t_range as set_moving_box_polynomials takes them, the columns of PRED_INFO, and
    (given, or want_local) the accurate local form.  Rows of an object whose status is PRED_EMPTY or PRED_BAD are left
    as they were (new tensors are zeroed).  One launch; asynchronous, capturable when every output is the caller's.
    opts: a GtopPredictOpts."""
    L = pred_library()
    N, H, phist, pcount, phead = _histories(ctx, hist, count, head)
    coef, pcoef = ctx._out("coef", coef, (N, 18), hist, make="zeros")
    t_range, ptr = ctx._out("t_range", t_range, (N, 2), hist, make="zeros")
    info, pinfo = ctx._out("info", info, (N, len(PRED_INFO)), hist)
    plocal = None
    if local is not None or want_local:
        local, plocal = ctx._out("local", local, (N, PRED_LOCAL), hist, make="zeros")
    ctx._chk(L.gtop_fit_predictions_device(ctx._h, N, H, phist, pcount, phead, C.byref(opts), pcoef, ptr, pinfo, plocal,
                                           _stream(stream, hist)))
    return coef, t_range, info, local


def refresh_box_predictions_device(ctx, hist, count, opts, head=None, scale=None, info=None, stream=None):
    """The same fit written straight into the context's polynomial box list (set_moving_box_polynomials with exactly N
    boxes must be in force: GtopError GTOP_ERR_STATE otherwise, nothing written) -> info (N, 12).  scale (N, 3) fp64,
    the full extents: the half extent written is 0.5 scale + opts.inflate * resmax; None keeps the extents in force.
    Everything enqueued behind it on `stream` reads the new rows; one launch, asynchronous, capturable when info is
    the caller's.  A captured refresh must be captured again after a setter that grows the box list."""
    L = pred_library()
    N, H, phist, pcount, phead = _histories(ctx, hist, count, head)
    pscale = None if scale is None else ctx._dev("scale", scale, N * 3)
    info, pinfo = ctx._out("info", info, (N, len(PRED_INFO)), hist)
    ctx._chk(L.gtop_refresh_box_predictions_device(ctx._h, N, H, phist, pcount, phead, C.byref(opts), pscale, pinfo,
                                                   _stream(stream, hist)))
    return info


def fit_predictions(hist, count, opts, head=None, want_local=True, fill=0.0):
    """The host form (no context, no GPU), the same bits: hist (N, H, 4), count (N,), head (N,) or None -> (coef (N,
    18), t_range (N, 2), info (N, 12), local (N, 20) or None).  Rows of an object that was not fitted hold `fill`."""
    L = pred_library()
    hist = _f64(hist)
    if hist.ndim != 3 or hist.shape[2] != 4:
        raise ValueError(f"hist: expected shape (N, H, 4), got {hist.shape}")
    N, H = hist.shape[:2]
    count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
    if count.shape[0] != N:
        raise ValueError(f"count: expected {N} entries, got {count.shape[0]}")
    phead = None
    if head is not None:
        head = np.ascontiguousarray(head, dtype=np.int32).reshape(-1)
        if head.shape[0] != N:
            raise ValueError(f"head: expected {N} entries, got {head.shape[0]}")
        phead = head.ctypes.data_as(_i32p)
    coef, t_range, info = np.full((N, 18), fill), np.full((N, 2), fill), np.zeros((N, len(PRED_INFO)))
    local = np.full((N, PRED_LOCAL), fill) if want_local else None
    rc = L.gtop_fit_predictions(N, H, _p(hist), count.ctypes.data_as(_i32p), phead, C.byref(opts), _p(coef), _p(t_range),
                                _p(info), None if local is None else _p(local))
    if rc != 0:
        raise GtopError(rc, "fit_predictions: bad arguments (mode, 1 <= degree <= 5, finite lambda >= 0, horizon >= 0, "
                            "finite inflate >= 0, regularise_horizon with a finite horizon, reserved 0, H >= 1)")
    return coef, t_range, info, local


__all__ = ["PRED_INFO", "PRED_LOCAL", "PRED_ABI_VERSION", "PRED_ENTRY_POINTS", "PREDICT_POLYFIT", "PREDICT_CONST_VEL",
           "PRED_OK", "PRED_LOWERED", "PRED_EMPTY", "PRED_BAD", "GtopPredictOpts", "pred_library", "pred_abi_version",
           "fit_predictions_device", "refresh_box_predictions_device", "fit_predictions"]
