"""The continuous-time clearance certificate (include/gtop.h: gtop_certify_trajectories_device, gtop_certify_batch,
gtop_select_best_certified_device; gtop_certify_moving_device, gtop_certify_moving_batch) over a GtopContext.

The sampled report (GtopContext.validate_device) says that none of the getTraj samples is within the margin; the
certificate bounds the interpolated distance over whole time intervals, so "SAFE" speaks about every point of the
curve.  certify_device / certify_batch speak about the STATIC field; certify_moving_device / certify_moving_batch about
the field AND the context's moving boxes (either kind of list) at the start times' clock, every point of the curve
against every time of its interval.  Both give the same (B, 8) rows, which select_best_certified_device takes.

Functions of a context, not methods of it: the device forms are built on the context's own argument helpers
(GtopContext._trajectory, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import GtopCertifyMovingOpts, GtopCertifyOpts
from ._lib import _f64, _p, _stream, _th

# the columns of a certificate row (GTOP_CERT_REPORT of include/gtop.h)
CERT_REPORT = ("verdict", "lo", "hi", "hi_t", "first_violation_t", "n_undecided", "n_refinements", "time_sum")
UNSAFE, UNDECIDED, SAFE = -1, 0, 1
# `require` of select_best_certified_device (GTOP_CERT_REQUIRE_*)
REQUIRE_SAFE, REQUIRE_NOT_UNSAFE = 1, 2


def certify_device(ctx, coeff, T, opts, cert=None, stream=None):
    """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> cert (B, 8), the columns of CERT_REPORT;
    asynchronous, capturable (pass `cert` to write into a buffer of the caller's).  opts: a GtopCertifyOpts."""
    traj = ctx._trajectory(coeff, T)
    cert, pcert = ctx._out("cert", cert, (traj[0], len(CERT_REPORT)), coeff)
    ctx._chk(ctx._L.gtop_certify_trajectories_device(ctx._h, *traj, C.byref(opts), pcert, _stream(stream, coeff)))
    return cert


def certify_moving_device(ctx, coeff, T, opts, cert=None, stream=None):
    """certify_device against the static field and the context's moving boxes: opts is a GtopCertifyMovingOpts
    (use_boxes False, or no boxes set: certify_device's result, bit for bit).  The boxes, the start times and the field
    are read when the launch runs; asynchronous, capturable."""
    traj = ctx._trajectory(coeff, T)
    cert, pcert = ctx._out("cert", cert, (traj[0], len(CERT_REPORT)), coeff)
    ctx._chk(ctx._L.gtop_certify_moving_device(ctx._h, *traj, C.byref(opts), pcert, _stream(stream, coeff)))
    return cert


def select_best_certified_device(ctx, report, cert, cost, limits, require=REQUIRE_SAFE, want_pass=True, best=None,
                                 stream=None):
    """report (B, 12), cert (B, 8), cost (B,) torch fp64 CUDA tensors -> (pass (B,) uint8 or None, best (2,) int32):
    GtopContext.select_best_device's rule, and the row's verdict must be SAFE (REQUIRE_SAFE) or must not be UNSAFE
    (REQUIRE_NOT_UNSAFE); asynchronous, capturable."""
    B = cost.numel()
    preport = ctx._dev("report", report, B * len(ctx.TRAJ_REPORT))
    pcert, pcost = ctx._dev("cert", cert, B * len(CERT_REPORT)), ctx._dev("cost", cost, B)
    ok, pok = ctx._out("pass", None, (B,), report, _th().uint8) if want_pass else (None, None)
    best, pbest = ctx._out("best", best, (2,), report, _th().int32)
    ctx._chk(ctx._L.gtop_select_best_certified_device(ctx._h, B, preport, pcert, pcost, C.byref(limits), int(require),
                                                      pok, pbest, _stream(stream, report)))
    return ok, best


def certify_batch(ctx, x, opts):
    """The certificates (B, 8) of the first B rows of the context's problem at free variables x (B, n), host arrays."""
    x = _f64(x)
    B = x.shape[0]
    cert = np.empty((B, len(CERT_REPORT)))
    ctx._chk(ctx._L.gtop_certify_batch(ctx._h, B, _p(x), C.byref(opts), _p(cert)))
    return cert


def certify_moving_batch(ctx, x, opts):
    """certify_batch against the static field and the context's moving boxes; opts: a GtopCertifyMovingOpts."""
    x = _f64(x)
    B = x.shape[0]
    cert = np.empty((B, len(CERT_REPORT)))
    ctx._chk(ctx._L.gtop_certify_moving_batch(ctx._h, B, _p(x), C.byref(opts), _p(cert)))
    return cert


__all__ = ["CERT_REPORT", "UNSAFE", "UNDECIDED", "SAFE", "REQUIRE_SAFE", "REQUIRE_NOT_UNSAFE", "GtopCertifyOpts",
           "GtopCertifyMovingOpts", "certify_device", "certify_moving_device", "select_best_certified_device",
           "certify_batch", "certify_moving_batch"]
