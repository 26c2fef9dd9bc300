"""Waypoint insertion (include/gtop.h: gtop_insert_waypoints_device, gtop_insert_waypoints) over a GtopContext.

A row that the report or the certificate calls unsafe has no free variable where the collision is.  The insertion cuts
one segment of every row in two — at a trajectory time (a column of a device report) or the longest segment in the
middle — and hands back a problem of m + 1 segments that describes the same curve: x_out, T_out and, when the bounds
of x are given, lb_out and ub_out, ready for GtopContext.optimize_device_ex.

Functions of a context, not methods of it: the device form is built on the context's own argument helpers
(GtopContext._trajectory, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import GtopInsert
from ._lib import _f64, _p, _stream

# the columns of an info row (GTOP_INSERT_INFO of include/gtop.h)
INSERT_INFO = ("segment", "local_time", "fell_back", "clamped", "distance", "pushed")


def insert_waypoints_device(ctx, opts, x, coeff, T, when=None, when_column=0, lb=None, ub=None, x_out=None, T_out=None,
                            lb_out=None, ub_out=None, info=None, want_info=True, stream=None):
    """torch fp64 CUDA tensors x (B, 9 (m - 1)), coeff (B, m, 18), T (B, m) or (m,) -> (x_out (B, 9 m), T_out
    (B, m + 1), lb_out, ub_out (B, 9 m) or None, info (B, 6) or None); asynchronous, capturable (pass the outputs to
    write into buffers of the caller's).  opts: a GtopInsert.

    when (AT_TIME; not read under LONGEST): a tensor (B,) of trajectory times, or a whole device report (B, k) of which
    column `when_column` holds them — validate_device's report with when_column=2, a certificate with 3 or 4 — read in
    place, with a stride of k doubles.  lb, ub (B, 9 (m - 1)): both or neither; with them lb_out and ub_out are made.
    want_info=False leaves the info row out.  Outputs must not overlap inputs."""
    B, m, pcoeff, pT, stride = ctx._trajectory(coeff, T)
    px = ctx._dev("x", x, B * 9 * (m - 1))
    pwhen, when_stride = None, 1
    if when is not None:
        when_stride = 1 if when.dim() == 1 else int(when.shape[-1])
        if not (when.dim() in (1, 2) and 0 <= int(when_column) < when_stride):
            raise ValueError(f"when: expected shape (B,) or (B, k) with 0 <= when_column < k, got {tuple(when.shape)} "
                             f"and column {when_column}")
        pwhen = ctx._dev("when", when, B * when_stride) + 8 * int(when_column)
    if (lb is None) != (ub is None):
        raise ValueError("lb, ub: both or neither")
    plb = pub = plb_out = pub_out = None
    if lb is not None:
        plb, pub = ctx._dev("lb", lb, B * 9 * (m - 1)), ctx._dev("ub", ub, B * 9 * (m - 1))
        lb_out, plb_out = ctx._out("lb_out", lb_out, (B, 9 * m), x)
        ub_out, pub_out = ctx._out("ub_out", ub_out, (B, 9 * m), x)
    elif lb_out is not None or ub_out is not None:
        raise ValueError("lb_out, ub_out: given without lb and ub")
    x_out, px_out = ctx._out("x_out", x_out, (B, 9 * m), x)
    T_out, pT_out = ctx._out("T_out", T_out, (B, m + 1), x)
    pinfo = None
    if want_info or info is not None:
        info, pinfo = ctx._out("info", info, (B, len(INSERT_INFO)), x)
    ctx._chk(ctx._L.gtop_insert_waypoints_device(ctx._h, C.byref(opts), B, m, px, pcoeff, pT, stride, pwhen, when_stride,
                                                 plb, pub, px_out, pT_out, plb_out, pub_out, pinfo, _stream(stream, x)))
    return x_out, T_out, lb_out, ub_out, info


def insert_waypoints(ctx, x, opts, when=None, lb=None, ub=None):
    """The same for the first B rows of the context's problem at free variables x (B, n), host arrays: (x_out (B, 9 m),
    T_out (B, m + 1), lb_out, ub_out or None, info (B, 6)).  when (B,): required under AT_TIME.  The context's problem is
    not changed: pass T_out to set_problem."""
    x = _f64(x)
    B, m = x.shape[0], ctx.m
    if (lb is None) != (ub is None):
        raise ValueError("lb, ub: both or neither")
    x_out, T_out, info = np.empty((B, 9 * m)), np.empty((B, m + 1)), np.empty((B, len(INSERT_INFO)))
    pwhen = plb = pub = plb_out = pub_out = None
    lb_out = ub_out = None
    if when is not None:
        when = _f64(when).reshape(-1)
        if when.shape[0] != B:
            raise ValueError(f"when: expected {B} entries, one per row of x, got {when.shape[0]}")
        pwhen = _p(when)
    if lb is not None:
        lb, ub = _f64(lb), _f64(ub)
        if not (lb.shape == x.shape == ub.shape):
            raise ValueError(f"lb, ub: expected the shape of x, {x.shape}")
        lb_out, ub_out = np.empty((B, 9 * m)), np.empty((B, 9 * m))
        plb, pub, plb_out, pub_out = _p(lb), _p(ub), _p(lb_out), _p(ub_out)
    ctx._chk(ctx._L.gtop_insert_waypoints(ctx._h, C.byref(opts), B, _p(x), pwhen, plb, pub, _p(x_out), _p(T_out), plb_out,
                                          pub_out, _p(info)))
    return x_out, T_out, lb_out, ub_out, info


__all__ = ["INSERT_INFO", "GtopInsert", "insert_waypoints_device", "insert_waypoints"]
