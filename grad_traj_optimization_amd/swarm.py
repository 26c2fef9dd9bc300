"""Pairwise separation as a cost (include/gtop_swarm.h: gtop_swarm_gradient_device, gtop_swarm_gradient_batch,
gtop_optimize_swarm_device, gtop_optimize_swarm) over a GtopContext.

separation_device reports how close the rows of a batch come to each other; this module is the term that moves them
apart.  swarm_gradient_device returns, per row, the penalty S_b on every partner closer than `radius` on the common
clock — a cubic hinge in the squared distance — and its gradient with respect to the row's free variables, against the
batch itself or against a frozen copy of it.  optimize_swarm_device is the decentralised swarm planner built on it: in
every sweep each row minimises its own cost plus S_b against the plans the others had at the sweep's start, by the
batched MMA loop.  The swarm's total is sum(S) / 2.

The companion header has its own table and its own version, apart from _abi.ENTRY_POINTS and ABI_VERSION (which speak
of include/gtop.h alone): the table is bound onto load_library()'s handle at first use.

Functions of a context, not methods of it: the device forms are built on the context's own argument helpers
(GtopContext._problem, _trajectory, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import library_path, load_library
from ._lib import _f64, _p, _stream, _th
from .separation import SEP_MAX_B, SEP_MAX_SAMPLES

# the version of include/gtop_swarm.h this module speaks: gtop_swarm_abi_version() of the in-tree build
SWARM_ABI_VERSION = 1


class GtopSwarmOpts(C.Structure):
    """gtop_swarm_opts of include/gtop_swarm.h: the grid tau_k = t_lo + k dt, k = 0 .. n_samples - 1, on the common
    clock and hold_ends, as GtopSepOpts; the weight w >= 0 of the term and the radius > 0 of interaction; two reserved
    words that must be 0."""
    _fields_ = [("t_lo", C.c_double), ("dt", C.c_double), ("w", C.c_double), ("radius", C.c_double),
                ("n_samples", C.c_int32), ("hold_ends", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, t_lo=0.0, dt=0.01, n_samples=256, w=1.0, radius=1.0, hold_ends=False, reserved=(0, 0)):
        super().__init__(float(t_lo), float(dt), float(w), float(radius), int(n_samples), int(hold_ends),
                         (C.c_int32 * 2)(*(int(r) for r in reserved)))


class GtopSwarmStop(C.Structure):
    """gtop_swarm_stop of include/gtop_swarm.h: the number of sweeps and of evaluations per row in a sweep (each
    >= 1); two reserved words that must be 0."""
    _fields_ = [("sweeps", C.c_int32), ("evals_per_sweep", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, sweeps=4, evals_per_sweep=25, reserved=(0, 0)):
        super().__init__(int(sweeps), int(evals_per_sweep), (C.c_int32 * 2)(*(int(r) for r in reserved)))


_i, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
_opt, _stop = C.POINTER(GtopSwarmOpts), C.POINTER(GtopSwarmStop)
# Every entry point of include/gtop_swarm.h: name -> (the header version that introduced it; restype; argtypes)
SWARM_ENTRY_POINTS = {
    "gtop_swarm_abi_version": (1, _i, []),
    "gtop_swarm_workspace_bytes": (1, _i, [_i, _i, _i, C.POINTER(C.c_size_t)]),
    "gtop_swarm_gradient_device": (1, _i, [_vp, _opt, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "gtop_swarm_gradient_batch": (1, _i, [_vp, _opt, _i, _dp, _dp, _dp, _dp, _dp]),
    "gtop_optimize_swarm_device": (1, _i, [_vp, _opt, _stop, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                           C.c_size_t, _vp]),
    "gtop_optimize_swarm": (1, _i, [_vp, _opt, _stop, _i, _dp, _dp, _dp, _dp, _dp]),
}

_bound = None


def swarm_library():
    """load_library()'s handle with SWARM_ENTRY_POINTS bound onto it.  Raises where the library has no swarm term: an
    older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_swarm_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_swarm_abi_version: it was built before include/gtop_swarm.h "
                          "and has no swarm separation cost (GTOP_HIP_LIB names an older build?)")
    L.gtop_swarm_abi_version.restype = C.c_int
    have = L.gtop_swarm_abi_version()
    for name, (since, restype, argtypes) in SWARM_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def swarm_abi_version():
    """gtop_swarm_abi_version() of the library in use."""
    return swarm_library().gtop_swarm_abi_version()


def swarm_workspace_bytes(B, m, n_samples):
    """The bytes of workspace the device forms need for B rows of m segments on n_samples samples (pure: no context,
    no GPU)."""
    n = C.c_size_t(0)
    if swarm_library().gtop_swarm_workspace_bytes(int(B), int(m), int(n_samples), C.byref(n)) != 0:
        raise ValueError(f"swarm_workspace_bytes: need 0 <= B <= {SEP_MAX_B}, 2 <= m <= 227 and 1 <= n_samples <= "
                         f"{SEP_MAX_SAMPLES}, got B = {B}, m = {m}, n_samples = {n_samples}")
    return int(n.value)


def _work(ctx, work, B, m, opts, like):
    """(tensor, address, bytes) of the workspace: the caller's, or one made here (then the call is not capturable)."""
    if work is None:
        need = 0
        if 0 <= B <= SEP_MAX_B and 2 <= m <= 227 and 1 <= opts.n_samples <= SEP_MAX_SAMPLES:   # (else: refused below)
            need = swarm_workspace_bytes(B, m, opts.n_samples)
        work = ctx._new((max(need, 1),), like, _th().uint8)
    return work, ctx._dev("work", work, work.numel(), _th().uint8), work.numel()


def swarm_gradient_device(ctx, opts, coeff, T, coeff_frozen=None, S=None, grad=None, active=None, want_active=False,
                          work=None, stream=None):
    """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,), coeff_frozen (B, m, 18) or None -> (S (B,), grad
    (B, 9 (m - 1)), active (B,) or None): per row the swarm penalty against the other rows of the batch (coeff_frozen
    None) or against the frozen rows j != i, its gradient with respect to the row's free variables, and (given, or
    want_active) the number of active terms.  Asynchronous, capturable when every output and `work` are the caller's
    (a uint8 tensor of at least swarm_workspace_bytes(B, m, opts.n_samples) bytes).  The start times are the context's,
    read when the kernels run.  opts: a GtopSwarmOpts."""
    L = swarm_library()
    B, m, pcoeff, pT, stride = ctx._trajectory(coeff, T)
    pfrozen = None if coeff_frozen is None else ctx._dev("coeff_frozen", coeff_frozen, B * m * 18)
    S, pS = ctx._out("S", S, (B,), coeff)
    grad, pg = ctx._out("grad", grad, (B, 9 * (m - 1)), coeff)
    pact = None
    if active is not None or want_active:
        active, pact = ctx._out("active", active, (B,), coeff)
    work, pwork, nwork = _work(ctx, work, B, m, opts, coeff)
    ctx._chk(L.gtop_swarm_gradient_device(ctx._h, C.byref(opts), B, m, pcoeff, pfrozen, pT, stride, pS, pg, pact, pwork,
                                          nwork, _stream(stream, coeff)))
    return S, grad, active


def swarm_gradient_batch(ctx, opts, x, x_frozen=None, want_active=True):
    """(S (B,), grad (B, n), active (B,) or None) of the first B rows of the context's problem at free variables x
    (B, n), host arrays; x_frozen (B, n) or None."""
    L = swarm_library()
    x = _f64(x)
    B = x.shape[0]
    pf = None
    if x_frozen is not None:
        x_frozen = _f64(x_frozen)
        if x_frozen.shape != x.shape:
            raise ValueError(f"x_frozen: expected the shape of x, {x.shape}, got {x_frozen.shape}")
        pf = _p(x_frozen)
    S, grad = np.empty(B), np.empty(x.shape)
    active = np.empty(B) if want_active else None
    ctx._chk(L.gtop_swarm_gradient_batch(ctx._h, C.byref(opts), B, _p(x), pf, _p(S), _p(grad),
                                         None if active is None else _p(active)))
    return S, grad, active


def optimize_swarm_device(ctx, opts, stop, x, Df, T, lb, ub, min_cost=None, joint=None, want_joint=False, work=None,
                          stream=None):
    """torch fp64 CUDA tensors, the optimizer's run of arguments; x is overwritten with every row's result.  Returns
    (x, min_cost (B,), joint (B, 2) or None): the last sweep's least cost + S_b per row and (given, or want_joint) the
    closing joint evaluation, the context's own cost | S_b with the others unfrozen.  Asynchronous; capturable after a
    first call when the outputs and `work` are the caller's.  opts: a GtopSwarmOpts; stop: a GtopSwarmStop."""
    L = swarm_library()
    args = ctx._bounded_problem(x, Df, T, lb, ub)
    B, m = args[:2]
    min_cost, pcost = ctx._out("min_cost", min_cost, (B,), x)
    pjoint = None
    if joint is not None or want_joint:
        joint, pjoint = ctx._out("joint", joint, (B, 2), x)
    work, pwork, nwork = _work(ctx, work, B, m, opts, x)
    ctx._chk(L.gtop_optimize_swarm_device(ctx._h, C.byref(opts), C.byref(stop), *args, pcost, pjoint, pwork, nwork,
                                          _stream(stream, x)))
    return x, min_cost, joint


def optimize_swarm(ctx, opts, stop, x0, lb, ub, want_joint=True):
    """Host arrays; (x (B, n), min_cost (B,), joint (B, 2) or None) of the first B rows of the context's problem."""
    L = swarm_library()
    x = _f64(x0).copy()
    B = x.shape[0]
    lb, ub = _f64(lb), _f64(ub)
    if not (lb.shape == x.shape == ub.shape):
        raise ValueError(f"lb, ub: expected the shape of x0, {x.shape}")
    min_cost = np.empty(B)
    joint = np.empty((B, 2)) if want_joint else None
    ctx._chk(L.gtop_optimize_swarm(ctx._h, C.byref(opts), C.byref(stop), B, _p(x), _p(lb), _p(ub), _p(min_cost),
                                   None if joint is None else _p(joint)))
    return x, min_cost, joint


__all__ = ["SWARM_ABI_VERSION", "SWARM_ENTRY_POINTS", "GtopSwarmOpts", "GtopSwarmStop", "swarm_library",
           "swarm_abi_version", "swarm_workspace_bytes", "swarm_gradient_device", "swarm_gradient_batch",
           "optimize_swarm_device", "optimize_swarm"]
