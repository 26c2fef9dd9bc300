"""Pairwise separation of the rows of a batch and the selection of distinct candidates (include/gtop_separation.h:
gtop_separation_device, gtop_separation_batch, gtop_select_distinct_device) over a GtopContext.

Every other figure of the library speaks of one row alone.  separation_device gives, for every pair of rows, the least
and the greatest distance between the two curves on a common time grid (pair_min, pair_max: (B, B), symmetric) and a
row summary (the columns of SEP_ROW): the mutual clearance of rows that are the robots of a swarm (with the context's
per-row start times), and the distance by which select_distinct_device tells the candidates of one robot apart — the
K cheapest passing rows that are pairwise at least min_gap apart somewhere on the grid.

The companion header has its own table and its own version, apart from _abi.ENTRY_POINTS and ABI_VERSION (which speak
of include/gtop.h alone): the table is bound onto load_library()'s handle at first use.

Functions of a context, not methods of it: the device forms are built on the context's own argument helpers
(GtopContext._trajectory, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import library_path, load_library
from ._lib import _f64, _p, _stream, _th

# the columns of a row summary (GTOP_SEP_ROW)
SEP_ROW = ("min_dist", "min_dist_row", "min_dist_t", "n_within_radius", "n_overlapping", "n_flown")
# the version of include/gtop_separation.h this module speaks: gtop_sep_abi_version() of the in-tree build
SEP_ABI_VERSION = 1
SEP_MAX_SAMPLES, SEP_MAX_B, SEP_MAX_DISTINCT = 65536, 4096, 64


class GtopSepOpts(C.Structure):
    """gtop_sep_opts of include/gtop_separation.h: the grid tau_k = t_lo + k dt, k = 0 .. n_samples - 1, on the common
    clock; the radius of the row summary's count (<= 0 or NaN: nothing is counted); hold_ends (False: a row exists only
    while it is flown; True: it stands at its start before and at its end after); two reserved words that must be 0."""
    _fields_ = [("t_lo", C.c_double), ("dt", C.c_double), ("radius", C.c_double), ("n_samples", C.c_int32),
                ("hold_ends", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, t_lo=0.0, dt=0.01, n_samples=256, radius=0.0, hold_ends=False, reserved=(0, 0)):
        super().__init__(float(t_lo), float(dt), float(radius), int(n_samples), int(hold_ends),
                         (C.c_int32 * 2)(*(int(r) for r in reserved)))


_i, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
_sep = C.POINTER(GtopSepOpts)
# Every entry point of include/gtop_separation.h: name -> (the header version that introduced it; restype; argtypes)
SEP_ENTRY_POINTS = {
    "gtop_sep_abi_version": (1, _i, []),
    "gtop_separation_workspace_bytes": (1, _i, [_i, _i, C.POINTER(C.c_size_t)]),
    "gtop_separation_device": (1, _i, [_vp, _i, _i, _vp, _vp, _i, _sep, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "gtop_separation_batch": (1, _i, [_vp, _i, _dp, _sep, _dp, _dp, _dp]),
    "gtop_select_distinct_device": (1, _i, [_vp, _i, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _vp]),
}

_bound = None


def sep_library():
    """load_library()'s handle with SEP_ENTRY_POINTS bound onto it.  Raises where the library has no separation
    figures: an older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_sep_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_sep_abi_version: it was built before include/gtop_separation.h "
                          "and has no pairwise separation (GTOP_HIP_LIB names an older build?)")
    L.gtop_sep_abi_version.restype = C.c_int
    have = L.gtop_sep_abi_version()
    for name, (since, restype, argtypes) in SEP_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def separation_workspace_bytes(B, n_samples):
    """The bytes of workspace separation_device needs for B rows on n_samples samples (pure: no context, no GPU)."""
    n = C.c_size_t(0)
    if sep_library().gtop_separation_workspace_bytes(int(B), int(n_samples), C.byref(n)) != 0:
        raise ValueError(f"separation_workspace_bytes: need 0 <= B <= {SEP_MAX_B} and 1 <= n_samples <= "
                         f"{SEP_MAX_SAMPLES}, got B = {B}, n_samples = {n_samples}")
    return int(n.value)


def separation_device(ctx, coeff, T, opts, pair_min=None, pair_max=None, rows=None, work=None, stream=None):
    """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> (pair_min (B, B), pair_max (B, B), rows (B, 6)),
    the columns of SEP_ROW; asynchronous, capturable when every output and `work` are the caller's (a uint8 tensor of
    at least separation_workspace_bytes(B, opts.n_samples) bytes; made here when None).  The start times are the
    context's (set_start_times[_device]), read when the kernels run.  opts: a GtopSepOpts."""
    L = sep_library()
    traj = ctx._trajectory(coeff, T)
    B = traj[0]
    pair_min, pmin = ctx._out("pair_min", pair_min, (B, B), coeff)
    pair_max, pmax = ctx._out("pair_max", pair_max, (B, B), coeff)
    rows, prows = ctx._out("rows", rows, (B, len(SEP_ROW)), coeff)
    if work is None:
        need = 0
        if 0 <= B <= SEP_MAX_B and 1 <= opts.n_samples <= SEP_MAX_SAMPLES:    # (otherwise the library refuses the call)
            need = separation_workspace_bytes(B, opts.n_samples)
        work = ctx._new((max(need, 1),), coeff, _th().uint8)
    pwork = ctx._dev("work", work, work.numel(), _th().uint8)
    ctx._chk(L.gtop_separation_device(ctx._h, *traj, C.byref(opts), pmin, pmax, prows, pwork, work.numel(),
                                      _stream(stream, coeff)))
    return pair_min, pair_max, rows


def separation_batch(ctx, x, opts):
    """(pair_min (B, B), pair_max (B, B), rows (B, 6)) of the first B rows of the context's problem at free variables
    x (B, n), host arrays."""
    L = sep_library()
    x = _f64(x)
    B = x.shape[0]
    pair_min, pair_max, rows = np.empty((B, B)), np.empty((B, B)), np.empty((B, len(SEP_ROW)))
    ctx._chk(L.gtop_separation_batch(ctx._h, B, _p(x), C.byref(opts), _p(pair_min), _p(pair_max), _p(rows)))
    return pair_min, pair_max, rows


def select_distinct_device(ctx, passed, cost, pair_max, min_gap, k, chosen=None, count=None, stream=None):
    """passed (B,) uint8 or None, cost (B,), pair_max (B, B) torch CUDA tensors -> (chosen (k,) int32, count (1,)
    int32): greedily the cheapest eligible row (passed != 0, finite cost; the lowest index on a tie), then the cheapest
    one whose pair_max against every row chosen so far is >= min_gap, until none qualifies or k are chosen; the rest
    of `chosen` is -1.  chosen[0] is best[0] of the select_best family on the same pass and cost; asynchronous,
    capturable."""
    L = sep_library()
    B = cost.numel()
    ppass = None if passed is None else ctx._dev("passed", passed, B, _th().uint8)
    pcost, ppm = ctx._dev("cost", cost, B), ctx._dev("pair_max", pair_max, B * B)
    chosen, pchosen = ctx._out("chosen", chosen, (max(int(k), 0),), cost, _th().int32)
    count, pcount = ctx._out("count", count, (1,), cost, _th().int32)
    ctx._chk(L.gtop_select_distinct_device(ctx._h, B, ppass, pcost, ppm, float(min_gap), int(k), pchosen, pcount,
                                           _stream(stream, cost)))
    return chosen, count


__all__ = ["SEP_ROW", "SEP_ABI_VERSION", "SEP_ENTRY_POINTS", "SEP_MAX_SAMPLES", "SEP_MAX_B", "SEP_MAX_DISTINCT",
           "GtopSepOpts", "sep_library", "separation_workspace_bytes", "separation_device", "separation_batch",
           "select_distinct_device"]
