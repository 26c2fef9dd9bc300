"""The continuous-time certificate of pairwise separation (include/gtop_separation_certificate.h:
gtop_certify_separation_device, gtop_certify_separation_batch) over a GtopContext.

separation_device gives the least distance of two rows on a time grid and knows nothing between two samples.
certify_separation_device bounds the distance of every pair of rows over the pair's whole common window of time, on the
interval tree of the other certificates: per pair a verdict (SAFE / UNDECIDED / UNSAFE against opts.min_sep), a
certified lower bound `lo` of the distance, the least distance met `hi` and where, and a row summary — with the
context's per-row start times, the mutual clearance of the robots of a swarm in continuous time.

The companion header has its own table and its own version, apart from _abi.ENTRY_POINTS and from
separation.SEP_ENTRY_POINTS: the table is bound onto load_library()'s handle at first use.

Functions of a context, not methods of it: the device form is built on the context's own argument helpers
(GtopContext._trajectory, _dev, _out), so the device-argument rules stated there hold here unchanged."""
import ctypes as C

import numpy as np

from ._abi import library_path, load_library
from ._lib import _f64, _p, _stream, _th

# the columns of a pair's row (GTOP_SEPCERT_PAIR) and of a row summary (GTOP_SEPCERT_ROW)
SEPCERT_PAIR = ("verdict", "lo", "hi", "hi_t", "first_violation_t", "n_open", "n_refined", "n_pieces")
SEPCERT_ROW = ("verdict", "min_lo", "min_lo_row", "min_hi", "min_hi_row", "min_hi_t", "first_violation_t", "n_unsafe",
               "n_undecided", "n_boxed")
# the version of include/gtop_separation_certificate.h this module speaks
SEPCERT_ABI_VERSION = 1
SEPCERT_MAX_B = 2048
SAFE, UNDECIDED, UNSAFE = 1, 0, -1


class GtopSepCertOpts(C.Structure):
    """gtop_sepcert_opts of include/gtop_separation_certificate.h: the separation required; the window [t_lo, t_hi] on
    the common clock (infinite ends allowed without hold_ends: the rows' flown ranges bound it); the tree's depth
    (0 .. 3) and the refinement budget per PAIR; hold_ends as GtopSepOpts; cull (True: pairs whose row boxes are at
    least min_sep apart are certified at once); two reserved words that must be 0."""
    _fields_ = [("min_sep", C.c_double), ("t_lo", C.c_double), ("t_hi", C.c_double), ("max_depth", C.c_int32),
                ("max_refine", C.c_int32), ("hold_ends", C.c_int32), ("cull", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, min_sep=0.5, t_lo=-np.inf, t_hi=np.inf, max_depth=2, max_refine=64, hold_ends=False, cull=False,
                 reserved=(0, 0)):
        super().__init__(float(min_sep), float(t_lo), float(t_hi), int(max_depth), int(max_refine), int(hold_ends),
                         int(cull), (C.c_int32 * 2)(*(int(r) for r in reserved)))


_i, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
_opt = C.POINTER(GtopSepCertOpts)
# Every entry point of the header: name -> (the header version that introduced it; restype; argtypes)
SEPCERT_ENTRY_POINTS = {
    "gtop_sepcert_abi_version": (1, _i, []),
    "gtop_sepcert_workspace_bytes": (1, _i, [_i, C.POINTER(C.c_size_t)]),
    "gtop_certify_separation_device": (1, _i, [_vp, _i, _i, _vp, _vp, _i, _opt, _vp, _vp, _vp, C.c_size_t, _vp]),
    "gtop_certify_separation_batch": (1, _i, [_vp, _i, _dp, _opt, _dp, _dp]),
}

_bound = None


def sepcert_library():
    """load_library()'s handle with SEPCERT_ENTRY_POINTS bound onto it.  Raises where the library has no separation
    certificate: an older build chosen through GTOP_HIP_LIB."""
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    if not hasattr(L, "gtop_sepcert_abi_version"):
        raise ImportError(f"{library_path()} has no gtop_sepcert_abi_version: it was built before "
                          "include/gtop_separation_certificate.h (GTOP_HIP_LIB names an older build?)")
    L.gtop_sepcert_abi_version.restype = C.c_int
    have = L.gtop_sepcert_abi_version()
    for name, (since, restype, argtypes) in SEPCERT_ENTRY_POINTS.items():
        if since <= have:
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _bound = L
    return L


def sepcert_workspace_bytes(B):
    """The bytes of workspace certify_separation_device needs for B rows (pure: no context, no GPU)."""
    n = C.c_size_t(0)
    if sepcert_library().gtop_sepcert_workspace_bytes(int(B), C.byref(n)) != 0:
        raise ValueError(f"sepcert_workspace_bytes: need 0 <= B <= {SEPCERT_MAX_B}, got B = {B}")
    return int(n.value)


def certify_separation_device(ctx, coeff, T, opts, pairs=None, rows=None, work=None, stream=None):
    """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> (pairs (B, B, 8), rows (B, 10)), the columns of
    SEPCERT_PAIR and SEPCERT_ROW; asynchronous, capturable when both outputs and `work` are the caller's (a uint8
    tensor of at least sepcert_workspace_bytes(B) bytes; made here when None).  The start times are the context's
    (set_start_times[_device]), read when the kernels run.  opts: a GtopSepCertOpts."""
    L = sepcert_library()
    traj = ctx._trajectory(coeff, T)
    B = traj[0]
    pairs, ppairs = ctx._out("pairs", pairs, (B, B, len(SEPCERT_PAIR)), coeff)
    rows, prows = ctx._out("rows", rows, (B, len(SEPCERT_ROW)), coeff)
    if work is None:
        need = sepcert_workspace_bytes(B) if 0 <= B <= SEPCERT_MAX_B else 0    # (otherwise the library refuses the call)
        work = ctx._new((max(need, 1),), coeff, _th().uint8)
    pwork = ctx._dev("work", work, work.numel(), _th().uint8)
    ctx._chk(L.gtop_certify_separation_device(ctx._h, *traj, C.byref(opts), ppairs, prows, pwork, work.numel(),
                                              _stream(stream, coeff)))
    return pairs, rows


def certify_separation_batch(ctx, x, opts):
    """(pairs (B, B, 8), rows (B, 10)) of the first B rows of the context's problem at free variables x (B, n), host
    arrays."""
    L = sepcert_library()
    x = _f64(x)
    B = x.shape[0]
    pairs, rows = np.empty((B, B, len(SEPCERT_PAIR))), np.empty((B, len(SEPCERT_ROW)))
    ctx._chk(L.gtop_certify_separation_batch(ctx._h, B, _p(x), C.byref(opts), _p(pairs), _p(rows)))
    return pairs, rows


__all__ = ["SEPCERT_PAIR", "SEPCERT_ROW", "SEPCERT_ABI_VERSION", "SEPCERT_ENTRY_POINTS", "SEPCERT_MAX_B", "SAFE",
           "UNDECIDED", "UNSAFE", "GtopSepCertOpts", "sepcert_library", "sepcert_workspace_bytes",
           "certify_separation_device", "certify_separation_batch"]
