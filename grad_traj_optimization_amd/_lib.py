"""ctypes binding of include/gtop.h (the C-ABI of libgtop_hip.so): the classes over the entry points of _abi.py.

A device tensor reaches the library as a raw address, and the library cannot know how long the buffer behind it is.
So every *_device method states, per tensor, what the entry point reads or writes, and GtopContext._dev refuses
(ValueError) whatever is not that before anything is called."""
import ctypes as C
import math

import numpy as np

from ._abi import (GTOP_F32, GTOP_F64, OPTI_NODE_PARAMS, _HERE, _SO, _STATUS, GtopError, GtopLimits,  # noqa: F401
                   GtopParams, GtopRetime, GtopStop, _preload_torch_hip_runtime, library_path, load_library)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


_torch = None


def _th():
    """torch, imported at first use: this module imports without it, for the build and for callers of the host arrays."""
    global _torch
    if _torch is None:
        import torch
        _torch = torch
    return _torch


def _stream(stream, tensor):
    """The stream argument of every method that has one, as the library takes it: None is torch's current stream on
    `tensor`'s device, an object with .cuda_stream (a torch Stream) is that handle, anything else is the handle."""
    if stream is None:
        stream = _th().cuda.current_stream(tensor.get_device())     # by index: a device object costs torch microseconds
    return getattr(stream, "cuda_stream", stream)


_PRECISIONS = {}


def _precision(name, t):
    """GTOP_F64 or GTOP_F32: the two precisions a field or an evaluation may have."""
    if not _PRECISIONS:
        _PRECISIONS.update({_th().float64: GTOP_F64, _th().float32: GTOP_F32})
    code = _PRECISIONS.get(t.dtype)
    if code is None:
        raise ValueError(f"{name}: expected a float64 or float32 tensor, got {t.dtype}")
    return code


def box_polynomial_centres(coef, times, t_range=None):
    """Centres (ntimes, nbox, 3) of polynomial boxes at `times`, by the arithmetic every kernel uses (the clamp into
    [t1, t2], then Horner in fp64 fmas; include/gtop.h, gtop_box_polynomial_centres).  Host only: no context, no GPU."""
    L = load_library()
    coef = _f64(coef).reshape(-1, 3, 6)
    times = _f64(np.atleast_1d(times)).reshape(-1)
    tr = None
    if t_range is not None:
        tr = _f64(t_range).reshape(-1, 2)
        if tr.shape[0] != coef.shape[0]:
            raise ValueError("t_range: expected one (t1, t2) per box")
    out = np.empty((times.shape[0], coef.shape[0], 3))
    rc = L.gtop_box_polynomial_centres(coef.shape[0], _p(coef), None if tr is None else _p(tr), times.shape[0], _p(times),
                                       _p(out))
    if rc != 0:
        raise GtopError(rc, "box_polynomial_centres: bad arguments (a non-finite coefficient, t1 > t2, a NaN bound)")
    return out


class _Handle:
    """Owner of one handle `_h` of the library `_L`.  `_prefix` names the handle's family of entry points: its
    <prefix>destroy runs once, at close() or collection, and _chk turns a status into a GtopError that carries
    <prefix>last_error."""
    _prefix = "gtop_"

    def _fn(self, name):
        return getattr(self._L, self._prefix + name)

    def _chk(self, rc):
        if rc != 0:
            raise GtopError(rc, self._fn("last_error")(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _HostProblem(_Handle):
    """What a context and a group of contexts do alike with host arrays."""

    def set_params(self, **kw):
        d = dict(OPTI_NODE_PARAMS)
        d.update(kw)
        self.params = d
        p = GtopParams(**d)
        self._chk(self._fn("set_params")(self._h, C.byref(p)))

    def set_problem(self, T, Df):
        Df = _f64(Df)
        B = Df.size // 18
        T = _f64(T)
        if T.ndim == 2:
            m, stride = T.shape[1], T.shape[1]
            if T.shape[0] != B:
                raise ValueError(f"T: expected {B} rows, one per 18 entries of Df, got {T.shape[0]}")
        else:
            m, stride = T.shape[0], 0
        self._chk(self._fn("set_problem")(self._h, B, m, _p(T), stride, _p(Df)))
        self.B, self.m = B, m

    def optimize_batch_ex(self, x0, lb, ub, max_evals, ftol_rel=0.0, xtol_rel=0.0, maxtime=0.0):
        """As optimize_batch, with NLopt's other stop rules; returns (x, cost, nevals, code).

        What lb / ub may hold, per variable (lb <= ub; include/gtop.h): -inf / +inf on either side — the side is
        open, the variable starts with asymptote width sigma = 1 and its sigma is never clamped to
        [0.01, 10] (ub - lb); lb == ub — the variable never moves and is returned as given; a start outside the box is
        clamped into it before the first evaluation.  The returned point lies inside [lb, ub] exactly."""
        x = _f64(x0).copy()
        B = x.shape[0]
        lb, ub = _f64(lb), _f64(ub)
        cost = np.empty(B)
        nev = np.empty(B, dtype=np.int32)
        code = np.empty(B, dtype=np.int32)
        stop = GtopStop(int(max_evals), float(ftol_rel), float(xtol_rel), float(maxtime))
        ip = C.POINTER(C.c_int32)
        self._chk(self._fn("optimize_batch_ex")(self._h, B, _p(x), _p(lb), _p(ub), C.byref(stop), _p(cost),
                                                nev.ctypes.data_as(ip), code.ctypes.data_as(ip)))
        return x, cost, nev, code


class GtopContext(_HostProblem):
    """One gtop_ctx (one per host thread / HIP stream)."""

    def __init__(self, device=0, params=None):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.gtop_create(C.byref(h), int(device))
        if rc != 0:
            raise GtopError(rc, self._L.gtop_last_error(None).decode()
                            + " — a gfx950 GPU is required; there is no CPU fallback")
        self._h = h
        self.device = int(device)
        self.set_params(**(params or {}))

    # -- device arguments --
    def _dev(self, name, t, count, dtype=None):
        """The address of tensor `t` (an int: the entry point's argtypes make it a void *), once `t` is what the entry
        point reads or writes: on this context's device (get_device() is -1 for a host tensor), contiguous, of `dtype`
        (None: float64) and of exactly `count` elements."""
        if dtype is None:
            dtype = _th().float64
        if not (t.get_device() == self.device and t.dtype == dtype and t.numel() == count and t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous {dtype} tensor of {count} elements on cuda:{self.device}, "
                             f"got {'a' if t.is_contiguous() else 'a non-contiguous'} {t.dtype} tensor of shape "
                             f"{tuple(t.shape)} on {t.device}")
        return t.data_ptr()

    def _new(self, shape, like, dtype=None, make="empty"):
        """The output a caller left out: a new tensor on `like`'s device (make="zeros": zeroed)."""
        return getattr(_th(), make)(shape, dtype=dtype or _th().float64, device=like.device)

    def _out(self, name, t, shape, like, dtype=None, make="empty"):
        """(tensor, address) of an output of `shape`: the caller's `t`, held to what _dev asks, or a new one."""
        if t is None:
            t = self._new(shape, like, dtype, make)
        return t, self._dev(name, t, math.prod(shape), dtype)

    def _times(self, T, B, m, dtype=None):
        """Segment times -> (address, time stride): a 2-D T holds B m of them, one row per trajectory (stride m);
        any other holds m, shared by the batch (stride 0)."""
        stride = m if T.dim() == 2 else 0
        return self._dev("T", T, B * m if stride else m, dtype), stride

    def _problem(self, x, Df, T, dtype=None):
        """The problem triple x (B, n), Df (18 B elements), T, with n == 9 (m - 1) -> (B, m, x, Df, T, time stride),
        the run of arguments every entry point that takes the triple has."""
        shape = x.shape
        if len(shape) != 2 or shape[1] % 9:
            raise ValueError(f"x: expected shape (B, 9 (m - 1)), got {tuple(shape)}")
        B, n = shape
        m = n // 9 + 1
        return (B, m, self._dev("x", x, B * n, dtype), self._dev("Df", Df, B * 18, dtype), *self._times(T, B, m, dtype))

    def _trajectory(self, coeff, T):
        """The trajectory pair coeff (B, m, 18), T -> (B, m, coeff, T, time stride), likewise."""
        shape = coeff.shape
        if len(shape) != 3 or shape[2] != 18:
            raise ValueError(f"coeff: expected shape (B, m, 18), got {tuple(shape)}")
        B, m = shape[:2]
        return (B, m, self._dev("coeff", coeff, B * m * 18), *self._times(T, B, m))

    def _points(self, pts):
        """(N, 3) fp64 occupied points -> (the tensor to keep until the call is made, its address, N): a tensor made
        from np.argwhere's transposed view is column-major, so the copy into row-major is made here."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"pts: expected shape (N, 3), got {tuple(pts.shape)}")
        pts = pts.contiguous()
        return pts, self._dev("pts", pts, pts.shape[0] * 3), pts.shape[0]

    # -- configuration --
    def set_sdf(self, dist, grid, origin, resolution, map_size=None):
        dist = _f64(dist).reshape(-1)
        nx, ny, nz = (int(g) for g in grid)
        if dist.size != nx * ny * nz:
            raise ValueError(f"dist: expected {nx * ny * nz} entries, got {dist.size}")
        ms = _p(_f64(map_size)) if map_size is not None else None
        self._chk(self._L.gtop_set_sdf(self._h, _p(dist), nx, ny, nz, _p(_f64(origin)), ms, float(resolution)))
        self.grid = (nx, ny, nz)

    def set_sdf_device(self, tensor, grid, origin, resolution, map_size=None):
        dtype = _precision("tensor", tensor)
        nx, ny, nz = (int(g) for g in grid)
        ms = _p(_f64(map_size)) if map_size is not None else None
        self._chk(self._L.gtop_set_sdf_device(self._h, dtype, self._dev("tensor", tensor, nx * ny * nz, tensor.dtype),
                                              nx, ny, nz, _p(_f64(origin)), ms, float(resolution)))
        self._sdf_keepalive = tensor
        self.grid = (nx, ny, nz)

    def init_sdf_map(self, map_size, origin, resolution):
        self._chk(self._L.gtop_init_sdf_map(self._h, _p(_f64(map_size)), _p(_f64(origin)), float(resolution)))
        g = (C.c_int * 3)()
        self._chk(self._L.gtop_get_sdf(self._h, None, g))
        self.grid = tuple(g)

    def update_sdf_map(self, pts):
        pts = _f64(pts).reshape(-1, 3)
        self._chk(self._L.gtop_update_sdf_map(self._h, _p(pts), pts.shape[0]))

    def update_sdf_map_device(self, pts, stream=None):
        """pts: (N, 3) float64 CUDA tensor; asynchronous on `stream` (default: torch's current stream)."""
        pts, *points = self._points(pts)
        self._chk(self._L.gtop_update_sdf_map_device(self._h, *points, _stream(stream, pts)))

    def update_sdf_map_window(self, min_pos, max_pos, pts):
        """The reference's local update (compare2.cpp:147-152): resetBuffer(min, max), setOccupancy per point,
        updateESDF3d over the box (gtop_update_sdf_map_window)."""
        pts = _f64(pts).reshape(-1, 3)
        mn, mx = _f64(min_pos).reshape(3), _f64(max_pos).reshape(3)
        self._chk(self._L.gtop_update_sdf_map_window(self._h, _p(mn), _p(mx), _p(pts) if pts.size else None, pts.shape[0]))

    def update_sdf_map_window_device(self, min_pos, max_pos, pts, stream=None):
        mn, mx = _f64(min_pos).reshape(3), _f64(max_pos).reshape(3)
        pts, *points = self._points(pts)
        self._chk(self._L.gtop_update_sdf_map_window_device(self._h, _p(mn), _p(mx), *points, _stream(stream, pts)))

    def get_sdf(self):
        g = (C.c_int * 3)()
        self._chk(self._L.gtop_get_sdf(self._h, None, g))
        out = np.empty(g[0] * g[1] * g[2])
        self._chk(self._L.gtop_get_sdf(self._h, _p(out), g))
        return out.reshape(tuple(g))

    def set_optimizer_fusion(self, mode=2):
        """2 (or True): whole optimizer loop in one launch; 1: MMA update fused into the
        evaluation kernel, one launch per iteration; 0 (or False): separate update launch."""
        mode = 2 if mode is True else int(mode)
        self._chk(self._L.gtop_set_optimizer_fusion(self._h, mode))

    def set_optimizer_precision(self, dtype="f64"):
        """"f64" (default) or "f32": the arithmetic of the evaluations inside the batched optimizer (state, update
        and results stay fp64)."""
        self._chk(self._L.gtop_set_optimizer_precision(self._h, {"f64": GTOP_F64, "f32": GTOP_F32}[dtype]))

    def set_launch_geometry(self, waves=0, samples_per_lane=0):
        self._chk(self._L.gtop_set_launch_geometry(self._h, int(waves), int(samples_per_lane)))

    # -- evaluation --
    def eval_batch(self, x):
        """Host arrays in, host arrays out (fp64, PCIe copies included)."""
        x = _f64(x)
        B = x.shape[0]
        n = 9 * (self.m - 1)
        assert x.shape == (B, n)
        cost = np.empty(B)
        grad = np.empty((B, n))
        self._chk(self._L.gtop_eval_batch(self._h, B, _p(x), _p(cost), _p(grad)))
        return cost, grad

    def cost_nlopt(self, x, want_grad=True):
        """The nlopt_func-shaped entry point on trajectory 0."""
        x = _f64(x)
        g = np.empty_like(x) if want_grad else None
        c = self._L.gtop_cost_nlopt(x.size, _p(x), _p(g) if want_grad else None, self._h)
        if not np.isfinite(c):
            raise GtopError(1, self._L.gtop_last_error(self._h).decode())
        return c, g

    def eval_device(self, x, Df, T, cost=None, grad=None, stream=None):
        """torch CUDA tensors in HBM; launches on `stream` (default: torch's
        current stream) and returns without synchronising."""
        dtype = x.dtype
        prob = self._problem(x, Df, T, dtype)
        B, n = prob[0], 9 * (prob[1] - 1)
        if cost is None:    # not through _out: this is the one method whose host time per launch is measured
            cost = self._new((B,), x, dtype)
        if grad is None:
            grad = self._new((B, n), x, dtype)
        self._chk(self._L.gtop_eval_device(self._h, _precision("x", x), *prob, self._dev("cost", cost, B, dtype),
                                           self._dev("grad", grad, B * n, dtype), _stream(stream, x)))
        return cost, grad

    def set_field_precisions(self, keep_fp32=True):
        """False: keep fp64 corner records only (the capturable map updates then skip the fp32 pass; fp32 evaluations fail)."""
        self._chk(self._L.gtop_set_field_precisions(self._h, 1 if keep_fp32 else 0))

    def set_field_sign(self, signed=True, max_depth=0.0):
        """Signed (True) or unsigned (False, the default) distance field from the next whole-map build on: negative
        inside obstacles, max(-max_depth, res - distance to the nearest free voxel); max_depth 0 means 10000
        (include/gtop.h, gtop_set_field_sign)."""
        self._chk(self._L.gtop_set_field_sign(self._h, 1 if signed else 0, float(max_depth)))

    def field_sign(self):
        """(signed, max_depth) of the resident field."""
        mode, depth = C.c_int(), C.c_double()
        self._chk(self._L.gtop_get_field_sign(self._h, C.byref(mode), C.byref(depth)))
        return bool(mode.value), depth.value

    def push_rows(self, src, dst_ptrs, nbytes=None, stream=None, clock_minmax=None):
        """ONE kernel copies `src` (a contiguous CUDA tensor, or its first nbytes) to every device address in dst_ptrs
        (ints: slots in this process's and in peers' mapped buffers) — gtop_push_rows, the all-gather as stores."""
        held = src.numel() * src.element_size()
        if nbytes is None:
            nbytes = held
        if int(nbytes) > held:
            raise ValueError(f"nbytes: expected at most the {held} bytes of src, got {nbytes}")
        arr = (C.c_void_p * len(dst_ptrs))(*[int(p) for p in dst_ptrs])
        pclock = None if clock_minmax is None else self._dev("clock_minmax", clock_minmax, 2, _th().int64)
        self._chk(self._L.gtop_push_rows(self._h, self._dev("src", src, src.numel(), src.dtype), int(nbytes), arr,
                                         len(dst_ptrs), pclock, _stream(stream, src)))

    def shared_alloc(self, nbytes):
        """(device address, 64-byte handle) of a zeroed allocation another process can map (gtop_shared_alloc)."""
        ptr = C.c_void_p()
        h = C.create_string_buffer(64)
        self._chk(self._L.gtop_shared_alloc(self._h, int(nbytes), C.byref(ptr), h))
        return int(ptr.value), bytes(h.raw)

    def shared_open(self, handle, owner_device=-1):
        """Device address, for this context's device, of a buffer a peer process made with shared_alloc (owner_device:
        that process's device ordinal, so that peer access is checked and enabled first)."""
        ptr = C.c_void_p()
        self._chk(self._L.gtop_shared_open(self._h, C.create_string_buffer(bytes(handle), 64), int(owner_device),
                                           C.byref(ptr)))
        return int(ptr.value)

    def shared_close(self, ptr):
        self._chk(self._L.gtop_shared_close(self._h, C.c_void_p(int(ptr))))

    def shared_free(self, ptr):
        self._chk(self._L.gtop_shared_free(self._h, C.c_void_p(int(ptr))))

    def clock_stamp(self, minmax, stream=None):
        """Enqueue a device-clock stamp: minmax (torch int64 tensor of 2 on the device, preset to [2**63 - 1, 0])
        becomes [min(., t), max(., t)] of the device's wall clock (gtop_device_clock_stamp)."""
        self._chk(self._L.gtop_device_clock_stamp(self._h, self._dev("minmax", minmax, 2, _th().int64),
                                                  _stream(stream, minmax)))

    def clock_hz(self):
        hz = C.c_double()
        self._chk(self._L.gtop_device_clock_hz(self._h, C.byref(hz)))
        return hz.value

    # -- setup / post-processing --
    TRAJ_STATS = ("time_sum", "length", "jerk", "mean_v", "max_v", "mean_a", "max_a", "acc_cost", "n_samples")

    def set_paths(self, waypoints, mean_v=1.8, init_time=0.3):
        """setPath for a batch: (B, m+1, 3) waypoints -> the context's problem; returns x0 (B, n)."""
        wp = _f64(waypoints)
        B, npts, _ = wp.shape
        m = npts - 1
        x0 = np.empty((B, 9 * (m - 1)))
        self._chk(self._L.gtop_set_paths(self._h, B, m, _p(wp), float(mean_v), float(init_time), _p(x0)))
        self.B, self.m = B, m
        return x0

    def get_problem(self):
        T = np.empty((self.B, self.m))
        Df = np.empty((self.B, 3, 6))
        self._chk(self._L.gtop_get_problem(self._h, _p(T), _p(Df)))
        return T, Df

    def min_jerk_start(self, x):
        """The minimum-jerk start point of the first B rows of the context's problem (include/gtop.h,
        gtop_min_jerk_start): a NEW array (B, n) with the positions of x and, in the velocity and acceleration entries,
        the minimiser of the smoothness term at those positions."""
        out = _f64(x).copy()
        if out.ndim != 2 or out.shape[1] != 9 * (self.m - 1):
            raise ValueError(f"x: expected shape (B, {9 * (self.m - 1)})")
        self._chk(self._L.gtop_min_jerk_start(self._h, out.shape[0], _p(out)))
        return out

    def min_jerk_start_device(self, x, Df, T, stream=None):
        """The same IN PLACE on a torch fp64 CUDA tensor x (B, n), with Df (B, 18) and T (B, m) or (m,): overwrites
        the velocity and acceleration entries of x; asynchronous, capturable.  Returns x."""
        self._chk(self._L.gtop_min_jerk_start_device(self._h, *self._problem(x, Df, T), _stream(stream, x)))
        return x

    def trajectory_stats(self, x, dt_sample=0.01):
        """(coefficients (B, m, 18), stats (B, 9)) for the context's problem at free variables x."""
        x = _f64(x)
        B = x.shape[0]
        coeff = np.empty((B, self.m, 18))
        stats = np.empty((B, len(self.TRAJ_STATS)))
        self._chk(self._L.gtop_trajectory_stats(self._h, B, _p(x), float(dt_sample), _p(coeff), _p(stats)))
        return coeff, stats

    def trajectory_samples(self, x, dt_sample=0.01, max_samples=4096):
        """PolynomialTraj::getTraj for the context's problem at free variables x:
        (stats (B, 9), samples (B, max_samples, 3)); trajectory b has stats[b, 8] points."""
        x = _f64(x)
        B = x.shape[0]
        stats = np.empty((B, len(self.TRAJ_STATS)))
        samples = np.zeros((B, int(max_samples), 3))
        self._chk(self._L.gtop_trajectory_samples(self._h, B, _p(x), float(dt_sample), None, _p(stats), _p(samples),
                                                  int(max_samples)))
        return stats, samples

    # -- static field + moving boxes (EDTEnvironment) --
    def set_moving_boxes(self, p0, vel, scale):
        """Boxes {p0, vel, scale}, each (nbox, 3): centre p0 + vel*t, extent +-scale/2."""
        p0, vel, scale = (_f64(a).reshape(-1, 3) for a in (p0, vel, scale))
        if not (p0.shape == vel.shape == scale.shape):
            raise ValueError("p0, vel, scale: expected one row of 3 per box in each")
        self._chk(self._L.gtop_set_moving_boxes(self._h, p0.shape[0], _p(p0), _p(vel), _p(scale)))

    BOXES_CONST_VEL, BOXES_POLYNOMIAL = 0, 1

    def set_moving_box_polynomials(self, coef, scale, t_range=None):
        """The box list as polynomial predictions (include/gtop.h, gtop_set_moving_box_polynomials): coef (nbox, 3, 6),
        axis-major, ascending powers; scale (nbox, 3); t_range (nbox, 2) = {t1, t2} per box, None = unbounded.  Outside
        [t1, t2] a box stands where its prediction ends.  Replaces whatever list was set, of either kind."""
        coef = _f64(coef).reshape(-1, 3, 6)
        scale = _f64(scale).reshape(-1, 3)
        if coef.shape[0] != scale.shape[0]:
            raise ValueError("scale: expected one row of 3 per box of coef")
        tr = None
        if t_range is not None:
            tr = _f64(t_range).reshape(-1, 2)
            if tr.shape[0] != coef.shape[0]:
                raise ValueError("t_range: expected one (t1, t2) per box of coef")
        self._chk(self._L.gtop_set_moving_box_polynomials(self._h, coef.shape[0], _p(coef), None if tr is None else _p(tr),
                                                          _p(scale)))

    def moving_box_kind(self):
        """(kind, nbox) of the list in force: BOXES_CONST_VEL or BOXES_POLYNOMIAL."""
        kind, nbox = C.c_int(0), C.c_int(0)
        self._chk(self._L.gtop_get_moving_box_kind(self._h, C.byref(kind), C.byref(nbox)))
        return int(kind.value), int(nbox.value)

    # -- moving-obstacle cost (include/gtop.h: not in the reference's callback) --
    MOVING_COST_MAX_BOXES = 32

    def set_moving_cost(self, enable=True):
        """The collision term of every fp64 evaluation and optimizer run looks its samples up against the static field
        AND the boxes of set_moving_boxes at the sample's absolute time (start time + segment times + local time).
        Off by default; on without boxes nothing changes (include/gtop.h, gtop_set_moving_cost)."""
        self._chk(self._L.gtop_set_moving_cost(self._h, 1 if enable else 0))

    def moving_cost(self):
        on = C.c_int(0)
        self._chk(self._L.gtop_get_moving_cost(self._h, C.byref(on)))
        return bool(on.value)

    # -- gradient mode (include/gtop.h: not in the reference) --
    GRADIENT_REFERENCE, GRADIENT_CONSISTENT = 0, 1

    def set_gradient_mode(self, consistent=True):
        """Which gradient every evaluation and optimizer run of this context returns / uses: the reference's callback
        line by line (False, the default: a drop-in reproduces the reference's iterates) or the gradient of the cost as
        returned (True: the one to optimise with).  The cost is the same bit for bit (include/gtop.h,
        gtop_set_gradient_mode)."""
        self._chk(self._L.gtop_set_gradient_mode(self._h, self.GRADIENT_CONSISTENT if consistent else self.GRADIENT_REFERENCE))

    @property
    def gradient_mode(self):
        mode = C.c_int(0)
        self._chk(self._L.gtop_get_gradient_mode(self._h, C.byref(mode)))
        return int(mode.value)

    def set_start_times(self, t0=None):
        """The trajectories' start times on the boxes' clock: None = all zero, a scalar = one shared value, else one
        per trajectory of the batch evaluated; finite and >= 0."""
        if t0 is None:
            self._chk(self._L.gtop_set_start_times(self._h, 0, None))
            return
        t0 = _f64(np.atleast_1d(t0)).reshape(-1)
        self._chk(self._L.gtop_set_start_times(self._h, t0.shape[0], _p(t0)))

    def set_start_times_device(self, t0):
        """The same from a torch fp64 CUDA tensor, BORROWED: every launch reads it (a captured launch reads what it
        holds at replay), so the caller keeps it alive; None = all zero."""
        if t0 is None:
            self._chk(self._L.gtop_set_start_times_device(self._h, 0, None))
            self._t0_keep = None
            return
        pt0 = self._dev("t0", t0, t0.numel())
        self._t0_keep = t0
        self._chk(self._L.gtop_set_start_times_device(self._h, t0.numel(), pt0))

    def edt_query(self, pos, time):
        """(dist (N,), grad (N, 3)) at pos (N, 3), time (N,); time < 0 = static field only."""
        pos = _f64(pos).reshape(-1, 3)
        time = _f64(np.broadcast_to(time, (pos.shape[0],)))
        dist = np.empty(pos.shape[0])
        grad = np.empty((pos.shape[0], 3))
        self._chk(self._L.gtop_edt_query(self._h, pos.shape[0], _p(pos), _p(time), _p(dist), _p(grad)))
        return dist, grad

    def edt_coarse_query(self, pos, time):
        """EDTEnvironment::evaluateCoarseEDT: dist (N,) at pos (N, 3), time (N,); time < 0 = static field only."""
        pos = _f64(pos).reshape(-1, 3)
        time = _f64(np.broadcast_to(time, (pos.shape[0],)))
        dist = np.empty(pos.shape[0])
        self._chk(self._L.gtop_edt_coarse_query(self._h, pos.shape[0], _p(pos), _p(time), _p(dist)))
        return dist

    def edt_query_device(self, pos, time, stream=None):
        """torch fp64 CUDA tensors pos (N, 3), time (N,) -> dist (N,), grad (N, 3); asynchronous."""
        if pos.dim() != 2 or pos.shape[1] != 3:
            raise ValueError(f"pos: expected shape (N, 3), got {tuple(pos.shape)}")
        N = pos.shape[0]
        ppos, ptime = self._dev("pos", pos, N * 3), self._dev("time", time, N)
        dist, pdist = self._out("dist", None, (N,), pos)
        grad, pgrad = self._out("grad", None, (N, 3), pos)
        self._chk(self._L.gtop_edt_query_device(self._h, N, ppos, ptime, pdist, pgrad, _stream(stream, pos)))
        return dist, grad

    def edt_coarse_query_device(self, pos, time, stream=None):
        """torch fp64 CUDA tensors pos (N, 3), time (N,) -> dist (N,): edt_coarse_query on the device; asynchronous."""
        if pos.dim() != 2 or pos.shape[1] != 3:
            raise ValueError(f"pos: expected shape (N, 3), got {tuple(pos.shape)}")
        N = pos.shape[0]
        ppos, ptime = self._dev("pos", pos, N * 3), self._dev("time", time, N)
        dist, pdist = self._out("dist", None, (N,), pos)
        self._chk(self._L.gtop_edt_coarse_query_device(self._h, N, ppos, ptime, pdist, _stream(stream, pos)))
        return dist

    # -- trajectory safety report and best-candidate selection (include/gtop.h) --
    TRAJ_REPORT = ("n_samples", "clearance", "clearance_t", "clearance_index", "n_below_margin", "first_below_t",
                   "n_out_of_map", "max_vel_norm", "max_acc_norm", "max_vel_axis", "max_acc_axis", "time_sum")

    def validate_batch(self, x, limits, cost=None, dt_sample=0.01):
        """The report of the context's problem at free variables x (B, n) and, with `cost` (B,) given, the selection:
        (report (B, 12), pass (B,) bool, best (2,) int32 = [index of the passing row of least cost or -1, passing
        rows]); pass and best are None without cost."""
        x = _f64(x)
        B = x.shape[0]
        report = np.empty((B, len(self.TRAJ_REPORT)))
        if cost is None:
            self._chk(self._L.gtop_validate_batch(self._h, B, _p(x), float(dt_sample), C.byref(limits), None, _p(report),
                                                  None, None))
            return report, None, None
        cost = _f64(cost).reshape(-1)
        if cost.shape[0] != B:
            raise ValueError(f"cost: expected {B} entries, one per row of x, got {cost.shape[0]}")
        ok = np.zeros(B, dtype=np.uint8)
        best = np.zeros(2, dtype=np.int32)
        self._chk(self._L.gtop_validate_batch(self._h, B, _p(x), float(dt_sample), C.byref(limits), _p(cost), _p(report),
                                              ok.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                              best.ctypes.data_as(C.POINTER(C.c_int32))))
        return report, ok.astype(bool), best

    def coefficients_device(self, x, Df, T, coeff=None, stream=None):
        """torch fp64 CUDA tensors x (B, n), Df (B, 18), T (B, m) or (m,) -> coeff (B, m, 18); asynchronous."""
        prob = self._problem(x, Df, T)
        coeff, pcoeff = self._out("coeff", coeff, (*prob[:2], 18), x)
        self._chk(self._L.gtop_coefficients_device(self._h, *prob, pcoeff, _stream(stream, x)))
        return coeff

    def setup_paths_device(self, waypoints, mean_v=1.8, init_time=0.3, T=None, Df=None, x0=None, stream=None):
        """torch fp64 CUDA tensor waypoints (B, m+1, 3) -> T (B, m), Df (B, 18), x0 (B, 9(m-1)): setPath's segment
        times, fixed derivatives and straight-line free variables; asynchronous."""
        if waypoints.dim() != 3 or waypoints.shape[2] != 3:
            raise ValueError(f"waypoints: expected shape (B, m + 1, 3), got {tuple(waypoints.shape)}")
        B, m = waypoints.shape[0], waypoints.shape[1] - 1
        pwp = self._dev("waypoints", waypoints, B * (m + 1) * 3)
        T, pT = self._out("T", T, (B, m), waypoints)
        Df, pDf = self._out("Df", Df, (B, 18), waypoints)
        x0, px0 = self._out("x0", x0, (B, max(9 * (m - 1), 0)), waypoints)
        self._chk(self._L.gtop_setup_paths_device(self._h, B, m, pwp, float(mean_v), float(init_time), pT, pDf, px0,
                                                  _stream(stream, waypoints)))
        return T, Df, x0

    def eval_trajectories_device(self, coeff, T, dt_sample=0.01, stats=None, stream=None):
        """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> stats (B, 9), the columns of TRAJ_STATS;
        asynchronous."""
        traj = self._trajectory(coeff, T)
        stats, pstats = self._out("stats", stats, (traj[0], len(self.TRAJ_STATS)), coeff)
        self._chk(self._L.gtop_eval_trajectories_device(self._h, *traj, float(dt_sample), pstats,
                                                        _stream(stream, coeff)))
        return stats

    def sample_trajectories_device(self, coeff, T, dt_sample=0.01, max_samples=4096, stats=None, samples=None,
                                   stream=None):
        """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> (stats (B, 9), samples (B, max_samples, 3)):
        the getTraj points; trajectory b has stats[b, 8] of them, the first max_samples are stored and the rows behind
        them are left as they were (zero in a buffer allocated here); asynchronous."""
        traj = self._trajectory(coeff, T)
        max_samples = int(max_samples)
        stats, pstats = self._out("stats", stats, (traj[0], len(self.TRAJ_STATS)), coeff)
        samples, psamples = self._out("samples", samples, (traj[0], max(max_samples, 0), 3), coeff, make="zeros")
        self._chk(self._L.gtop_sample_trajectories_device(self._h, *traj, float(dt_sample), pstats, psamples,
                                                          max_samples, _stream(stream, coeff)))
        return stats, samples

    def validate_device(self, coeff, T, limits, dt_sample=0.01, report=None, stream=None):
        """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> report (B, 12); asynchronous, capturable
        (pass `report` to write into a buffer of the caller's)."""
        traj = self._trajectory(coeff, T)
        report, preport = self._out("report", report, (traj[0], len(self.TRAJ_REPORT)), coeff)
        self._chk(self._L.gtop_validate_trajectories_device(self._h, *traj, float(dt_sample), C.byref(limits), preport,
                                                            _stream(stream, coeff)))
        return report

    def select_best_device(self, report, cost, limits, want_pass=True, best=None, stream=None):
        """report (B, 12), cost (B,) torch fp64 CUDA tensors -> (pass (B,) uint8 or None, best (2,) int32);
        asynchronous, capturable."""
        B = cost.numel()
        preport, pcost = self._dev("report", report, B * len(self.TRAJ_REPORT)), self._dev("cost", cost, B)
        ok, pok = self._out("pass", None, (B,), report, _th().uint8) if want_pass else (None, None)
        best, pbest = self._out("best", best, (2,), report, _th().int32)
        self._chk(self._L.gtop_select_best_device(self._h, B, preport, pcost, C.byref(limits), pok, pbest,
                                                  _stream(stream, report)))
        return ok, best

    # -- per-segment report and segment-time reallocation (include/gtop.h) --
    SEG_REPORT = ("n_samples", "first_sample", "clearance", "clearance_t", "n_below_margin", "n_out_of_map",
                  "max_vel_norm", "max_acc_norm", "max_vel_axis", "max_acc_axis")

    def validate_segments(self, x, limits, dt_sample=0.01):
        """The per-segment report (B, m, 10) of the context's problem at free variables x (B, n): the samples and
        distances of validate_batch, reduced per segment (the columns of SEG_REPORT)."""
        x = _f64(x)
        B = x.shape[0]
        seg = np.empty((B, self.m, len(self.SEG_REPORT)))
        self._chk(self._L.gtop_validate_segments(self._h, B, _p(x), float(dt_sample), C.byref(limits), _p(seg)))
        return seg

    def validate_segments_device(self, coeff, T, limits, dt_sample=0.01, seg_report=None, stream=None):
        """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> seg_report (B, m, 10); asynchronous,
        capturable (pass `seg_report` to write into a buffer of the caller's)."""
        traj = self._trajectory(coeff, T)
        seg_report, pseg = self._out("seg_report", seg_report, (*traj[:2], len(self.SEG_REPORT)), coeff)
        self._chk(self._L.gtop_validate_segments_device(self._h, *traj, float(dt_sample), C.byref(limits), pseg,
                                                        _stream(stream, coeff)))
        return seg_report

    def reallocate_times(self, x, options, limits=None, dt_sample=0.01):
        """New segment times (B, m) for the first B rows of the context's problem at free variables x (B, n), by
        `options` (a GtopRetime).  LIMITS forms the segment report itself from `limits` and dt_sample; LENGTH ignores
        both.  Returns (T_out, x): x is a copy, rescaled under scale_x.  The context's problem is not changed: pass
        T_out to set_problem."""
        x = _f64(x).copy()
        B = x.shape[0]
        T_out = np.empty((B, self.m))
        if limits is None:
            limits = GtopLimits()
        self._chk(self._L.gtop_reallocate_times(self._h, C.byref(options), B, _p(x), float(dt_sample), C.byref(limits),
                                                _p(T_out)))
        return T_out, x

    def reallocate_times_device(self, options, x=None, Df=None, T=None, seg_report=None, T_out=None, stream=None):
        """torch fp64 CUDA tensors -> T_out (B, m); asynchronous, capturable.  LENGTH reads x (B, n) and Df (B, 18);
        LIMITS reads T (B, m) or (m,) and seg_report (B, m, 10) and, under scale_x, rescales x in place.  T_out may be
        T itself when T is (B, m)."""
        first = x if x is not None else seg_report
        if first is None or first.dim() < 2:
            raise ValueError("x or seg_report: expected x (B, n) or seg_report (B, m, 10)")
        B, m = (x.shape[0], x.shape[1] // 9 + 1) if x is not None else seg_report.shape[:2]
        # the library refuses a buffer that the mode reads and that is absent; one that is given is held to its size
        px, pDf, pseg = (None if t is None else self._dev(name, t, count) for name, t, count in
                         (("x", x, B * 9 * (m - 1)), ("Df", Df, B * 18), ("seg_report", seg_report, B * m * 10)))
        pT, stride = (None, m) if T is None else self._times(T, B, m)
        T_out, pT_out = self._out("T_out", T_out, (B, m), first)
        self._chk(self._L.gtop_reallocate_times_device(self._h, C.byref(options), B, m, px, pDf, pT, stride, pseg,
                                                       pT_out, _stream(stream, first)))
        return T_out

    # -- batched optimizer --
    @staticmethod
    def default_bounds(waypoints, bos=3.0, vos=8.0, aos=10.0):
        """(B, m+1, 3) waypoints -> lb, ub of shape (B, n) (opti_node.launch bos/vos/aos)."""
        wp = _f64(waypoints)
        B, npts, _ = wp.shape
        m = npts - 1
        lb = np.empty((B, 9 * (m - 1)))
        ub = np.empty_like(lb)
        rc = load_library().gtop_default_bounds(B, m, _p(wp), bos, vos, aos, _p(lb), _p(ub))
        if rc != 0:
            raise GtopError(rc, "gtop_default_bounds")
        return lb, ub

    def optimize_batch(self, x0, lb, ub, max_evals):
        """Host arrays; returns (best x, its cost) for the problem of set_problem."""
        x = _f64(x0).copy()
        B = x.shape[0]
        lb, ub = _f64(lb), _f64(ub)
        if not (lb.shape == x.shape == ub.shape):
            raise ValueError(f"lb, ub: expected the shape of x0, {x.shape}")
        cost = np.empty(B)
        self._chk(self._L.gtop_optimize_batch(self._h, B, _p(x), _p(lb), _p(ub), int(max_evals), _p(cost)))
        return x, cost

    def _bounded_problem(self, x, Df, T, lb, ub):
        """The optimizer's run of arguments: the problem triple, then lb and ub of B n elements each."""
        prob = self._problem(x, Df, T)
        return (*prob, self._dev("lb", lb, x.numel()), self._dev("ub", ub, x.numel()))

    def optimize_device_ex(self, x, Df, T, lb, ub, max_evals, ftol_rel=0.0, xtol_rel=0.0, maxtime=0.0, stream=None):
        """torch fp64 CUDA tensors; x is overwritten with the best point; returns (x, min_cost, nevals, code)."""
        args = self._bounded_problem(x, Df, T, lb, ub)
        min_cost, pcost = self._out("min_cost", None, (args[0],), x)
        nev, pnev = self._out("nevals", None, (args[0],), x, _th().int32)
        code, pcode = self._out("code", None, (args[0],), x, _th().int32)
        stop = GtopStop(int(max_evals), float(ftol_rel), float(xtol_rel), float(maxtime))
        self._chk(self._L.gtop_optimize_device_ex(self._h, *args, C.byref(stop), pcost, pnev, pcode, _stream(stream, x)))
        return x, min_cost, nev, code

    def optimize_device(self, x, Df, T, lb, ub, max_evals, min_cost=None, stream=None):
        """torch fp64 CUDA tensors; x is overwritten with the best point."""
        args = self._bounded_problem(x, Df, T, lb, ub)
        min_cost, pcost = self._out("min_cost", min_cost, (args[0],), x)
        self._chk(self._L.gtop_optimize_device(self._h, *args, int(max_evals), pcost, _stream(stream, x)))
        return x, min_cost

    # -- bookkeeping --
    def stats(self):
        it = C.c_int64()
        tt = C.c_double()
        self._chk(self._L.gtop_get_stats(self._h, C.byref(it), C.byref(tt)))
        return it.value, tt.value

    def reset_stats(self):
        self._chk(self._L.gtop_reset_stats(self._h))

    def cost_curve(self):
        cnt = C.c_int()
        self._chk(self._L.gtop_get_cost_curve(self._h, None, None, 0, C.byref(cnt)))
        c = np.empty(cnt.value)
        t = np.empty(cnt.value)
        if cnt.value:
            self._chk(self._L.gtop_get_cost_curve(self._h, _p(c), _p(t), cnt.value, C.byref(cnt)))
        return c, t

    def clear_cost_curve(self):
        self._chk(self._L.gtop_clear_cost_curve(self._h))


class Rendezvous(_Handle):
    """N serial callers sharing one launch (include/gtop.h, gtop_rendezvous_*).  The context's problem must hold
    the N trajectories (row i = caller i).  Each caller thread uses `cost(i, x)` as its objective and calls
    `leave(i)` when its optimizer has returned."""
    _prefix = "gtop_rendezvous_"    # no last_error of its own: errors are read from the context

    def __init__(self, ctx, n_slots, m):
        self._L = load_library()
        self._ctx = ctx
        h = C.c_void_p()
        rc = self._L.gtop_rendezvous_create(C.byref(h), ctx._h, int(n_slots), int(m))
        if rc != 0:
            raise GtopError(rc, "gtop_rendezvous_create")
        self._h = h
        self.n = 9 * (m - 1)
        self._slots = [C.c_void_p(self._L.gtop_rendezvous_get_slot(h, i)) for i in range(n_slots)]

    def cost(self, i, x, want_grad=True):
        x = _f64(x)
        g = np.empty_like(x) if want_grad else None
        c = self._L.gtop_cost_nlopt_shared(x.size, _p(x), _p(g) if want_grad else None, self._slots[i])
        if not np.isfinite(c):
            raise GtopError(1, "gtop_cost_nlopt_shared: " + self._L.gtop_last_error(self._ctx._h).decode())
        return c, g

    def leave(self, i):
        return self._L.gtop_rendezvous_leave(self._slots[i])

    def set_timeout(self, seconds):
        """Longest a caller waits for the others; past it the rendezvous breaks for everybody (0 = for ever)."""
        self._L.gtop_rendezvous_set_timeout(self._h, float(seconds))

    def abort(self):
        """Wake every caller; all calls return an error from now on."""
        self._L.gtop_rendezvous_abort(self._h)

    def stats(self):
        n, cb, s = C.c_int64(), C.c_int64(), C.c_double()
        self._L.gtop_rendezvous_stats(self._h, C.byref(n), C.byref(s), C.byref(cb))
        return dict(launches=n.value, launch_seconds=s.value, callbacks=cb.value)


class GtopGroup(_HostProblem):
    """One batch over several devices from one process (include/gtop.h, gtop_group_*): the field replicated, the
    batch in contiguous slices, every slice launched on its own device, results gathered on the host or all-gathered
    on the devices (RCCL when the devices differ, peer copies otherwise)."""
    _prefix = "gtop_group_"

    def __init__(self, devices, params=None):
        self._L = load_library()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._L.gtop_group_create(C.byref(h), devs, len(devices))
        if rc != 0:
            raise GtopError(rc, self._L.gtop_group_last_error(None).decode())
        self._h = h
        self.devices = [int(d) for d in devices]
        self.set_params(**(params or {}))

    @property
    def gather_backend(self):
        return self._L.gtop_group_gather_backend(self._h).decode()

    def gather_note(self):
        """The backend and why: a fallback from RCCL to peer copies names its reason."""
        return self._L.gtop_group_gather_note(self._h).decode()

    def set_gradient_mode(self, consistent=True):
        """GtopContext.set_gradient_mode on every member."""
        self._chk(self._L.gtop_group_set_gradient_mode(self._h, 1 if consistent else 0))

    def set_field_sign(self, signed=True, max_depth=0.0):
        """GtopContext.set_field_sign on every member."""
        self._chk(self._L.gtop_group_set_field_sign(self._h, 1 if signed else 0, float(max_depth)))

    def init_sdf_map(self, map_size, origin, resolution):
        self._chk(self._L.gtop_group_init_sdf_map(self._h, _p(_f64(map_size)), _p(_f64(origin)), float(resolution)))

    def update_sdf_map(self, pts):
        pts = _f64(pts).reshape(-1, 3)
        self._chk(self._L.gtop_group_update_sdf_map(self._h, _p(pts), pts.shape[0]))

    def update_sdf_map_window(self, min_pos, max_pos, pts):
        pts = _f64(pts).reshape(-1, 3)
        mn, mx = _f64(min_pos).reshape(3), _f64(max_pos).reshape(3)
        self._chk(self._L.gtop_group_update_sdf_map_window(self._h, _p(mn), _p(mx), _p(pts) if pts.size else None, pts.shape[0]))

    def shards(self):
        out = []
        for i in range(len(self.devices)):
            a, b = C.c_int(), C.c_int()
            self._chk(self._L.gtop_group_shard(self._h, i, C.byref(a), C.byref(b)))
            out.append((a.value, b.value))
        return out

    def eval_batch(self, x):
        x = _f64(x)
        B, n = x.shape
        cost = np.empty(B)
        grad = np.empty((B, n))
        self._chk(self._L.gtop_group_eval_batch(self._h, B, _p(x), _p(cost), _p(grad)))
        return cost, grad

    def eval_resident(self, x=None, gather=1):
        """Evaluate the resident slices (x uploaded first when given) and all-gather on the devices; returns, per
        member, the gathered (cost, grad) as that device holds them (grad None unless gather == 2)."""
        if x is not None:
            x = _f64(x)
            self._chk(self._L.gtop_group_upload_x(self._h, x.shape[0], _p(x)))
        self._chk(self._L.gtop_group_eval_resident(self._h, int(gather), 1))
        n = 9 * (self.m - 1)
        out = []
        for i in range(len(self.devices)):
            c = np.empty(self.B)
            g = np.empty((self.B, n)) if gather == 2 else None
            self._chk(self._L.gtop_group_read_gathered(self._h, i, _p(c), _p(g) if g is not None else None))
            out.append((c, g))
        return out

    def set_launch_geometry(self, waves=0, samples_per_lane=0):
        """gtop_set_launch_geometry on every member's context (pins the kernel body: a slice and the whole batch then
        sum in the same order whatever their sizes)."""
        for i in range(len(self.devices)):
            ctx = C.c_void_p(self._L.gtop_group_context(self._h, i))
            rc = self._L.gtop_set_launch_geometry(ctx, int(waves), int(samples_per_lane))
            if rc != 0:
                raise GtopError(rc, self._L.gtop_last_error(ctx).decode())

    def launch_resident(self, x=None, gather=1):
        """eval_resident without waiting: the slices' evaluations and the all-gather are only ENQUEUED on the members'
        streams (gtop_group_eval_resident(synchronize = 0)); read the results with read_gathered() after synchronize()."""
        if x is not None:
            x = _f64(x)
            self._chk(self._L.gtop_group_upload_x(self._h, x.shape[0], _p(x)))
        self._chk(self._L.gtop_group_eval_resident(self._h, int(gather), 0))

    def synchronize(self):
        self._chk(self._L.gtop_group_synchronize(self._h))

    def read_gathered(self, member, grads=False):
        n = 9 * (self.m - 1)
        c = np.empty(self.B)
        g = np.empty((self.B, n)) if grads else None
        self._chk(self._L.gtop_group_read_gathered(self._h, int(member), _p(c), _p(g) if grads else None))
        return c, g
