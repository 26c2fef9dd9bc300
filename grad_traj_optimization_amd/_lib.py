"""ctypes binding of include/gtop.h (the C-ABI of libgtop_hip.so)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GTOP_HIP_LIB selects another build of the same C-ABI (kernel tuning variants)
_SO = os.environ.get("GTOP_HIP_LIB") or os.path.join(_HERE, "libgtop_hip.so")

GTOP_F64, GTOP_F32 = 0, 1
_STATUS = {0: "GTOP_OK", 1: "GTOP_ERR_INVALID", 2: "GTOP_ERR_HIP", 3: "GTOP_ERR_NO_DEVICE",
           4: "GTOP_ERR_STATE"}


class GtopError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"{_STATUS.get(code, code)}: {msg}")


class GtopParams(C.Structure):
    """gtop_params — the ROS parameters the callback reads
    (src/grad_traj_optimizer.cpp:5-32 of the reference) + step + enable_dyn."""
    _fields_ = [
        ("ws", C.c_double), ("wc", C.c_double),
        ("alpha", C.c_double), ("r", C.c_double), ("d0", C.c_double),
        ("alpha_v", C.c_double), ("r_v", C.c_double), ("v0", C.c_double),
        ("alpha_a", C.c_double), ("r_a", C.c_double), ("a0", C.c_double),
        ("step", C.c_int32), ("enable_dyn", C.c_int32),
    ]


class GtopStop(C.Structure):
    """gtop_stop — evaluation cap + NLopt's ftol_rel / xtol_rel / maxtime."""
    _fields_ = [("max_evals", C.c_int32), ("ftol_rel", C.c_double), ("xtol_rel", C.c_double), ("maxtime", C.c_double)]


# launch/opti_node.launch:3-28 of the reference — the only parameter set whose
# names match what the ctor reads.
OPTI_NODE_PARAMS = dict(ws=1.0, wc=5.0, alpha=10.0, r=0.5, d0=0.8,
                        alpha_v=0.0, r_v=1.5, v0=2.5, alpha_a=0.0, r_a=1.5, a0=3.5,
                        step=2, enable_dyn=0)

_lib = None


class GtopLimits(C.Structure):
    """gtop_limits of include/gtop.h: what a trajectory must keep to pass (validate_batch / select_best_device)."""
    _fields_ = [("margin", C.c_double), ("max_vel", C.c_double), ("max_acc", C.c_double), ("per_axis", C.c_int32),
                ("allow_out_of_map", C.c_int32), ("use_boxes", C.c_int32)]

    def __init__(self, margin=0.0, max_vel=0.0, max_acc=0.0, per_axis=False, allow_out_of_map=False, use_boxes=False):
        super().__init__(float(margin), float(max_vel), float(max_acc), int(bool(per_axis)), int(bool(allow_out_of_map)),
                         int(bool(use_boxes)))


class GtopRetime(C.Structure):
    """gtop_retime of include/gtop.h: how reallocate_times[_device] forms the new segment times.  mode 0 (LENGTH):
    length / mean_v of the waypoints as they stand in x, init_time on the first and last segment; mode 1 (LIMITS): the
    segments whose figure in the segment report breaks max_vel / max_acc are stretched."""
    LENGTH, LIMITS = 0, 1
    _fields_ = [("mode", C.c_int32), ("mean_v", C.c_double), ("init_time", C.c_double), ("max_vel", C.c_double),
                ("max_acc", C.c_double), ("per_axis", C.c_int32), ("uniform", C.c_int32), ("scale_x", C.c_int32),
                ("max_ratio", C.c_double)]

    def __init__(self, mode=0, mean_v=1.8, init_time=0.3, max_vel=0.0, max_acc=0.0, per_axis=False, uniform=False,
                 scale_x=False, max_ratio=4.0):
        super().__init__(int(mode), float(mean_v), float(init_time), float(max_vel), float(max_acc), int(bool(per_axis)),
                         int(bool(uniform)), int(bool(scale_x)), float(max_ratio))


def library_path():
    return _SO


def _preload_torch_hip_runtime():
    """One process must hold ONE HIP runtime.  The PyTorch-ROCm wheel bundles
    its own libamdhip64.so (SONAME libamdhip64.so.7, the name libgtop_hip.so
    needs): if libgtop_hip.so were loaded first it would pull /opt/rocm's copy,
    a later `import torch` would add the bundled one, and whichever initialises
    second sees "no ROCm-capable device".  So when torch is installed, map its
    copy first (by path, without importing torch); the loader then resolves our
    NEEDED entry to it by SONAME, and torch finds it already loaded."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library():
    """Load libgtop_hip.so.  Raises (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(
            f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C grad_traj_optimization_amd/csrc` — there is no CPU fallback")
    _preload_torch_hip_runtime()
    L = C.CDLL(_SO)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    sig = {
        "gtop_abi_version": (C.c_int, []),
        "gtop_create": (C.c_int, [C.POINTER(vp), C.c_int]),
        "gtop_destroy": (C.c_int, [vp]),
        "gtop_last_error": (C.c_char_p, [vp]),
        "gtop_set_params": (C.c_int, [vp, C.POINTER(GtopParams)]),
        "gtop_set_sdf": (C.c_int, [vp, dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double]),
        "gtop_set_sdf_device": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double]),
        "gtop_init_sdf_map": (C.c_int, [vp, dp, dp, C.c_double]),
        "gtop_update_sdf_map": (C.c_int, [vp, dp, C.c_int]),
        "gtop_update_sdf_map_device": (C.c_int, [vp, vp, C.c_int, vp]),
        "gtop_get_sdf": (C.c_int, [vp, dp, ip]),
        "gtop_set_problem": (C.c_int, [vp, C.c_int, C.c_int, dp, C.c_int, dp]),
        "gtop_eval_batch": (C.c_int, [vp, C.c_int, dp, dp, dp]),
        "gtop_cost_nlopt": (C.c_double, [C.c_uint, dp, dp, vp]),
        "gtop_eval_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]),
        "gtop_set_paths": (C.c_int, [vp, C.c_int, C.c_int, dp, C.c_double, C.c_double, dp]),
        "gtop_setup_paths_device": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_double, C.c_double, vp, vp, vp, vp]),
        "gtop_get_problem": (C.c_int, [vp, dp, dp]),
        "gtop_min_jerk_start_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
        "gtop_min_jerk_start": (C.c_int, [vp, C.c_int, dp]),
        "gtop_coefficients_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]),
        "gtop_eval_trajectories_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_double, vp, vp]),
        "gtop_trajectory_stats": (C.c_int, [vp, C.c_int, dp, C.c_double, dp, dp]),
        "gtop_set_moving_boxes": (C.c_int, [vp, C.c_int, dp, dp, dp]),
        "gtop_set_moving_box_polynomials": (C.c_int, [vp, C.c_int, dp, dp, dp]),
        "gtop_get_moving_box_kind": (C.c_int, [vp, ip, ip]),
        "gtop_box_polynomial_centres": (C.c_int, [C.c_int, dp, dp, C.c_int, dp, dp]),
        "gtop_set_moving_cost": (C.c_int, [vp, C.c_int]),
        "gtop_get_moving_cost": (C.c_int, [vp, ip]),
        "gtop_set_gradient_mode": (C.c_int, [vp, C.c_int]),
        "gtop_get_gradient_mode": (C.c_int, [vp, ip]),
        "gtop_group_set_gradient_mode": (C.c_int, [vp, C.c_int]),
        "gtop_set_start_times": (C.c_int, [vp, C.c_int, dp]),
        "gtop_set_start_times_device": (C.c_int, [vp, C.c_int, vp]),
        "gtop_edt_query_device": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp]),
        "gtop_edt_query": (C.c_int, [vp, C.c_int, dp, dp, dp, dp]),
        "gtop_edt_coarse_query_device": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        "gtop_edt_coarse_query": (C.c_int, [vp, C.c_int, dp, dp, dp]),
        "gtop_sample_trajectories_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_double, vp, vp, C.c_int, vp]),
        "gtop_trajectory_samples": (C.c_int, [vp, C.c_int, dp, C.c_double, dp, dp, dp, C.c_int]),
        "gtop_validate_trajectories_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_double,
                                                        C.POINTER(GtopLimits), vp, vp]),
        "gtop_select_best_device": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(GtopLimits), vp, vp, vp]),
        "gtop_validate_batch": (C.c_int, [vp, C.c_int, dp, C.c_double, C.POINTER(GtopLimits), dp, dp,
                                          C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)]),
        "gtop_validate_segments_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_double,
                                                    C.POINTER(GtopLimits), vp, vp]),
        "gtop_validate_segments": (C.c_int, [vp, C.c_int, dp, C.c_double, C.POINTER(GtopLimits), dp]),
        "gtop_reallocate_times_device": (C.c_int, [vp, C.POINTER(GtopRetime), C.c_int, C.c_int, vp, vp, vp, C.c_int, vp,
                                                   vp, vp]),
        "gtop_reallocate_times": (C.c_int, [vp, C.POINTER(GtopRetime), C.c_int, dp, C.c_double, C.POINTER(GtopLimits),
                                            dp]),
        "gtop_default_bounds": (C.c_int, [C.c_int, C.c_int, dp, C.c_double, C.c_double, C.c_double, dp, dp]),
        "gtop_optimize_batch": (C.c_int, [vp, C.c_int, dp, dp, dp, C.c_int, dp]),
        "gtop_optimize_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]),
        "gtop_optimize_batch_ex": (C.c_int, [vp, C.c_int, dp, dp, dp, C.POINTER(GtopStop), dp, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]),
        "gtop_optimize_device_ex": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.POINTER(GtopStop), vp,
                                              vp, vp, vp]),
        "gtop_get_stats": (C.c_int, [vp, C.POINTER(C.c_int64), dp]),
        "gtop_reset_stats": (C.c_int, [vp]),
        "gtop_get_cost_curve": (C.c_int, [vp, dp, dp, C.c_int, ip]),
        "gtop_clear_cost_curve": (C.c_int, [vp]),
        "gtop_set_launch_geometry": (C.c_int, [vp, C.c_int, C.c_int]),
        "gtop_update_sdf_map_window": (C.c_int, [vp, dp, dp, dp, C.c_int]),
        "gtop_update_sdf_map_window_device": (C.c_int, [vp, dp, dp, vp, C.c_int, vp]),
        "gtop_set_field_precisions": (C.c_int, [vp, C.c_int]),
        "gtop_set_field_sign": (C.c_int, [vp, C.c_int, C.c_double]),
        "gtop_get_field_sign": (C.c_int, [vp, ip, dp]),
        "gtop_group_set_field_sign": (C.c_int, [vp, C.c_int, C.c_double]),
        "gtop_device_clock_stamp": (C.c_int, [vp, vp, vp]),
        "gtop_push_rows": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_void_p), C.c_int, vp, vp]),
        "gtop_shared_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(C.c_void_p), C.c_char_p]),
        "gtop_shared_open": (C.c_int, [vp, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
        "gtop_shared_close": (C.c_int, [vp, vp]),
        "gtop_shared_free": (C.c_int, [vp, vp]),
        "gtop_device_clock_hz": (C.c_int, [vp, dp]),
        "gtop_rendezvous_create": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int]),
        "gtop_rendezvous_destroy": (C.c_int, [vp]),
        "gtop_rendezvous_get_slot": (vp, [vp, C.c_int]),
        "gtop_cost_nlopt_shared": (C.c_double, [C.c_uint, dp, dp, vp]),
        "gtop_rendezvous_leave": (C.c_int, [vp]),
        "gtop_rendezvous_set_timeout": (C.c_int, [vp, C.c_double]),
        "gtop_rendezvous_abort": (C.c_int, [vp]),
        "gtop_rendezvous_stats": (C.c_int, [vp, C.POINTER(C.c_int64), dp, C.POINTER(C.c_int64)]),
        "gtop_set_optimizer_fusion": (C.c_int, [vp, C.c_int]),
        "gtop_set_optimizer_precision": (C.c_int, [vp, C.c_int]),
        "gtop_group_create": (C.c_int, [C.POINTER(vp), ip, C.c_int]),
        "gtop_group_destroy": (C.c_int, [vp]),
        "gtop_group_size": (C.c_int, [vp]),
        "gtop_group_context": (vp, [vp, C.c_int]),
        "gtop_group_last_error": (C.c_char_p, [vp]),
        "gtop_group_gather_backend": (C.c_char_p, [vp]),
        "gtop_group_gather_note": (C.c_char_p, [vp]),
        "gtop_group_update_sdf_map_window": (C.c_int, [vp, dp, dp, dp, C.c_int]),
        "gtop_group_set_params": (C.c_int, [vp, C.POINTER(GtopParams)]),
        "gtop_group_init_sdf_map": (C.c_int, [vp, dp, dp, C.c_double]),
        "gtop_group_update_sdf_map": (C.c_int, [vp, dp, C.c_int]),
        "gtop_group_set_sdf": (C.c_int, [vp, dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double]),
        "gtop_group_set_problem": (C.c_int, [vp, C.c_int, C.c_int, dp, C.c_int, dp]),
        "gtop_group_shard": (C.c_int, [vp, C.c_int, ip, ip]),
        "gtop_group_eval_batch": (C.c_int, [vp, C.c_int, dp, dp, dp]),
        "gtop_group_upload_x": (C.c_int, [vp, C.c_int, dp]),
        "gtop_group_eval_resident": (C.c_int, [vp, C.c_int, C.c_int]),
        "gtop_group_synchronize": (C.c_int, [vp]),
        "gtop_group_read_gathered": (C.c_int, [vp, C.c_int, dp, dp]),
        "gtop_group_device_buffers": (C.c_int, [vp, C.c_int] + [C.POINTER(vp)] * 6),
        "gtop_group_optimize_batch_ex": (C.c_int, [vp, C.c_int, dp, dp, dp, C.POINTER(GtopStop), dp, C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32)]),
    }
    # An OLDER build chosen through GTOP_HIP_LIB (A/B timing against a parent commit) lacks the entry points of a later
    # ABI version: those stay unbound there (calling one raises AttributeError); the in-tree library must have them all.
    since = {"gtop_set_moving_cost": 4, "gtop_get_moving_cost": 4, "gtop_set_start_times": 4,
             "gtop_set_start_times_device": 4, "gtop_validate_trajectories_device": 5, "gtop_select_best_device": 5,
             "gtop_validate_batch": 5, "gtop_set_gradient_mode": 6, "gtop_get_gradient_mode": 6,
             "gtop_group_set_gradient_mode": 6, "gtop_set_moving_box_polynomials": 7, "gtop_get_moving_box_kind": 7,
             "gtop_box_polynomial_centres": 7, "gtop_min_jerk_start_device": 8, "gtop_min_jerk_start": 8,
             "gtop_validate_segments_device": 9, "gtop_validate_segments": 9, "gtop_reallocate_times_device": 9,
             "gtop_reallocate_times": 9}
    L.gtop_abi_version.restype = C.c_int
    abi = L.gtop_abi_version() if os.environ.get("GTOP_HIP_LIB") else max(since.values())
    for name, (res, args) in sig.items():
        if since.get(name, 0) > abi:
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def box_polynomial_centres(coef, times, t_range=None):
    """Centres (ntimes, nbox, 3) of polynomial boxes at `times`, by the arithmetic every kernel uses (the clamp into
    [t1, t2], then Horner in fp64 fmas; include/gtop.h, gtop_box_polynomial_centres).  Host only: no context, no GPU."""
    L = load_library()
    coef = _f64(coef).reshape(-1, 3, 6)
    times = _f64(np.atleast_1d(times)).reshape(-1)
    tr = None
    if t_range is not None:
        tr = _f64(t_range).reshape(-1, 2)
        assert tr.shape[0] == coef.shape[0]
    out = np.empty((times.shape[0], coef.shape[0], 3))
    rc = L.gtop_box_polynomial_centres(coef.shape[0], _p(coef), None if tr is None else _p(tr), times.shape[0], _p(times),
                                       _p(out))
    if rc != 0:
        raise GtopError(rc, "box_polynomial_centres: bad arguments (a non-finite coefficient, t1 > t2, a NaN bound)")
    return out


class GtopContext:
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

    # -- helpers --
    def _chk(self, rc):
        if rc != 0:
            raise GtopError(rc, self._L.gtop_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.gtop_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration --
    def set_params(self, **kw):
        d = dict(OPTI_NODE_PARAMS)
        d.update(kw)
        self.params = d
        p = GtopParams(**d)
        self._chk(self._L.gtop_set_params(self._h, C.byref(p)))

    def set_sdf(self, dist, grid, origin, resolution, map_size=None):
        dist = _f64(dist).reshape(-1)
        nx, ny, nz = (int(g) for g in grid)
        assert dist.size == nx * ny * nz
        ms = _p(_f64(map_size)) if map_size is not None else None
        self._chk(self._L.gtop_set_sdf(self._h, _p(dist), nx, ny, nz, _p(_f64(origin)), ms, float(resolution)))
        self.grid = (nx, ny, nz)

    def set_sdf_device(self, tensor, grid, origin, resolution, map_size=None):
        import torch
        dtype = {torch.float64: GTOP_F64, torch.float32: GTOP_F32}[tensor.dtype]
        nx, ny, nz = (int(g) for g in grid)
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == nx * ny * nz
        ms = _p(_f64(map_size)) if map_size is not None else None
        self._chk(self._L.gtop_set_sdf_device(self._h, dtype, C.c_void_p(tensor.data_ptr()), nx, ny, nz,
                                              _p(_f64(origin)), ms, float(resolution)))
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
        import torch
        assert pts.is_cuda and pts.dtype == torch.float64 and pts.dim() == 2 and pts.shape[1] == 3
        pts = pts.contiguous()   # (a tensor made from np.argwhere's transposed view is column-major)
        st = stream if stream is not None else torch.cuda.current_stream()
        self._chk(self._L.gtop_update_sdf_map_device(self._h, C.c_void_p(pts.data_ptr()), pts.shape[0],
                                                     C.c_void_p(st.cuda_stream)))

    def update_sdf_map_window(self, min_pos, max_pos, pts):
        """The reference's local update (compare2.cpp:147-152): resetBuffer(min, max), setOccupancy per point,
        updateESDF3d over the box (gtop_update_sdf_map_window)."""
        pts = _f64(pts).reshape(-1, 3)
        mn, mx = _f64(min_pos).reshape(3), _f64(max_pos).reshape(3)
        self._chk(self._L.gtop_update_sdf_map_window(self._h, _p(mn), _p(mx), _p(pts) if pts.size else None, pts.shape[0]))

    def update_sdf_map_window_device(self, min_pos, max_pos, pts, stream=None):
        import torch
        assert pts.is_cuda and pts.dtype == torch.float64 and pts.dim() == 2 and pts.shape[1] == 3
        pts = pts.contiguous()
        mn, mx = _f64(min_pos).reshape(3), _f64(max_pos).reshape(3)
        st = stream if stream is not None else torch.cuda.current_stream()
        self._chk(self._L.gtop_update_sdf_map_window_device(self._h, _p(mn), _p(mx), C.c_void_p(pts.data_ptr()),
                                                            pts.shape[0], C.c_void_p(st.cuda_stream)))

    def get_sdf(self):
        g = (C.c_int * 3)()
        self._chk(self._L.gtop_get_sdf(self._h, None, g))
        out = np.empty(g[0] * g[1] * g[2])
        self._chk(self._L.gtop_get_sdf(self._h, _p(out), g))
        return out.reshape(tuple(g))

    def set_problem(self, T, Df):
        Df = _f64(Df)
        B = Df.size // 18
        T = _f64(T)
        if T.ndim == 2:
            m, stride = T.shape[1], T.shape[1]
            assert T.shape[0] == B
        else:
            m, stride = T.shape[0], 0
        self._chk(self._L.gtop_set_problem(self._h, B, m, _p(T), stride, _p(Df)))
        self.B, self.m = B, m

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
        import torch
        dtype = {torch.float64: GTOP_F64, torch.float32: GTOP_F32}[x.dtype]
        B, n = x.shape
        m = n // 9 + 1
        assert n == 9 * (m - 1) and Df.numel() == B * 18
        stride = m if T.dim() == 2 else 0
        assert T.numel() == (B * m if stride else m)
        for t in (x, Df, T):
            assert t.is_cuda and t.is_contiguous() and t.dtype == x.dtype
        if cost is None:
            cost = torch.empty(B, dtype=x.dtype, device=x.device)
        if grad is None:
            grad = torch.empty(B, n, dtype=x.dtype, device=x.device)
        assert cost.is_contiguous() and grad.is_contiguous() and cost.numel() == B and grad.numel() == B * n
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        self._chk(self._L.gtop_eval_device(self._h, dtype, B, m, C.c_void_p(x.data_ptr()),
                                           C.c_void_p(Df.data_ptr()), C.c_void_p(T.data_ptr()), stride,
                                           C.c_void_p(cost.data_ptr()), C.c_void_p(grad.data_ptr()),
                                           C.c_void_p(stream)))
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
        import torch
        assert src.is_cuda and src.is_contiguous()
        if nbytes is None:
            nbytes = src.numel() * src.element_size()
        if stream is None:
            stream = torch.cuda.current_stream(src.device).cuda_stream
        arr = (C.c_void_p * len(dst_ptrs))(*[int(p) for p in dst_ptrs])
        self._chk(self._L.gtop_push_rows(self._h, C.c_void_p(src.data_ptr()), int(nbytes), arr, len(dst_ptrs),
                                         C.c_void_p(clock_minmax.data_ptr()) if clock_minmax is not None else None,
                                         C.c_void_p(stream)))

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
        import torch
        assert minmax.is_cuda and minmax.dtype == torch.int64 and minmax.numel() == 2 and minmax.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(minmax.device).cuda_stream
        self._chk(self._L.gtop_device_clock_stamp(self._h, C.c_void_p(minmax.data_ptr()), C.c_void_p(stream)))

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
        assert out.ndim == 2 and out.shape[1] == 9 * (self.m - 1)
        self._chk(self._L.gtop_min_jerk_start(self._h, out.shape[0], _p(out)))
        return out

    def min_jerk_start_device(self, x, Df, T, stream=None):
        """The same IN PLACE on a torch fp64 CUDA tensor x (B, n), with Df (B, 18) and T (B, m) or (m,): overwrites
        the velocity and acceleration entries of x; asynchronous, capturable.  Returns x."""
        import torch
        B, n = x.shape
        m = n // 9 + 1
        assert n == 9 * (m - 1) and Df.numel() == B * 18
        stride = m if T.dim() == 2 else 0
        assert T.numel() == (B * m if stride else m)
        for t in (x, Df, T):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        self._chk(self._L.gtop_min_jerk_start_device(self._h, B, m, C.c_void_p(x.data_ptr()), C.c_void_p(Df.data_ptr()),
                                                     C.c_void_p(T.data_ptr()), stride, C.c_void_p(stream)))
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
        assert p0.shape == vel.shape == scale.shape
        self._chk(self._L.gtop_set_moving_boxes(self._h, p0.shape[0], _p(p0), _p(vel), _p(scale)))

    BOXES_CONST_VEL, BOXES_POLYNOMIAL = 0, 1

    def set_moving_box_polynomials(self, coef, scale, t_range=None):
        """The box list as polynomial predictions (include/gtop.h, gtop_set_moving_box_polynomials): coef (nbox, 3, 6),
        axis-major, ascending powers; scale (nbox, 3); t_range (nbox, 2) = {t1, t2} per box, None = unbounded.  Outside
        [t1, t2] a box stands where its prediction ends.  Replaces whatever list was set, of either kind."""
        coef = _f64(coef).reshape(-1, 3, 6)
        scale = _f64(scale).reshape(-1, 3)
        assert coef.shape[0] == scale.shape[0]
        tr = None
        if t_range is not None:
            tr = _f64(t_range).reshape(-1, 2)
            assert tr.shape[0] == coef.shape[0]
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
        import torch
        assert t0.is_cuda and t0.dtype == torch.float64 and t0.is_contiguous()
        self._t0_keep = t0
        self._chk(self._L.gtop_set_start_times_device(self._h, t0.numel(), C.c_void_p(t0.data_ptr())))

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
        import torch
        assert pos.is_cuda and pos.dtype == torch.float64 and pos.is_contiguous() and time.is_contiguous()
        N = pos.shape[0]
        dist = torch.empty(N, dtype=torch.float64, device=pos.device)
        grad = torch.empty(N, 3, dtype=torch.float64, device=pos.device)
        if stream is None:
            stream = torch.cuda.current_stream(pos.device).cuda_stream
        self._chk(self._L.gtop_edt_query_device(self._h, N, C.c_void_p(pos.data_ptr()), C.c_void_p(time.data_ptr()),
                                                C.c_void_p(dist.data_ptr()), C.c_void_p(grad.data_ptr()),
                                                C.c_void_p(stream)))
        return dist, grad

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
        assert cost.shape[0] == B
        ok = np.zeros(B, dtype=np.uint8)
        best = np.zeros(2, dtype=np.int32)
        self._chk(self._L.gtop_validate_batch(self._h, B, _p(x), float(dt_sample), C.byref(limits), _p(cost), _p(report),
                                              ok.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                              best.ctypes.data_as(C.POINTER(C.c_int32))))
        return report, ok.astype(bool), best

    def coefficients_device(self, x, Df, T, coeff=None, stream=None):
        """torch fp64 CUDA tensors x (B, n), Df (B, 18), T (B, m) or (m,) -> coeff (B, m, 18); asynchronous."""
        import torch
        assert x.is_cuda and Df.is_cuda and T.is_cuda and x.dtype == Df.dtype == T.dtype == torch.float64
        assert x.is_contiguous() and Df.is_contiguous() and T.is_contiguous()
        B, m = x.shape[0], T.shape[-1]
        assert x.numel() == B * 9 * (m - 1) and Df.numel() == B * 18 and (T.dim() == 1 or T.shape == (B, m))
        if coeff is None:
            coeff = torch.empty(B, m, 18, dtype=torch.float64, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        self._chk(self._L.gtop_coefficients_device(self._h, B, m, C.c_void_p(x.data_ptr()), C.c_void_p(Df.data_ptr()),
                                                   C.c_void_p(T.data_ptr()), m if T.dim() == 2 else 0,
                                                   C.c_void_p(coeff.data_ptr()), C.c_void_p(stream)))
        return coeff

    def setup_paths_device(self, waypoints, mean_v=1.8, init_time=0.3, T=None, Df=None, x0=None, stream=None):
        """torch fp64 CUDA tensor waypoints (B, m+1, 3) -> T (B, m), Df (B, 18), x0 (B, 9(m-1)): setPath's segment
        times, fixed derivatives and straight-line free variables; asynchronous."""
        import torch
        assert waypoints.is_cuda and waypoints.dtype == torch.float64 and waypoints.is_contiguous()
        assert waypoints.dim() == 3 and waypoints.shape[2] == 3
        B, m = waypoints.shape[0], waypoints.shape[1] - 1
        n = 9 * (m - 1)
        if T is None:
            T = torch.empty(B, m, dtype=torch.float64, device=waypoints.device)
        if Df is None:
            Df = torch.empty(B, 18, dtype=torch.float64, device=waypoints.device)
        if x0 is None:
            x0 = torch.empty(B, max(n, 0), dtype=torch.float64, device=waypoints.device)
        for t, cnt in ((T, B * m), (Df, B * 18), (x0, B * n)):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == max(cnt, 0)
        if stream is None:
            stream = torch.cuda.current_stream(waypoints.device).cuda_stream
        self._chk(self._L.gtop_setup_paths_device(self._h, B, m, C.c_void_p(waypoints.data_ptr()), float(mean_v),
                                                  float(init_time), C.c_void_p(T.data_ptr()), C.c_void_p(Df.data_ptr()),
                                                  C.c_void_p(x0.data_ptr()), C.c_void_p(stream)))
        return T, Df, x0

    def eval_trajectories_device(self, coeff, T, dt_sample=0.01, stats=None, stream=None):
        """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> stats (B, 9), the columns of TRAJ_STATS;
        asynchronous."""
        import torch
        assert coeff.is_cuda and T.is_cuda and coeff.dtype == T.dtype == torch.float64
        assert coeff.is_contiguous() and T.is_contiguous() and coeff.dim() == 3 and coeff.shape[2] == 18
        B, m = coeff.shape[0], coeff.shape[1]
        assert T.shape == (m,) or T.shape == (B, m)
        if stats is None:
            stats = torch.empty(B, len(self.TRAJ_STATS), dtype=torch.float64, device=coeff.device)
        assert stats.is_cuda and stats.is_contiguous() and stats.dtype == torch.float64
        assert stats.numel() == B * len(self.TRAJ_STATS)
        if stream is None:
            stream = torch.cuda.current_stream(coeff.device).cuda_stream
        self._chk(self._L.gtop_eval_trajectories_device(self._h, B, m, C.c_void_p(coeff.data_ptr()),
                                                        C.c_void_p(T.data_ptr()), m if T.dim() == 2 else 0,
                                                        float(dt_sample), C.c_void_p(stats.data_ptr()),
                                                        C.c_void_p(stream)))
        return stats

    def sample_trajectories_device(self, coeff, T, dt_sample=0.01, max_samples=4096, stats=None, samples=None,
                                   stream=None):
        """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> (stats (B, 9), samples (B, max_samples, 3)):
        the getTraj points; trajectory b has stats[b, 8] of them, the first max_samples are stored and the rows behind
        them are left as they were (zero in a buffer allocated here); asynchronous."""
        import torch
        assert coeff.is_cuda and T.is_cuda and coeff.dtype == T.dtype == torch.float64
        assert coeff.is_contiguous() and T.is_contiguous() and coeff.dim() == 3 and coeff.shape[2] == 18
        B, m = coeff.shape[0], coeff.shape[1]
        assert T.shape == (m,) or T.shape == (B, m)
        max_samples = int(max_samples)
        if stats is None:
            stats = torch.empty(B, len(self.TRAJ_STATS), dtype=torch.float64, device=coeff.device)
        if samples is None:
            samples = torch.zeros(B, max(max_samples, 0), 3, dtype=torch.float64, device=coeff.device)
        for t, cnt in ((stats, B * len(self.TRAJ_STATS)), (samples, B * max_samples * 3)):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == max(cnt, 0)
        if stream is None:
            stream = torch.cuda.current_stream(coeff.device).cuda_stream
        self._chk(self._L.gtop_sample_trajectories_device(self._h, B, m, C.c_void_p(coeff.data_ptr()),
                                                          C.c_void_p(T.data_ptr()), m if T.dim() == 2 else 0,
                                                          float(dt_sample), C.c_void_p(stats.data_ptr()),
                                                          C.c_void_p(samples.data_ptr()), max_samples,
                                                          C.c_void_p(stream)))
        return stats, samples

    def validate_device(self, coeff, T, limits, dt_sample=0.01, report=None, stream=None):
        """torch fp64 CUDA tensors coeff (B, m, 18), T (B, m) or (m,) -> report (B, 12); asynchronous, capturable
        (pass `report` to write into a buffer of the caller's)."""
        import torch
        assert coeff.is_cuda and coeff.dtype == T.dtype == torch.float64 and coeff.is_contiguous() and T.is_contiguous()
        B, m = coeff.shape[0], coeff.shape[1]
        if report is None:
            report = torch.empty(B, len(self.TRAJ_REPORT), dtype=torch.float64, device=coeff.device)
        assert report.is_contiguous() and report.dtype == torch.float64 and report.numel() == B * len(self.TRAJ_REPORT)
        if stream is None:
            stream = torch.cuda.current_stream(coeff.device).cuda_stream
        self._chk(self._L.gtop_validate_trajectories_device(self._h, B, m, C.c_void_p(coeff.data_ptr()),
                                                            C.c_void_p(T.data_ptr()), m if T.dim() == 2 else 0,
                                                            float(dt_sample), C.byref(limits),
                                                            C.c_void_p(report.data_ptr()), C.c_void_p(stream)))
        return report

    def select_best_device(self, report, cost, limits, want_pass=True, best=None, stream=None):
        """report (B, 12), cost (B,) torch fp64 CUDA tensors -> (pass (B,) uint8 or None, best (2,) int32);
        asynchronous, capturable."""
        import torch
        assert report.is_cuda and report.dtype == cost.dtype == torch.float64 and report.is_contiguous() and cost.is_contiguous()
        B = cost.numel()
        assert report.numel() == B * len(self.TRAJ_REPORT)
        ok = torch.empty(B, dtype=torch.uint8, device=report.device) if want_pass else None
        if best is None:
            best = torch.empty(2, dtype=torch.int32, device=report.device)
        if stream is None:
            stream = torch.cuda.current_stream(report.device).cuda_stream
        self._chk(self._L.gtop_select_best_device(self._h, B, C.c_void_p(report.data_ptr()), C.c_void_p(cost.data_ptr()),
                                                  C.byref(limits), C.c_void_p(ok.data_ptr()) if want_pass else None,
                                                  C.c_void_p(best.data_ptr()), C.c_void_p(stream)))
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
        import torch
        assert coeff.is_cuda and coeff.dtype == T.dtype == torch.float64 and coeff.is_contiguous() and T.is_contiguous()
        B, m = coeff.shape[0], coeff.shape[1]
        assert T.shape == (m,) or T.shape == (B, m)
        if seg_report is None:
            seg_report = torch.empty(B, m, len(self.SEG_REPORT), dtype=torch.float64, device=coeff.device)
        assert seg_report.is_cuda and seg_report.is_contiguous() and seg_report.dtype == torch.float64
        assert seg_report.numel() == B * m * len(self.SEG_REPORT)
        if stream is None:
            stream = torch.cuda.current_stream(coeff.device).cuda_stream
        self._chk(self._L.gtop_validate_segments_device(self._h, B, m, C.c_void_p(coeff.data_ptr()),
                                                        C.c_void_p(T.data_ptr()), m if T.dim() == 2 else 0,
                                                        float(dt_sample), C.byref(limits),
                                                        C.c_void_p(seg_report.data_ptr()), C.c_void_p(stream)))
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
        import torch
        given = [t for t in (x, Df, T, seg_report, T_out) if t is not None]
        for t in given:
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
        if x is not None:
            B, m = x.shape[0], x.shape[1] // 9 + 1
        else:
            B, m = seg_report.shape[0], seg_report.shape[1]
        stride = m if (T is None or T.dim() == 2) else 0
        if T_out is None:
            T_out = torch.empty(B, m, dtype=torch.float64, device=given[0].device)
        assert T_out.numel() == B * m
        if stream is None:
            stream = torch.cuda.current_stream(T_out.device).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self._L.gtop_reallocate_times_device(self._h, C.byref(options), B, m, ptr(x), ptr(Df), ptr(T), stride,
                                                       ptr(seg_report), ptr(T_out), C.c_void_p(stream)))
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
        assert lb.shape == x.shape == ub.shape
        cost = np.empty(B)
        self._chk(self._L.gtop_optimize_batch(self._h, B, _p(x), _p(lb), _p(ub), int(max_evals), _p(cost)))
        return x, cost

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
        self._chk(self._L.gtop_optimize_batch_ex(self._h, B, _p(x), _p(lb), _p(ub), C.byref(stop), _p(cost),
                                                 nev.ctypes.data_as(ip), code.ctypes.data_as(ip)))
        return x, cost, nev, code

    def optimize_device_ex(self, x, Df, T, lb, ub, max_evals, ftol_rel=0.0, xtol_rel=0.0, maxtime=0.0, stream=None):
        """torch fp64 CUDA tensors; x is overwritten with the best point; returns (x, min_cost, nevals, code)."""
        import torch
        B, n = x.shape
        m = n // 9 + 1
        stride = m if T.dim() == 2 else 0
        for t in (x, Df, T, lb, ub):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
        min_cost = torch.empty(B, dtype=torch.float64, device=x.device)
        nev = torch.empty(B, dtype=torch.int32, device=x.device)
        code = torch.empty(B, dtype=torch.int32, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        stop = GtopStop(int(max_evals), float(ftol_rel), float(xtol_rel), float(maxtime))
        self._chk(self._L.gtop_optimize_device_ex(
            self._h, B, m, C.c_void_p(x.data_ptr()), C.c_void_p(Df.data_ptr()), C.c_void_p(T.data_ptr()), stride,
            C.c_void_p(lb.data_ptr()), C.c_void_p(ub.data_ptr()), C.byref(stop), C.c_void_p(min_cost.data_ptr()),
            C.c_void_p(nev.data_ptr()), C.c_void_p(code.data_ptr()), C.c_void_p(stream)))
        return x, min_cost, nev, code

    def optimize_device(self, x, Df, T, lb, ub, max_evals, min_cost=None, stream=None):
        """torch fp64 CUDA tensors; x is overwritten with the best point."""
        import torch
        B, n = x.shape
        m = n // 9 + 1
        stride = m if T.dim() == 2 else 0
        for t in (x, Df, T, lb, ub):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
        if min_cost is None:
            min_cost = torch.empty(B, dtype=torch.float64, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        self._chk(self._L.gtop_optimize_device(self._h, B, m, C.c_void_p(x.data_ptr()), C.c_void_p(Df.data_ptr()),
                                               C.c_void_p(T.data_ptr()), stride, C.c_void_p(lb.data_ptr()),
                                               C.c_void_p(ub.data_ptr()), int(max_evals),
                                               C.c_void_p(min_cost.data_ptr()), C.c_void_p(stream)))
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


class Rendezvous:
    """N serial callers sharing one launch (include/gtop.h, gtop_rendezvous_*).  The context's problem must hold
    the N trajectories (row i = caller i).  Each caller thread uses `cost(i, x)` as its objective and calls
    `leave(i)` when its optimizer has returned."""

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

    def close(self):
        if getattr(self, "_h", None):
            self._L.gtop_rendezvous_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GtopGroup:
    """One batch over several devices from one process (include/gtop.h, gtop_group_*): the field replicated, the
    batch in contiguous slices, every slice launched on its own device, results gathered on the host or all-gathered
    on the devices (RCCL when the devices differ, peer copies otherwise)."""

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

    def _chk(self, rc):
        if rc != 0:
            raise GtopError(rc, self._L.gtop_group_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.gtop_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def gather_backend(self):
        return self._L.gtop_group_gather_backend(self._h).decode()

    def gather_note(self):
        """The backend and why: a fallback from RCCL to peer copies names its reason."""
        return self._L.gtop_group_gather_note(self._h).decode()

    def set_params(self, **kw):
        d = dict(OPTI_NODE_PARAMS)
        d.update(kw)
        p = GtopParams(**d)
        self._chk(self._L.gtop_group_set_params(self._h, C.byref(p)))

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

    def set_problem(self, T, Df):
        Df = _f64(Df)
        B = Df.size // 18
        T = _f64(T)
        m, stride = (T.shape[1], T.shape[1]) if T.ndim == 2 else (T.shape[0], 0)
        self._chk(self._L.gtop_group_set_problem(self._h, B, m, _p(T), stride, _p(Df)))
        self.B, self.m = B, m

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
        self._L.gtop_group_context.restype = C.c_void_p
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

    def optimize_batch_ex(self, x0, lb, ub, max_evals, ftol_rel=0.0, xtol_rel=0.0, maxtime=0.0):
        x = _f64(x0).copy()
        B = x.shape[0]
        lb, ub = _f64(lb), _f64(ub)
        cost = np.empty(B)
        nev = np.empty(B, dtype=np.int32)
        code = np.empty(B, dtype=np.int32)
        stop = GtopStop(int(max_evals), float(ftol_rel), float(xtol_rel), float(maxtime))
        ip = C.POINTER(C.c_int32)
        self._chk(self._L.gtop_group_optimize_batch_ex(self._h, B, _p(x), _p(lb), _p(ub), C.byref(stop), _p(cost),
                                                       nev.ctypes.data_as(ip), code.ctypes.data_as(ip)))
        return x, cost, nev, code
