"""The C-ABI of libgtop_hip.so as ctypes sees it (include/gtop.h): its structures, the table of its entry points and
the loader.  _lib.py wraps it in classes."""
import ctypes as C
import os

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


class GtopCertifyOpts(C.Structure):
    """gtop_certify_opts of include/gtop.h: the margin of the continuous-time clearance certificate, the levels of
    refinement below a segment's 64 intervals (0 .. 3) and the refinements a trajectory may spend."""
    _fields_ = [("margin", C.c_double), ("max_depth", C.c_int32), ("max_refine", C.c_int32)]

    def __init__(self, margin=0.0, max_depth=2, max_refine=256):
        super().__init__(float(margin), int(max_depth), int(max_refine))


class GtopCertifyMovingOpts(C.Structure):
    """gtop_certify_moving_opts of include/gtop.h: GtopCertifyOpts' three fields, use_boxes (False: the static
    certificate, bit for bit) and a reserved word that must be 0."""
    _fields_ = [("margin", C.c_double), ("max_depth", C.c_int32), ("max_refine", C.c_int32), ("use_boxes", C.c_int32),
                ("reserved", C.c_int32)]

    def __init__(self, margin=0.0, max_depth=2, max_refine=256, use_boxes=True, reserved=0):
        super().__init__(float(margin), int(max_depth), int(max_refine), int(bool(use_boxes)), int(reserved))


class GtopInsert(C.Structure):
    """gtop_insert of include/gtop.h: how insert_waypoints[_device] (insert.py) cuts one segment of every row in two.
    mode 0 (AT_TIME): at the trajectory time `when` gives; mode 1 (LONGEST): the longest segment in the middle.
    min_fraction in (0, 0.5] keeps that share of the segment on either side of the cut; push > 0 moves the new waypoint
    that far up the static field's gradient where the distance is below push_below; bos, vos, aos bound the new
    waypoint when lb / ub are given; reserved must be 0."""
    AT_TIME, LONGEST = 0, 1
    _fields_ = [("mode", C.c_int32), ("min_fraction", C.c_double), ("push", C.c_double), ("push_below", C.c_double),
                ("bos", C.c_double), ("vos", C.c_double), ("aos", C.c_double), ("reserved", C.c_int32)]

    def __init__(self, mode=1, min_fraction=0.1, push=0.0, push_below=0.0, bos=3.0, vos=8.0, aos=10.0, reserved=0):
        super().__init__(int(mode), float(min_fraction), float(push), float(push_below), float(bos), float(vos),
                         float(aos), int(reserved))


_i, _d, _vp, _dp, _ip = C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_params, _stop, _limits, _retime = (C.POINTER(s) for s in (GtopParams, GtopStop, GtopLimits, GtopRetime))
_certify, _certify_moving = C.POINTER(GtopCertifyOpts), C.POINTER(GtopCertifyMovingOpts)
_insert = C.POINTER(GtopInsert)

# Every entry point of include/gtop.h: name -> (the ABI version that introduced it, 0 when the header does not say;
# restype; argtypes).
ENTRY_POINTS = {
    "gtop_abi_version": (0, _i, []),
    "gtop_create": (0, _i, [C.POINTER(_vp), _i]),
    "gtop_destroy": (0, _i, [_vp]),
    "gtop_last_error": (0, C.c_char_p, [_vp]),
    "gtop_set_params": (0, _i, [_vp, _params]),
    "gtop_set_sdf": (0, _i, [_vp, _dp, _i, _i, _i, _dp, _dp, _d]),
    "gtop_set_sdf_device": (0, _i, [_vp, _i, _vp, _i, _i, _i, _dp, _dp, _d]),
    "gtop_init_sdf_map": (0, _i, [_vp, _dp, _dp, _d]),
    "gtop_update_sdf_map": (0, _i, [_vp, _dp, _i]),
    "gtop_update_sdf_map_device": (0, _i, [_vp, _vp, _i, _vp]),
    "gtop_get_sdf": (0, _i, [_vp, _dp, _ip]),
    "gtop_set_problem": (0, _i, [_vp, _i, _i, _dp, _i, _dp]),
    "gtop_eval_batch": (0, _i, [_vp, _i, _dp, _dp, _dp]),
    "gtop_cost_nlopt": (0, _d, [C.c_uint, _dp, _dp, _vp]),
    "gtop_eval_device": (0, _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "gtop_set_paths": (0, _i, [_vp, _i, _i, _dp, _d, _d, _dp]),
    "gtop_setup_paths_device": (0, _i, [_vp, _i, _i, _vp, _d, _d, _vp, _vp, _vp, _vp]),
    "gtop_get_problem": (0, _i, [_vp, _dp, _dp]),
    "gtop_min_jerk_start_device": (8, _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "gtop_min_jerk_start": (8, _i, [_vp, _i, _dp]),
    "gtop_coefficients_device": (0, _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "gtop_eval_trajectories_device": (0, _i, [_vp, _i, _i, _vp, _vp, _i, _d, _vp, _vp]),
    "gtop_trajectory_stats": (0, _i, [_vp, _i, _dp, _d, _dp, _dp]),
    "gtop_set_moving_boxes": (0, _i, [_vp, _i, _dp, _dp, _dp]),
    "gtop_set_moving_box_polynomials": (7, _i, [_vp, _i, _dp, _dp, _dp]),
    "gtop_get_moving_box_kind": (7, _i, [_vp, _ip, _ip]),
    "gtop_box_polynomial_centres": (7, _i, [_i, _dp, _dp, _i, _dp, _dp]),
    "gtop_set_moving_cost": (4, _i, [_vp, _i]),
    "gtop_get_moving_cost": (4, _i, [_vp, _ip]),
    "gtop_set_gradient_mode": (6, _i, [_vp, _i]),
    "gtop_get_gradient_mode": (6, _i, [_vp, _ip]),
    "gtop_group_set_gradient_mode": (6, _i, [_vp, _i]),
    "gtop_set_start_times": (4, _i, [_vp, _i, _dp]),
    "gtop_set_start_times_device": (4, _i, [_vp, _i, _vp]),
    "gtop_edt_query_device": (0, _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gtop_edt_query": (0, _i, [_vp, _i, _dp, _dp, _dp, _dp]),
    "gtop_edt_coarse_query_device": (0, _i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "gtop_edt_coarse_query": (0, _i, [_vp, _i, _dp, _dp, _dp]),
    "gtop_sample_trajectories_device": (0, _i, [_vp, _i, _i, _vp, _vp, _i, _d, _vp, _vp, _i, _vp]),
    "gtop_trajectory_samples": (0, _i, [_vp, _i, _dp, _d, _dp, _dp, _dp, _i]),
    "gtop_validate_trajectories_device": (5, _i, [_vp, _i, _i, _vp, _vp, _i, _d, _limits, _vp, _vp]),
    "gtop_select_best_device": (5, _i, [_vp, _i, _vp, _vp, _limits, _vp, _vp, _vp]),
    "gtop_validate_batch": (5, _i, [_vp, _i, _dp, _d, _limits, _dp, _dp, C.POINTER(C.c_ubyte), _i32p]),
    "gtop_validate_segments_device": (9, _i, [_vp, _i, _i, _vp, _vp, _i, _d, _limits, _vp, _vp]),
    "gtop_validate_segments": (9, _i, [_vp, _i, _dp, _d, _limits, _dp]),
    "gtop_reallocate_times_device": (9, _i, [_vp, _retime, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "gtop_reallocate_times": (9, _i, [_vp, _retime, _i, _dp, _d, _limits, _dp]),
    "gtop_default_bounds": (0, _i, [_i, _i, _dp, _d, _d, _d, _dp, _dp]),
    "gtop_optimize_batch": (0, _i, [_vp, _i, _dp, _dp, _dp, _i, _dp]),
    "gtop_optimize_device": (0, _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "gtop_optimize_batch_ex": (0, _i, [_vp, _i, _dp, _dp, _dp, _stop, _dp, _i32p, _i32p]),
    "gtop_optimize_device_ex": (0, _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _stop, _vp, _vp, _vp, _vp]),
    "gtop_get_stats": (0, _i, [_vp, _i64p, _dp]),
    "gtop_reset_stats": (0, _i, [_vp]),
    "gtop_get_cost_curve": (0, _i, [_vp, _dp, _dp, _i, _ip]),
    "gtop_clear_cost_curve": (0, _i, [_vp]),
    "gtop_set_launch_geometry": (0, _i, [_vp, _i, _i]),
    "gtop_update_sdf_map_window": (0, _i, [_vp, _dp, _dp, _dp, _i]),
    "gtop_update_sdf_map_window_device": (0, _i, [_vp, _dp, _dp, _vp, _i, _vp]),
    "gtop_set_field_precisions": (0, _i, [_vp, _i]),
    "gtop_set_field_sign": (0, _i, [_vp, _i, _d]),
    "gtop_get_field_sign": (0, _i, [_vp, _ip, _dp]),
    "gtop_group_set_field_sign": (0, _i, [_vp, _i, _d]),
    "gtop_device_clock_stamp": (0, _i, [_vp, _vp, _vp]),
    "gtop_push_rows": (0, _i, [_vp, _vp, C.c_size_t, C.POINTER(_vp), _i, _vp, _vp]),
    "gtop_shared_alloc": (0, _i, [_vp, C.c_size_t, C.POINTER(_vp), C.c_char_p]),
    "gtop_shared_open": (0, _i, [_vp, C.c_char_p, _i, C.POINTER(_vp)]),
    "gtop_shared_close": (0, _i, [_vp, _vp]),
    "gtop_shared_free": (0, _i, [_vp, _vp]),
    "gtop_device_clock_hz": (0, _i, [_vp, _dp]),
    "gtop_rendezvous_create": (0, _i, [C.POINTER(_vp), _vp, _i, _i]),
    "gtop_rendezvous_destroy": (0, _i, [_vp]),
    "gtop_rendezvous_get_slot": (0, _vp, [_vp, _i]),
    "gtop_cost_nlopt_shared": (0, _d, [C.c_uint, _dp, _dp, _vp]),
    "gtop_rendezvous_leave": (0, _i, [_vp]),
    "gtop_rendezvous_set_timeout": (0, _i, [_vp, _d]),
    "gtop_rendezvous_abort": (0, _i, [_vp]),
    "gtop_rendezvous_stats": (0, _i, [_vp, _i64p, _dp, _i64p]),
    "gtop_set_optimizer_fusion": (0, _i, [_vp, _i]),
    "gtop_set_optimizer_precision": (0, _i, [_vp, _i]),
    "gtop_group_create": (0, _i, [C.POINTER(_vp), _ip, _i]),
    "gtop_group_destroy": (0, _i, [_vp]),
    "gtop_group_size": (0, _i, [_vp]),
    "gtop_group_context": (0, _vp, [_vp, _i]),
    "gtop_group_last_error": (0, C.c_char_p, [_vp]),
    "gtop_group_gather_backend": (0, C.c_char_p, [_vp]),
    "gtop_group_gather_note": (0, C.c_char_p, [_vp]),
    "gtop_group_update_sdf_map_window": (0, _i, [_vp, _dp, _dp, _dp, _i]),
    "gtop_group_set_params": (0, _i, [_vp, _params]),
    "gtop_group_init_sdf_map": (0, _i, [_vp, _dp, _dp, _d]),
    "gtop_group_update_sdf_map": (0, _i, [_vp, _dp, _i]),
    "gtop_group_set_sdf": (0, _i, [_vp, _dp, _i, _i, _i, _dp, _dp, _d]),
    "gtop_group_set_problem": (0, _i, [_vp, _i, _i, _dp, _i, _dp]),
    "gtop_group_shard": (0, _i, [_vp, _i, _ip, _ip]),
    "gtop_group_eval_batch": (0, _i, [_vp, _i, _dp, _dp, _dp]),
    "gtop_group_upload_x": (0, _i, [_vp, _i, _dp]),
    "gtop_group_eval_resident": (0, _i, [_vp, _i, _i]),
    "gtop_group_synchronize": (0, _i, [_vp]),
    "gtop_group_read_gathered": (0, _i, [_vp, _i, _dp, _dp]),
    "gtop_group_device_buffers": (0, _i, [_vp, _i] + [C.POINTER(_vp)] * 6),
    "gtop_group_optimize_batch_ex": (0, _i, [_vp, _i, _dp, _dp, _dp, _stop, _dp, _i32p, _i32p]),
    "gtop_certify_trajectories_device": (10, _i, [_vp, _i, _i, _vp, _vp, _i, _certify, _vp, _vp]),
    "gtop_certify_batch": (10, _i, [_vp, _i, _dp, _certify, _dp]),
    "gtop_select_best_certified_device": (10, _i, [_vp, _i, _vp, _vp, _vp, _limits, _i, _vp, _vp, _vp]),
    "gtop_certify_moving_device": (11, _i, [_vp, _i, _i, _vp, _vp, _i, _certify_moving, _vp, _vp]),
    "gtop_certify_moving_batch": (11, _i, [_vp, _i, _dp, _certify_moving, _dp]),
    "gtop_insert_waypoints_device": (12, _i, [_vp, _insert, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp]),
    "gtop_insert_waypoints": (12, _i, [_vp, _insert, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
}
# the ABI version this package speaks: gtop_abi_version() of the in-tree build
ABI_VERSION = max(since for since, _, _ in ENTRY_POINTS.values())


def entry_points(abi):
    """The names a library of ABI version `abi` has."""
    return [name for name, (since, _, _) in ENTRY_POINTS.items() if since <= abi]


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


_lib = None


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
    # An OLDER build chosen through GTOP_HIP_LIB (A/B timing against a parent commit) lacks the entry points of a later
    # ABI version: those stay unbound there (calling one raises AttributeError); the in-tree library must have them all.
    L.gtop_abi_version.restype = C.c_int
    other = bool(os.environ.get("GTOP_HIP_LIB"))
    for name in entry_points(L.gtop_abi_version() if other else ABI_VERSION):
        f = getattr(L, name)
        _, f.restype, f.argtypes = ENTRY_POINTS[name]
    _lib = L
    return L
