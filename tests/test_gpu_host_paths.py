"""The host paths of csrc/gtop_capi_boxes.cpp, gtop_capi_report.cpp and gtop_capi_remedy.cpp (and gtop_trajectory_samples
of gtop_capi_problem.cpp, which shares their opening check and coefficient staging), held to what the library did
BEFORE the three files were cut out of one and their repeated scaffolding was written once.  The expectations are
literals copied from that earlier source, not read from the code under test, and the file passes unchanged on a build
of that commit chosen through GTOP_HIP_LIB.

(1) A table of refused calls, (status, exact error text) each, through the raw entry points: every entry of the three
    files with a NULL context; at least one row per distinct text; the order of the checks where two of them apply;
    B = 0 with every buffer NULL (GTOP_OK) for every device form that has buffers to leave out — the two selections
    always need `best` (B = 0 with every buffer NULL is refused there; with `best` alone it is {-1, 0}).  A refused
    call launches nothing: every non-NULL device argument is one zeroed buffer larger than any of these shapes reads.
(2) The start-time list and the static certificate: with 3 start times set for 2 rows the static certificate (device
    and host form) still runs and gives the rows it gave with none set, bit for bit; the moving certificate and the
    report with use_boxes = 0 are refused.
(3) The paths that are one path now agree bit for bit: certify_batch and certify_moving_batch(use_boxes = 0);
    select_best_device and select_best_certified_device over certificates that all say SAFE; the coefficients
    gtop_trajectory_samples returns, coefficients_device's on the same x, and what gtop_validate_batch staged (its
    report is validate_device's on those coefficients).

One context: an 8 x 8 x 8 map at 0.5 m with one obstacle point, a problem of B = 2 rows of m = 2 segments."""
import ctypes as C
import math

import numpy as np
import pytest

from grad_traj_optimization_amd import _abi, certify, insert

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, 1, 4
B, M, N = 2, 2, 9
NO_PROBLEM = "gtop_set_problem / gtop_set_paths has not been called"
NO_FIELD = "no fp64 distance field resident"
V_NEED = "validate: need B >= 0, m >= 1, dt_sample > 0, time_stride in {0, m}"
V_NULL_LIMITS = "validate: limits is NULL"
V_FINITE = "validate: margin, max_vel and max_acc must be finite"
V_T0 = "validate: the number of start times does not match the batch"
SEL = "select_best: need B >= 0, best, and report and cost for B > 0"
SELC = "select_best_certified: need B >= 0, best, and report, cert and cost for B > 0"
SELC_REQUIRE = "select_best_certified: require is neither SAFE nor NOT_UNSAFE"
VB_ROWS = "validate_batch: 1 <= B <= problem batch, x and report required"
VS_ROWS = "validate_segments: 1 <= B <= problem batch, x and seg_report required"
C_NULL = "certify: options is NULL"
C_OPTS = "certify: need a finite margin, max_depth in 0 .. 3, max_refine >= 0"
C_NEED = "certify: need B >= 0, 2 <= m <= 227, time_stride in {0, m}"
CB_ROWS = "certify_batch: 1 <= B <= problem batch, x and cert required"
CM_NULL = "certify_moving: options is NULL"
CM_RESERVED = "certify_moving: reserved must be 0"
CM_T0 = "certify_moving: the number of start times does not match the batch"
CMB_ROWS = "certify_moving_batch: 1 <= B <= problem batch, x and cert required"
R_NULL = "reallocate_times: options is NULL"
R_LENGTH = "reallocate_times: LENGTH needs a finite mean_v > 0 and a finite init_time >= 0"
R_LIMITS = "reallocate_times: LIMITS needs a finite max_ratio >= 1"
R_NEED = "reallocate_times: need B >= 0, 2 <= m <= 227, time_stride in {0, m}"
R_BUF_LENGTH = "reallocate_times: NULL buffer (LENGTH: x, Df, T_out)"
R_BUF_LIMITS = "reallocate_times: NULL buffer (LIMITS: T, seg_report, T_out; x with scale_x)"
R_SHARED = "reallocate_times: a shared time vector cannot be its own per-trajectory output"
R_ROWS = "reallocate_times: 1 <= B <= problem batch, x and T_out required"
I_FRACTION = "insert_waypoints: min_fraction must lie in (0, 0.5]"
I_OUT = "insert_waypoints: lb_out and ub_out are required exactly when lb and ub are given"
I_NEED = "insert_waypoints: need B >= 0, 2 <= m <= 226, time_stride in {0, m}"
I_BUF = "insert_waypoints: NULL buffer (x, coeff, T, x_out, T_out; when under AT_TIME)"
I_ROWS = "insert_waypoints: 1 <= B <= problem batch; x, x_out and T_out required, when under AT_TIME"
TS_ROWS = "trajectory_stats: 1 <= B <= problem batch, x and an output required"
MOV_T0 = "moving-obstacle cost: the number of start times does not match the batch"

NAN, INF = math.nan, math.inf
Limits, Retime, Insert = _abi.GtopLimits, _abi.GtopRetime, _abi.GtopInsert
Opts, MovingOpts = _abi.GtopCertifyOpts, _abi.GtopCertifyMovingOpts


def ref(s):
    return None if s is None else C.byref(s)


def hp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class Env:
    """The one context, the zeroed device buffer D behind every non-NULL device argument of a refused call, and host
    arrays to point at."""

    def __init__(self, gtop):
        import torch
        self.torch, self.gtop = torch, gtop
        self.ctx = gtop.GtopContext(0)
        self.L, self.h = self.ctx._L, self.ctx._h
        self.pad = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
        self.D = self.pad.data_ptr()
        self.host = np.zeros(4096)
        self.H = hp(self.host)

    def call(self, name, *args):
        """(status, the context's error text after the call)"""
        rc = getattr(self.L, name)(self.h, *args)
        return rc, self.L.gtop_last_error(self.h).decode()

    def make_ready(self):
        """the field and the problem; returns x0"""
        self.ctx.init_sdf_map([4.0, 4.0, 4.0], [-2.0, -2.0, 0.0], 0.5)
        self.ctx.update_sdf_map(np.array([[0.2, 0.3, 1.0]]))
        wp = np.array([[[-1.2, -1.0, 1.0], [0.1, 0.5, 1.2], [1.2, 1.0, 1.0]],
                       [[-1.0, 1.2, 0.8], [-0.2, 0.1, 1.5], [1.1, -1.2, 1.1]]])
        self.x0 = self.ctx.set_paths(wp)
        assert self.x0.shape == (B, N) and (self.ctx.B, self.ctx.m) == (B, M)
        return self.x0

    def dev(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


@pytest.fixture(scope="module")
def env(gtop):
    e = Env(gtop)
    yield e
    e.ctx.close()


def device_rows(e, have_field):
    """(entry, args, status, text): the device forms and the setters, which need no problem.  have_field False: what a
    context without a distance field answers where the field is asked for (after the options and shape rules)."""
    D, H = e.D, e.H
    lim, opt, mov = Limits(), Opts(0.1, 1, 4), MovingOpts(0.1, 1, 4, True)
    length, limits_mode = Retime(mode=0), Retime(mode=1)
    longest, at_time = Insert(mode=1), Insert(mode=0)
    rows = []

    def add(entry, args, status, text=None):
        rows.append((entry, args, status, text))

    # -- the sampled reports (both say "validate:" but for the NULL-buffer text): shape rules, then limits, then start
    # times, then the field, then B == 0, then the buffers
    for entry, who in (("gtop_validate_trajectories_device", "validate"), ("gtop_validate_segments_device", "validate_segments")):
        add(entry, (B, M, D, D, M, 0.01, None, D, None), INVALID, V_NULL_LIMITS)
        add(entry, (B, 0, D, D, 0, 0.01, None, D, None), INVALID, V_NEED)        # (the shape rules come first here)
        for bad in ((-1, M, D, D, M, 0.01), (B, M, D, D, M, 0.0), (B, M, D, D, M, NAN), (B, M, D, D, 1, 0.01)):
            add(entry, (*bad, ref(lim), D, None), INVALID, V_NEED)
        for bad in (Limits(margin=INF), Limits(max_vel=NAN), Limits(max_acc=-INF)):
            add(entry, (B, M, D, D, M, 0.01, ref(bad), D, None), INVALID, V_FINITE)
        if have_field:
            add(entry, (0, M, None, None, 0, 0.01, ref(lim), None, None), OK)
            for nulls in ((None, D, D), (D, None, D), (D, D, None)):
                add(entry, (B, M, nulls[0], nulls[1], M, 0.01, ref(lim), nulls[2], None), INVALID, who + ": NULL buffer")
        else:
            add(entry, (0, M, None, None, 0, 0.01, ref(lim), None, None), STATE, NO_FIELD)
            add(entry, (B, M, None, None, M, 0.01, ref(lim), None, None), STATE, NO_FIELD)
    # -- the selections: limits, (require,) then B and the buffers; no field needed
    add("gtop_select_best_device", (B, D, D, None, D, D, None), INVALID, V_NULL_LIMITS)
    add("gtop_select_best_device", (-1, None, None, None, None, None, None), INVALID, V_NULL_LIMITS)
    add("gtop_select_best_device", (B, D, D, ref(Limits(max_vel=NAN)), D, D, None), INVALID, V_FINITE)
    for bad in ((-1, D, D, D, D), (B, None, D, D, D), (B, D, None, D, D), (B, D, D, D, None), (0, None, None, None, None)):
        add("gtop_select_best_device", (bad[0], bad[1], bad[2], ref(lim), bad[3], bad[4], None), INVALID, SEL)
    add("gtop_select_best_certified_device", (B, D, D, D, None, 0, D, D, None), INVALID, V_NULL_LIMITS)
    add("gtop_select_best_certified_device", (B, D, D, D, ref(Limits(margin=NAN)), 1, D, D, None), INVALID, V_FINITE)
    for require in (0, 3, -1):
        add("gtop_select_best_certified_device", (B, D, D, D, ref(lim), require, None, None, None), INVALID, SELC_REQUIRE)
    for bad in ((-1, D, D, D, D), (B, None, D, D, D), (B, D, None, D, D), (B, D, D, None, D), (B, D, D, D, None),
                (0, None, None, None, None)):
        add("gtop_select_best_certified_device", (*bad[:4], ref(lim), 2, D, bad[4], None), INVALID, SELC)
    # -- the certificates: options, (reserved,) their values, the shape rules, the field, (start times,) B == 0, buffers
    for entry, who, o, null_text in (("gtop_certify_trajectories_device", "certify", opt, C_NULL),
                                     ("gtop_certify_moving_device", "certify_moving", mov, CM_NULL)):
        moving = o is mov
        make = (lambda *a: MovingOpts(*a, True)) if moving else Opts
        add(entry, (B, M, D, D, M, None, D, None), INVALID, null_text)
        add(entry, (-1, 1, None, None, 1, None, None, None), INVALID, null_text)   # before the shape rules
        for bad in (make(NAN, 1, 4), make(INF, 1, 4), make(0.1, -1, 4), make(0.1, 4, 4), make(0.1, 1, -1)):
            add(entry, (B, M, D, D, M, ref(bad), D, None), INVALID, C_OPTS)
            add(entry, (-1, 1, D, D, M, ref(bad), D, None), INVALID, C_OPTS)      # before the shape rules
        for bad in ((-1, M, M), (B, 1, 1), (B, 228, 228), (B, M, 1)):
            add(entry, (bad[0], bad[1], D, D, bad[2], ref(o), D, None), INVALID, C_NEED)
        add(entry, (B, 227, D, D, 227, ref(o), None, None),
            *((INVALID, who + ": NULL buffer") if have_field else (STATE, NO_FIELD)))
        if have_field:
            add(entry, (0, M, None, None, 0, ref(o), None, None), OK)
            for nulls in ((None, D, D), (D, None, D), (D, D, None)):
                add(entry, (B, M, nulls[0], nulls[1], M, ref(o), nulls[2], None), INVALID, who + ": NULL buffer")
        else:
            add(entry, (0, M, None, None, 0, ref(o), None, None), STATE, NO_FIELD)
    add("gtop_certify_moving_device", (B, M, D, D, M, ref(MovingOpts(0.1, 1, 4, True, 1)), D, None), INVALID, CM_RESERVED)
    add("gtop_certify_moving_device", (B, 1, D, D, 1, ref(MovingOpts(NAN, 9, 4, False, -2)), D, None), INVALID, CM_RESERVED)
    # -- the segment-time reallocation: options, the shape rules, B == 0, the mode's buffers; no field needed
    add("gtop_reallocate_times_device", (None, B, M, D, D, D, M, D, D, None), INVALID, R_NULL)
    add("gtop_reallocate_times_device", (None, -1, 1, None, None, None, 1, None, None, None), INVALID, R_NULL)
    for bad in (Retime(mode=0, mean_v=0.0), Retime(mode=0, mean_v=INF), Retime(mode=0, mean_v=NAN),
                Retime(mode=0, init_time=-0.1), Retime(mode=0, init_time=INF)):
        add("gtop_reallocate_times_device", (ref(bad), B, M, D, D, D, M, D, D, None), INVALID, R_LENGTH)
    for bad in (Retime(mode=1, max_ratio=0.5), Retime(mode=1, max_ratio=INF), Retime(mode=1, max_ratio=NAN)):
        add("gtop_reallocate_times_device", (ref(bad), B, 1, D, D, D, M, D, D, None), INVALID, R_LIMITS)
    for mode in (2, -1):
        add("gtop_reallocate_times_device", (ref(Retime(mode=mode)), B, M, D, D, D, M, D, D, None), INVALID,
            "reallocate_times: unknown mode")
    for o in (length, limits_mode):
        for bad in ((-1, M, M), (B, 1, 1), (B, 228, 228), (B, M, 1)):
            add("gtop_reallocate_times_device", (ref(o), bad[0], bad[1], D, D, D, bad[2], D, D, None), INVALID, R_NEED)
        add("gtop_reallocate_times_device", (ref(o), 0, M, None, None, None, 0, None, None, None), OK)
    for nulls in ((None, D, D), (D, None, D), (D, D, None)):
        add("gtop_reallocate_times_device", (ref(length), B, M, nulls[0], nulls[1], None, M, None, nulls[2], None), INVALID,
            R_BUF_LENGTH)
        add("gtop_reallocate_times_device", (ref(limits_mode), B, M, None, None, nulls[0], M, nulls[1], nulls[2], None),
            INVALID, R_BUF_LIMITS)
    add("gtop_reallocate_times_device", (ref(Retime(mode=1, scale_x=True)), B, M, None, None, D, M, D, D, None), INVALID,
        R_BUF_LIMITS)
    add("gtop_reallocate_times_device", (ref(limits_mode), B, M, D, D, D, 0, D, D, None), INVALID, R_SHARED)
    # -- the waypoint insertion: options in the order of their fields' checks, the bounds' pairing, the shape rules,
    # when_stride, the field (only with a push), B == 0, the buffers
    def ins(o, b=B, m=M, x=D, coeff=D, T=D, ts=None, when=D, ws=1, lb=None, ub=None, x_out=D, T_out=D, lb_out=None,
            ub_out=None, info=None):
        return (ref(o), b, m, x, coeff, T, m if ts is None else ts, when, ws, lb, ub, x_out, T_out, lb_out, ub_out, info, None)

    entry = "gtop_insert_waypoints_device"
    add(entry, ins(None), INVALID, "insert_waypoints: options is NULL")
    add(entry, ins(None, b=-1, m=1), INVALID, "insert_waypoints: options is NULL")
    for mode in (2, -1):
        add(entry, ins(Insert(mode=mode, reserved=1)), INVALID, "insert_waypoints: unknown mode")
    add(entry, ins(Insert(reserved=1, min_fraction=0.0)), INVALID, "insert_waypoints: reserved must be 0")
    for f in (0.0, -0.1, 0.51, NAN):
        add(entry, ins(Insert(min_fraction=f, push=INF)), INVALID, I_FRACTION)
    for push, below in ((INF, 0.0), (NAN, 0.0), (0.0, INF), (0.0, NAN)):
        add(entry, ins(Insert(push=push, push_below=below), lb=D), INVALID, "insert_waypoints: push and push_below must be finite")
    add(entry, ins(longest, lb=D), INVALID, "insert_waypoints: lb and ub go together")
    add(entry, ins(longest, ub=D, lb_out=D, ub_out=D), INVALID, "insert_waypoints: lb and ub go together")
    for outs in ((None, None), (D, None), (None, D)):
        add(entry, ins(longest, lb=D, ub=D, lb_out=outs[0], ub_out=outs[1]), INVALID, I_OUT)
    add(entry, ins(longest, lb_out=D, ub_out=D), INVALID, I_OUT)
    for bad in (dict(bos=-1.0), dict(vos=INF), dict(aos=NAN)):
        add(entry, ins(Insert(**bad), m=1, lb=D, ub=D, lb_out=D, ub_out=D), INVALID,
            "insert_waypoints: bos, vos and aos must be finite and >= 0")
        # (no bounds given: not looked at)
        add(entry, ins(Insert(**bad), b=0, x=None, coeff=None, T=None, when=None, x_out=None, T_out=None), OK)
    for o in (longest, at_time):
        for bad in (dict(b=-1), dict(m=1), dict(m=227), dict(ts=1)):
            add(entry, ins(o, ws=0, **bad), INVALID, I_NEED)
        add(entry, ins(o, b=0, ts=0, x=None, coeff=None, T=None, when=None, x_out=None, T_out=None), OK)
        for missing in ("x", "coeff", "T", "x_out", "T_out"):
            add(entry, ins(o, **{missing: None}), INVALID, I_BUF)
    for ws in (0, -1):
        add(entry, ins(at_time, ws=ws, x=None), INVALID, "insert_waypoints: AT_TIME needs when_stride >= 1")
    add(entry, ins(longest, ws=0, when=None, x=None), INVALID, I_BUF)      # (LONGEST reads neither `when` nor its stride)
    add(entry, ins(at_time, when=None), INVALID, I_BUF)
    add(entry, ins(Insert(push=0.1), x=None), *((INVALID, I_BUF) if have_field else (STATE, NO_FIELD)))
    # -- the box lists and the start times
    add("gtop_set_moving_boxes", (-1, H, H, H), INVALID, "set_moving_boxes: bad box list")
    for nulls in ((None, H, H), (H, None, H), (H, H, None)):
        add("gtop_set_moving_boxes", (1, *nulls), INVALID, "set_moving_boxes: bad box list")
    add("gtop_set_moving_box_polynomials", (-1, H, None, H), INVALID, "set_moving_box_polynomials: bad box list")
    add("gtop_set_moving_box_polynomials", (1, None, None, H), INVALID, "set_moving_box_polynomials: bad box list")
    add("gtop_set_moving_box_polynomials", (1, H, None, None), INVALID, "set_moving_box_polynomials: bad box list")
    coef_inf, scale_bad = np.zeros(18), np.array([1.0, -1.0, 1.0])
    coef_inf[17] = INF
    e.keep = [coef_inf, scale_bad, np.array([1.0, 0.0]), np.array([0.0, NAN]), np.array([-1.0]), np.array([0.0, INF])]
    add("gtop_set_moving_box_polynomials", (1, hp(coef_inf), None, H), INVALID, "box polynomials: a coefficient is not finite")
    add("gtop_set_moving_box_polynomials", (1, H, hp(e.keep[2]), hp(scale_bad)), INVALID,
        "box polynomials: need t1 <= t2, neither NaN")
    add("gtop_set_moving_box_polynomials", (1, H, hp(e.keep[3]), H), INVALID, "box polynomials: need t1 <= t2, neither NaN")
    add("gtop_set_moving_box_polynomials", (1, H, None, hp(scale_bad)), INVALID, "box polynomials: scale must be finite and >= 0")
    add("gtop_set_start_times", (-1, H), INVALID, "set_start_times: count < 0")
    add("gtop_set_start_times", (-1, None), INVALID, "set_start_times: count < 0")
    add("gtop_set_start_times", (1, hp(e.keep[4])), INVALID, "set_start_times: start times must be finite and >= 0")
    add("gtop_set_start_times", (2, hp(e.keep[5])), INVALID, "set_start_times: start times must be finite and >= 0")
    add("gtop_set_start_times_device", (-1, D), INVALID, "set_start_times_device: count < 0")
    # -- the distance queries.  Device forms: the field, N, N == 0, the buffers; host forms: N and the buffers in one text
    for entry, who, coarse in (("gtop_edt_query_device", "edt_query", False),
                               ("gtop_edt_coarse_query_device", "edt_coarse_query", True)):
        tail = (None,) if coarse else (D, None)      # (grad,) stream
        if not have_field:
            add(entry, (-1, D, D, D, *tail), STATE, NO_FIELD)
            continue
        add(entry, (-1, D, D, D, *tail), INVALID, who + ": N < 0")
        add(entry, (0, None, None, None, *((None,) * len(tail))), OK)
        for nulls in ((None, D, D), (D, None, D), (D, D, None)):
            add(entry, (1, *nulls, *tail), INVALID, who + ": NULL buffer")
    if have_field:
        add("gtop_edt_query_device", (1, D, D, D, None, None), INVALID, "edt_query: NULL buffer")
    for entry, who, coarse in (("gtop_edt_query", "edt_query", False), ("gtop_edt_coarse_query", "edt_coarse_query", True)):
        tail = () if coarse else (H,)
        add(entry, (-1, H, H, H, *tail), INVALID, who + ": bad arguments")
        for nulls in ((None, H, H), (H, None, H), (H, H, None)):
            add(entry, (1, *nulls, *tail), INVALID, who + ": bad arguments")
        add(entry, (0, None, None, None, *((None,) * len(tail))), OK)
        if not have_field:
            add(entry, (1, H, H, H, *tail), STATE, NO_FIELD)
    add("gtop_edt_query", (1, H, H, H, None), INVALID, "edt_query: bad arguments")
    return rows


def host_rows(e, have_problem):
    """The host forms over the problem set.  have_problem False: every one of them answers GTOP_ERR_STATE first,
    whatever else is wrong with the call."""
    H = e.H
    lim = Limits()
    length, limits_mode = Retime(mode=0), Retime(mode=1)
    longest, at_time = Insert(mode=1), Insert(mode=0)
    rows = []

    def add(entry, args, status, text):
        rows.append((entry, args, *((status, text) if have_problem else (STATE, NO_PROBLEM))))

    def ins(o, b=B, x=H, when=None, lb=None, ub=None, x_out=H, T_out=H, lb_out=None, ub_out=None, info=None):
        return (ref(o), b, x, when, lb, ub, x_out, T_out, lb_out, ub_out, info)

    for b, x, out in ((0, H, H), (-1, H, H), (B + 1, H, H), (B, None, H), (B, H, None)):
        add("gtop_validate_batch", (b, x, 0.0, None, None, out, None, None), INVALID, VB_ROWS)
        add("gtop_validate_segments", (b, x, 0.0, None, out), INVALID, VS_ROWS)
        add("gtop_certify_batch", (b, x, None, out), INVALID, CB_ROWS)
        add("gtop_certify_moving_batch", (b, x, None, out), INVALID, CMB_ROWS)
        add("gtop_reallocate_times", (ref(length), b, x, 0.0, None, out), INVALID, R_ROWS)
        add("gtop_reallocate_times", (ref(limits_mode), b, x, 0.0, None, out), INVALID, R_ROWS)
        add("gtop_reallocate_times", (None, b, x, 0.01, ref(lim), out), INVALID, R_NULL)          # the options come first
        add("gtop_reallocate_times", (ref(Retime(mode=5)), b, x, 0.01, ref(lim), out), INVALID, "reallocate_times: unknown mode")
        if b >= 0:
            add("gtop_insert_waypoints", ins(longest, b=b, x=x, x_out=out), INVALID, I_ROWS)
            add("gtop_insert_waypoints", ins(longest, b=b, x=x, T_out=out), INVALID, I_ROWS)
        add("gtop_insert_waypoints", ins(None, b=b, x=x, x_out=out), INVALID, "insert_waypoints: options is NULL")   # likewise
        add("gtop_insert_waypoints", ins(Insert(min_fraction=0.6), b=b, x=x, x_out=out), INVALID, I_FRACTION)
        add("gtop_trajectory_samples", (b, x, 0.01, out, None, None, 0), INVALID, TS_ROWS)
    add("gtop_insert_waypoints", ins(longest, b=-1), INVALID, I_NEED)      # (the shape rules speak before the rows' text)
    add("gtop_insert_waypoints", ins(at_time, when=None), INVALID, I_ROWS)
    add("gtop_insert_waypoints", ins(longest, lb=H), INVALID, "insert_waypoints: lb and ub go together")
    add("gtop_insert_waypoints", ins(longest, lb=H, ub=H), INVALID, I_OUT)
    add("gtop_insert_waypoints", ins(Insert(reserved=1)), INVALID, "insert_waypoints: reserved must be 0")
    add("gtop_trajectory_samples", (B, H, 0.01, None, None, None, 0), INVALID, TS_ROWS)
    add("gtop_trajectory_samples", (B, H, 0.01, H, None, None, -1), INVALID, TS_ROWS)
    add("gtop_trajectory_samples", (B, H, 0.01, None, None, H, 0), INVALID, TS_ROWS)
    add("gtop_validate_batch", (B, H, 0.0, None, None, H, None, None), INVALID, "validate_batch: dt_sample must be > 0")
    add("gtop_validate_batch", (B, H, NAN, ref(lim), None, H, None, None), INVALID, "validate_batch: dt_sample must be > 0")
    add("gtop_validate_batch", (B, H, 0.01, None, None, H, None, None), INVALID, V_NULL_LIMITS)
    add("gtop_validate_batch", (B, H, 0.01, ref(Limits(max_acc=NAN)), None, H, None, None), INVALID, V_FINITE)
    add("gtop_validate_segments", (B, H, 0.0, None, H), INVALID, V_NEED)
    add("gtop_validate_segments", (B, H, 0.01, None, H), INVALID, V_NULL_LIMITS)
    add("gtop_validate_segments", (B, H, 0.01, ref(Limits(margin=INF)), H), INVALID, V_FINITE)
    add("gtop_certify_batch", (B, H, None, H), INVALID, C_NULL)
    add("gtop_certify_batch", (B, H, ref(Opts(0.1, 4, 4)), H), INVALID, C_OPTS)
    add("gtop_certify_moving_batch", (B, H, None, H), INVALID, CM_NULL)
    add("gtop_certify_moving_batch", (B, H, ref(MovingOpts(0.1, 4, 4, True, 1)), H), INVALID, CM_RESERVED)
    add("gtop_certify_moving_batch", (B, H, ref(MovingOpts(0.1, 1, -1, False)), H), INVALID, C_OPTS)
    add("gtop_reallocate_times", (ref(Retime(mode=0, mean_v=-1.0)), B, H, 0.01, None, H), INVALID, R_LENGTH)
    add("gtop_reallocate_times", (ref(Retime(mode=1, max_ratio=0.0)), B, H, 0.01, None, H), INVALID, R_LIMITS)
    add("gtop_reallocate_times", (ref(limits_mode), B, H, 0.0, ref(lim), H), INVALID, V_NEED)
    add("gtop_reallocate_times", (ref(limits_mode), B, H, 0.01, None, H), INVALID, V_NULL_LIMITS)
    add("gtop_reallocate_times", (ref(limits_mode), B, H, 0.01, ref(Limits(max_vel=INF)), H), INVALID, V_FINITE)
    return rows


def check(e, rows):
    bad = []
    for entry, args, status, text in rows:
        rc, err = e.call(entry, *args)
        if rc != status or (text is not None and err != text):
            bad.append((entry, rc, err, "expected", status, text))
    assert not bad, "\n".join(map(repr, bad))
    return len(rows)


def test_refusals_and_the_order_of_the_checks(env):
    e = env
    L = e.L
    # every entry of the three files, and gtop_trajectory_samples, with no context: GTOP_ERR_INVALID and nothing else
    z = {C.c_int: 0, C.c_double: 0.0}
    for name in ("gtop_set_moving_boxes", "gtop_set_moving_box_polynomials", "gtop_get_moving_box_kind", "gtop_set_moving_cost",
                 "gtop_get_moving_cost", "gtop_set_start_times", "gtop_set_start_times_device", "gtop_edt_query_device",
                 "gtop_edt_query", "gtop_edt_coarse_query_device", "gtop_edt_coarse_query",
                 "gtop_validate_trajectories_device", "gtop_select_best_device", "gtop_validate_batch",
                 "gtop_validate_segments_device", "gtop_validate_segments", "gtop_certify_trajectories_device",
                 "gtop_certify_batch", "gtop_certify_moving_device", "gtop_certify_moving_batch",
                 "gtop_select_best_certified_device", "gtop_reallocate_times_device", "gtop_reallocate_times",
                 "gtop_insert_waypoints_device", "gtop_insert_waypoints", "gtop_trajectory_samples"):
        args = [z.get(t) for t in _abi.ENTRY_POINTS[name][2][1:]]
        assert getattr(L, name)(None, *args) == INVALID, name
    kind, count = C.c_int(-7), C.c_int(-7)
    assert e.call("gtop_get_moving_box_kind", None, C.byref(count))[0] == INVALID
    assert e.call("gtop_get_moving_box_kind", C.byref(kind), None)[0] == INVALID
    assert e.call("gtop_get_moving_cost", None)[0] == INVALID
    # gtop_box_polynomial_centres has no context: a status alone
    one, coef_inf = np.zeros(18), np.full(18, INF)
    for args in ((-1, hp(one), None, 1, e.H, e.H), (1, hp(one), None, -1, e.H, e.H), (1, None, None, 1, e.H, e.H),
                 (1, hp(one), None, 1, None, e.H), (1, hp(one), None, 1, e.H, None), (1, hp(coef_inf), None, 1, e.H, e.H),
                 (1, hp(one), hp(np.array([2.0, 1.0])), 1, e.H, e.H)):
        assert L.gtop_box_polynomial_centres(*args) == INVALID, args
    assert L.gtop_box_polynomial_centres(0, None, None, 0, None, None) == OK

    # a context with neither a field nor a problem
    n = check(e, device_rows(e, have_field=False)) + check(e, host_rows(e, have_problem=False))
    e.make_ready()
    n += check(e, device_rows(e, have_field=True)) + check(e, host_rows(e, have_problem=True))
    print(f"{n} refused or empty calls")

    # a refused list leaves the one in force
    e.ctx.set_moving_boxes(np.zeros((2, 3)), np.zeros((2, 3)), np.ones((2, 3)))
    n += check(e, [r for r in device_rows(e, True) if r[0].startswith("gtop_set_moving_box")])
    assert e.call("gtop_get_moving_box_kind", C.byref(kind), C.byref(count))[0] == OK and (kind.value, count.value) == (0, 2)

    # the moving-obstacle cost's own checks (gtop_moving_args), reached through an evaluation in moving mode
    D = e.D
    evaluate = ("gtop_eval_device", (_abi.GTOP_F64, B, M, D, D, D, M, D, D, None))
    e.ctx.set_moving_cost(True)
    e.ctx.set_moving_boxes(np.zeros((33, 3)), np.zeros((33, 3)), np.ones((33, 3)))
    check(e, [(*evaluate, INVALID, "moving-obstacle cost: more boxes set than GTOP_MOVING_COST_MAX_BOXES")])
    e.ctx.set_moving_boxes(np.zeros((1, 3)), np.zeros((1, 3)), -np.ones((1, 3)))
    check(e, [(*evaluate, INVALID, "moving-obstacle cost: the box list has a non-finite value or a negative extent")])
    e.ctx.set_moving_boxes(np.zeros((1, 3)), np.zeros((1, 3)), np.ones((1, 3)))
    e.ctx.set_start_times([0.0, 1.0, 2.0])
    check(e, [(*evaluate, INVALID, MOV_T0)])
    e.ctx.set_moving_cost(False)
    e.ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))

    # three start times for two rows: whoever looks at the list refuses, with boxes or without
    H, lim, box_lim = e.H, Limits(), Limits(use_boxes=True)
    for o in (MovingOpts(0.1, 1, 4, False), MovingOpts(0.1, 1, 4, True)):
        check(e, [("gtop_certify_moving_device", (B, M, D, D, M, ref(o), D, None), INVALID, CM_T0),
                  ("gtop_certify_moving_device", (0, M, None, None, 0, ref(o), None, None), INVALID, CM_T0),
                  ("gtop_certify_moving_batch", (B, H, ref(o), H), INVALID, CM_T0),
                  ("gtop_certify_moving_batch", (1, H, ref(o), H), INVALID, CM_T0)])
    for o in (lim, box_lim):
        check(e, [("gtop_validate_trajectories_device", (B, M, D, D, M, 0.01, ref(o), D, None), INVALID, V_T0),
                  ("gtop_validate_segments_device", (B, M, D, D, M, 0.01, ref(o), D, None), INVALID, V_T0),
                  ("gtop_validate_batch", (B, H, 0.01, ref(o), None, H, None, None), INVALID, V_T0),
                  ("gtop_validate_segments", (B, H, 0.01, ref(o), H), INVALID, V_T0),
                  ("gtop_reallocate_times", (ref(Retime(mode=1)), B, H, 0.01, ref(o), H), INVALID, V_T0)])
    # (3 = B: the list fits a device call of three rows, and the next check speaks)
    check(e, [("gtop_certify_moving_device", (3, M, None, D, M, ref(MovingOpts(0.1, 1, 4, False)), D, None), INVALID,
               "certify_moving: NULL buffer"),
              ("gtop_validate_trajectories_device", (3, M, None, D, M, 0.01, ref(lim), D, None), INVALID, "validate: NULL buffer")])
    e.ctx.set_start_times(None)


@pytest.fixture(scope="module")
def problem(env):
    """x, and the problem's coefficients as coefficients_device forms them; the context clean of boxes and start times"""
    e = env
    if not hasattr(e, "x0"):
        e.make_ready()
    e.ctx.set_moving_cost(False)
    e.ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    e.ctx.set_start_times(None)
    rng = np.random.default_rng(5)
    x = e.x0 + 0.05 * rng.standard_normal(e.x0.shape)
    T, Df = e.ctx.get_problem()
    coeff = e.ctx.coefficients_device(e.dev(x), e.dev(Df.reshape(B, 18)), e.dev(T))
    e.torch.cuda.synchronize()
    return x, coeff, e.dev(T)


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else (np.int32 if a.dtype.itemsize == 4 else np.int64))


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def test_the_static_certificate_ignores_the_start_times(env, problem):
    e = env
    x, coeff, T = problem
    opts = Opts(0.1, 2, 16)
    dev0 = certify.certify_device(e.ctx, coeff, T, opts)
    host0 = certify.certify_batch(e.ctx, x, opts)
    e.torch.cuda.synchronize()
    assert same_bits(dev0, host0) and np.all(np.isfinite(host0[:, 7])) and np.all(host0[:, 7] > 0)
    e.ctx.set_start_times([0.5, 1.0, 1.5])          # 3 for 2 rows: does not fit
    try:
        dev3 = certify.certify_device(e.ctx, coeff, T, opts)
        host3 = certify.certify_batch(e.ctx, x, opts)
        e.torch.cuda.synchronize()
        assert same_bits(dev3, dev0) and same_bits(host3, host0)
        with pytest.raises(e.gtop.GtopError) as err:
            certify.certify_moving_device(e.ctx, coeff, T, MovingOpts(0.1, 2, 16, False))
        assert (err.value.code, str(err.value)) == (INVALID, "GTOP_ERR_INVALID: " + CM_T0)
        with pytest.raises(e.gtop.GtopError) as err:
            e.ctx.validate_device(coeff, T, Limits(use_boxes=False))
        assert (err.value.code, str(err.value)) == (INVALID, "GTOP_ERR_INVALID: " + V_T0)
    finally:
        e.ctx.set_start_times(None)


def test_the_merged_paths_agree_bit_for_bit(env, problem):
    e = env
    torch = e.torch
    x, coeff, T = problem
    # (a) the static host certificate and the moving one with the boxes off, under a start-time list that fits
    e.ctx.set_start_times([0.5, 1.0])
    try:
        for margin, depth, refine in ((0.1, 2, 16), (0.3, 0, 0)):
            a = certify.certify_batch(e.ctx, x, Opts(margin, depth, refine))
            b = certify.certify_moving_batch(e.ctx, x, MovingOpts(margin, depth, refine, False))
            assert same_bits(a, b), (margin, depth, refine)
    finally:
        e.ctx.set_start_times(None)
    # (b) the two selections on one report, every certificate row SAFE: a limit between the two rows' top speeds
    report = e.ctx.validate_device(coeff, T, Limits(margin=0.05, allow_out_of_map=True))
    cert = certify.certify_device(e.ctx, coeff, T, Opts(0.05, 2, 16))
    cert[:, 0] = certify.SAFE
    top = report[:, 7].cpu().numpy()
    assert top[0] != top[1]
    cost = e.dev([2.0, 1.0])
    for max_vel, passing in ((0.5 * (top[0] + top[1]), 1), (0.0, 2), (0.5 * top.min(), 0)):
        lim = Limits(margin=0.05, max_vel=max_vel, allow_out_of_map=True)
        ok0, best0 = e.ctx.select_best_device(report, cost, lim)
        for require in (certify.REQUIRE_SAFE, certify.REQUIRE_NOT_UNSAFE):
            ok1, best1 = certify.select_best_certified_device(e.ctx, report, cert, cost, lim, require)
            torch.cuda.synchronize()
            assert same_bits(ok0, ok1) and same_bits(best0, best1)
        if float(report[:, 4].sum()) == 0.0:       # (no sample below the margin: the count is the speed limit's alone)
            assert int(best0[1]) == passing
    # B = 0 needs `best` alone and answers {-1, 0}
    best = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    assert e.call("gtop_select_best_device", 0, None, None, ref(Limits()), None, best.data_ptr(), None)[0] == OK
    torch.cuda.synchronize()
    assert best.tolist() == [-1, 0]
    best.fill_(7)
    assert e.call("gtop_select_best_certified_device", 0, None, None, None, ref(Limits()), 1, None, best.data_ptr(), None)[0] == OK
    torch.cuda.synchronize()
    assert best.tolist() == [-1, 0]
    # (c) one coefficient staging: gtop_trajectory_samples' coefficients are coefficients_device's on the same x, and
    # gtop_validate_batch's report is validate_device's on them
    host_coeff, stats = np.empty((B, M, 18)), np.empty((B, 9))
    assert e.call("gtop_trajectory_samples", B, hp(x), 0.01, hp(host_coeff), hp(stats), None, 0)[0] == OK
    assert same_bits(host_coeff, coeff)
    lim = Limits(margin=0.05, allow_out_of_map=True)
    host_report, _, _ = e.ctx.validate_batch(x, lim)
    torch.cuda.synchronize()
    assert same_bits(host_report, report)
    seg_host = e.ctx.validate_segments(x, lim)
    seg_dev = e.ctx.validate_segments_device(coeff, T, lim)
    torch.cuda.synchronize()
    assert same_bits(seg_host, seg_dev)
    # the insertion's host form stages the same coefficients: its rows are the device form's
    o = Insert(mode=1)
    x_out, T_out = np.empty((B, 9 * M)), np.empty((B, M + 1))
    assert e.call("gtop_insert_waypoints", ref(o), B, hp(x), None, None, None, hp(x_out), hp(T_out), None, None, None)[0] == OK
    dx, dT, _, _, _ = insert.insert_waypoints_device(e.ctx, o, e.dev(x), coeff, T)
    torch.cuda.synchronize()
    assert same_bits(x_out, dx) and same_bits(T_out, dT)
