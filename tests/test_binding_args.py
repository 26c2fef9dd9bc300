"""The Python binding's rules for device arguments, without a GPU and without the library: a GtopContext made with
object.__new__ over a stub library that records every call, driven with stand-in tensors.

What is checked, for every method that hands a tensor's address to the library (the seventeen with a `stream`
parameter, set_sdf_device and set_start_times_device):
  1. the call that reaches the library, argument by argument (written from what the binding did before its device
     rules were stated once: the same harness passes against that file, but for the stream forms it refused);
  2. the one stream rule: a handle arrives as it is, an object with .cuda_stream as that attribute;
  3. the refusals: a host tensor, another device, a non-contiguous tensor, another dtype and a tensor one element
     short each raise ValueError before anything is called;
  4. what is allocated for an output the caller leaves out;
  5. the table of entry points and the selection by ABI version."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

from grad_traj_optimization_amd import _abi
from grad_traj_optimization_amd._lib import GTOP_F32, GTOP_F64, GtopContext, GtopLimits, GtopRetime, GtopStop

B, M, N = 3, 3, 18          # trajectories, segments, free variables 9 (M - 1)
HANDLE, STREAM = 0xABC, 777
F64, F32, I64, I32, U8 = torch.float64, torch.float32, torch.int64, torch.int32, torch.uint8
T_FORMS = (((M,), 0), ((B, M), M))      # (shape of T, time stride): shared by the batch, or one row per trajectory

_addresses = {}


def p(name):
    """The fake address of the tensor called `name`."""
    return _addresses.setdefault(name, 0x10000 * (len(_addresses) + 1))


class FakeTensor:
    def __init__(self, name, shape, dtype=F64, device=torch.device("cuda", 0), contiguous=True):
        self.name, self.shape, self.dtype, self.device, self._contiguous = name, tuple(shape), dtype, device, contiguous
        self.is_cuda = device.type == "cuda"

    def get_device(self):
        return self.device.index if self.is_cuda else -1

    def dim(self):
        return len(self.shape)

    def numel(self):
        return math.prod(self.shape)

    def element_size(self):
        return self.dtype.itemsize

    def is_contiguous(self):
        return self._contiguous

    def contiguous(self):
        return self if self._contiguous else FakeTensor(self.name, self.shape, self.dtype, self.device)

    def data_ptr(self):
        return p(self.name)


def t(name, shape, dtype=F64):
    return FakeTensor(name, shape, dtype)


DEFECTS = {
    "host": lambda a: FakeTensor(a.name, a.shape, a.dtype, torch.device("cpu")),
    "device": lambda a: FakeTensor(a.name, a.shape, a.dtype, torch.device("cuda", 1)),
    "noncontiguous": lambda a: FakeTensor(a.name, a.shape, a.dtype, a.device, contiguous=False),
    "dtype": lambda a: FakeTensor(a.name, a.shape, torch.float16, a.device),
    "short": lambda a: FakeTensor(a.name, (a.numel() - 1,), a.dtype, a.device),
}
# The defects that are none, by case: pts is made contiguous by the binding itself; the library reads as many start
# times as t0 has, and as many bytes of src as nbytes says (all of src without nbytes), whatever src's dtype.
NOT_A_DEFECT = {("update_sdf_map_device", "pts", "noncontiguous"), ("update_sdf_map_window_device", "pts", "noncontiguous"),
                ("set_start_times_device", "t0", "short"), ("push_rows", "src", "dtype"),
                ("push_rows[whole]", "src", "dtype"), ("push_rows[whole]", "src", "short")}


def _norm(a):
    """An argument as the stub library received it, in a form that compares."""
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C.POINTER(C.c_double)):
        return tuple(a[:3])                     # origin, map_size, min_pos, max_pos: three doubles each
    if isinstance(a, C.Array):
        return list(a)
    if type(a).__name__ == "CArgObject":        # C.byref(structure)
        a = a._obj
        return ("stop", a.max_evals, a.ftol_rel, a.xtol_rel, a.maxtime) if isinstance(a, GtopStop) else a
    return a


class StubLibrary:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gtop_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, tuple(_norm(a) for a in args)))
            return 0
        return entry


def make_context():
    ctx = object.__new__(GtopContext)
    ctx._L, ctx._h, ctx.device, ctx.B, ctx.m = StubLibrary(), C.c_void_p(HANDLE), 0, B, M
    return ctx


@pytest.fixture
def allocations(monkeypatch):
    """torch.empty / torch.zeros replaced: the tensors the binding allocates are stand-ins 'new0', 'new1', ... and
    every allocation is listed as (function, shape, dtype, device)."""
    made = []

    def maker(fn):
        def make(*size, dtype=None, device=None):
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list)) else size
            made.append((fn, shape, dtype, device))
            return FakeTensor(f"new{len(made) - 1}", shape, dtype, device)
        return make
    monkeypatch.setattr(torch, "empty", maker("empty"))
    monkeypatch.setattr(torch, "zeros", maker("zeros"))
    return made


class Case:
    """One call: the method, its good arguments (a function, so that every use gets fresh ones), the outputs among
    them that may be left out with what is then allocated, the entry point and the arguments it must receive but for
    the stream, which is the last."""

    def __init__(self, method, args, entry, expect, outputs=None, label=""):
        self.method, self.args, self.entry, self.expect, self.outputs = method, args, entry, expect, outputs or {}
        self.id = method + label
        code = GtopContext.__dict__[method].__code__
        self.has_stream = "stream" in code.co_varnames[:code.co_argcount]

    def call(self, ctx, args, stream=STREAM):
        if self.has_stream:
            args = dict(args, stream=stream)
        return getattr(ctx, self.method)(**args)


LIMITS = GtopLimits(margin=0.3)
RETIME_LIMITS, RETIME_LENGTH = GtopRetime(mode=1, max_vel=2.0), GtopRetime(mode=0)


def _cases():
    h = HANDLE
    out = [
        Case("set_sdf_device", lambda: dict(tensor=t("field", (4, 3, 2)), grid=(4, 3, 2), origin=(0.0, 1.0, 2.0),
                                            resolution=0.5, map_size=(2.0, 1.5, 1.0)),
             "gtop_set_sdf_device", (h, GTOP_F64, p("field"), 4, 3, 2, (0.0, 1.0, 2.0), (2.0, 1.5, 1.0), 0.5)),
        Case("set_sdf_device", lambda: dict(tensor=t("field", (24,), F32), grid=(4, 3, 2), origin=(0.0, 1.0, 2.0),
                                            resolution=0.5),
             "gtop_set_sdf_device", (h, GTOP_F32, p("field"), 4, 3, 2, (0.0, 1.0, 2.0), None, 0.5), label="[f32]"),
        Case("set_start_times_device", lambda: dict(t0=t("t0", (B,))), "gtop_set_start_times_device", (h, B, p("t0"))),
        Case("update_sdf_map_device", lambda: dict(pts=t("pts", (5, 3))), "gtop_update_sdf_map_device", (h, p("pts"), 5)),
        Case("update_sdf_map_window_device", lambda: dict(min_pos=(0.0, 0.5, 1.0), max_pos=(2.0, 2.5, 3.0),
                                                          pts=t("pts", (5, 3))),
             "gtop_update_sdf_map_window_device", (h, (0.0, 0.5, 1.0), (2.0, 2.5, 3.0), p("pts"), 5)),
        Case("push_rows", lambda: dict(src=t("src", (8,)), dst_ptrs=[0x5000, 0x6000], nbytes=64,
                                       clock_minmax=t("minmax", (2,), I64)),
             "gtop_push_rows", (h, p("src"), 64, [0x5000, 0x6000], 2, p("minmax"))),
        Case("push_rows", lambda: dict(src=t("src", (8,), F32), dst_ptrs=[0x5000]),
             "gtop_push_rows", (h, p("src"), 32, [0x5000], 1, None), label="[whole]"),
        Case("clock_stamp", lambda: dict(minmax=t("minmax", (2,), I64)), "gtop_device_clock_stamp", (h, p("minmax"))),
        Case("edt_query_device", lambda: dict(pos=t("pos", (4, 3)), time=t("time", (4,))),
             "gtop_edt_query_device", (h, 4, p("pos"), p("time"), p("new0"), p("new1"))),
        Case("edt_coarse_query_device", lambda: dict(pos=t("pos", (4, 3)), time=t("time", (4,))),
             "gtop_edt_coarse_query_device", (h, 4, p("pos"), p("time"), p("new0"))),
        Case("setup_paths_device", lambda: dict(waypoints=t("waypoints", (B, M + 1, 3)), mean_v=1.5, init_time=0.25,
                                                T=t("T", (B, M)), Df=t("Df", (B, 18)), x0=t("x0", (B, N))),
             "gtop_setup_paths_device", (h, B, M, p("waypoints"), 1.5, 0.25, p("T"), p("Df"), p("x0")),
             outputs=dict(T=("empty", (B, M), F64), Df=("empty", (B, 18), F64), x0=("empty", (B, N), F64))),
        Case("select_best_device", lambda: dict(report=t("report", (B, 12)), cost=t("cost", (B,)), limits=LIMITS,
                                                best=t("best", (2,), I32)),
             "gtop_select_best_device", (h, B, p("report"), p("cost"), LIMITS, p("new0"), p("best")),
             outputs=dict(best=("empty", (2,), I32))),
        Case("select_best_device", lambda: dict(report=t("report", (B, 12)), cost=t("cost", (B,)), limits=LIMITS,
                                                want_pass=False, best=t("best", (2,), I32)),
             "gtop_select_best_device", (h, B, p("report"), p("cost"), LIMITS, None, p("best")), label="[no pass]"),
        Case("reallocate_times_device", lambda: dict(options=RETIME_LENGTH, x=t("x", (B, N)), Df=t("Df", (B, 18)),
                                                     T_out=t("T_out", (B, M))),
             "gtop_reallocate_times_device", (h, RETIME_LENGTH, B, M, p("x"), p("Df"), None, M, None, p("T_out")),
             outputs=dict(T_out=("empty", (B, M), F64)), label="[length]"),
        Case("reallocate_times_device", lambda: dict(options=RETIME_LIMITS, T=t("T", (M,)),
                                                     seg_report=t("seg_report", (B, M, 10)), T_out=t("T_out", (B, M))),
             "gtop_reallocate_times_device", (h, RETIME_LIMITS, B, M, None, None, p("T"), 0, p("seg_report"), p("T_out")),
             label="[limits, no x]"),
    ]
    for dtype, code in ((F64, GTOP_F64), (F32, GTOP_F32)):
        for shape, stride in T_FORMS:
            out.append(Case("eval_device", lambda shape=shape, dtype=dtype: dict(
                x=t("x", (B, N), dtype), Df=t("Df", (B, 18), dtype), T=t("T", shape, dtype),
                cost=t("cost", (B,), dtype), grad=t("grad", (B, N), dtype)),
                "gtop_eval_device", (h, code, B, M, p("x"), p("Df"), p("T"), stride, p("cost"), p("grad")),
                outputs=dict(cost=("empty", (B,), dtype), grad=("empty", (B, N), dtype)), label=f"[{dtype}, T{shape}]"))
    for shape, stride in T_FORMS:
        label = f"[T{shape}]"

        def problem(shape=shape, **more):
            return dict(x=t("x", (B, N)), Df=t("Df", (B, 18)), T=t("T", shape), **more)

        def trajectory(shape=shape, **more):
            return dict(coeff=t("coeff", (B, M, 18)), T=t("T", shape), **more)

        def bounds():
            return dict(lb=t("lb", (B, N)), ub=t("ub", (B, N)))
        triple, pair = (B, M, p("x"), p("Df"), p("T"), stride), (B, M, p("coeff"), p("T"), stride)
        out += [
            Case("min_jerk_start_device", problem, "gtop_min_jerk_start_device", (h, *triple), label=label),
            Case("coefficients_device", lambda problem=problem: problem(coeff=t("coeff", (B, M, 18))),
                 "gtop_coefficients_device", (h, *triple, p("coeff")),
                 outputs=dict(coeff=("empty", (B, M, 18), F64)), label=label),
            Case("optimize_device", lambda problem=problem: problem(**bounds(), max_evals=12, min_cost=t("min_cost", (B,))),
                 "gtop_optimize_device", (h, *triple, p("lb"), p("ub"), 12, p("min_cost")),
                 outputs=dict(min_cost=("empty", (B,), F64)), label=label),
            Case("optimize_device_ex", lambda problem=problem: problem(**bounds(), max_evals=12, ftol_rel=1e-3,
                                                                       xtol_rel=1e-4, maxtime=0.5),
                 "gtop_optimize_device_ex", (h, *triple, p("lb"), p("ub"), ("stop", 12, 1e-3, 1e-4, 0.5),
                                             p("new0"), p("new1"), p("new2")), label=label),
            Case("reallocate_times_device", lambda problem=problem: dict(
                options=RETIME_LIMITS, seg_report=t("seg_report", (B, M, 10)), T_out=t("T_out", (B, M)), **problem()),
                "gtop_reallocate_times_device", (h, RETIME_LIMITS, *triple, p("seg_report"), p("T_out")), label=label),
            Case("eval_trajectories_device", lambda trajectory=trajectory: trajectory(dt_sample=0.02, stats=t("stats", (B, 9))),
                 "gtop_eval_trajectories_device", (h, *pair, 0.02, p("stats")),
                 outputs=dict(stats=("empty", (B, 9), F64)), label=label),
            Case("sample_trajectories_device", lambda trajectory=trajectory: trajectory(
                dt_sample=0.02, max_samples=7, stats=t("stats", (B, 9)), samples=t("samples", (B, 7, 3))),
                "gtop_sample_trajectories_device", (h, *pair, 0.02, p("stats"), p("samples"), 7),
                outputs=dict(stats=("empty", (B, 9), F64), samples=("zeros", (B, 7, 3), F64)), label=label),
            Case("validate_device", lambda trajectory=trajectory: trajectory(limits=LIMITS, dt_sample=0.02,
                                                                            report=t("report", (B, 12))),
                 "gtop_validate_trajectories_device", (h, *pair, 0.02, LIMITS, p("report")),
                 outputs=dict(report=("empty", (B, 12), F64)), label=label),
            Case("validate_segments_device", lambda trajectory=trajectory: trajectory(
                limits=LIMITS, dt_sample=0.02, seg_report=t("seg_report", (B, M, 10))),
                "gtop_validate_segments_device", (h, *pair, 0.02, LIMITS, p("seg_report")),
                outputs=dict(seg_report=("empty", (B, M, 10), F64)), label=label),
        ]
    return out


CASES = _cases()
STREAM_CASES = [c for c in CASES if c.has_stream]
by_id = dict(ids=lambda c: c.id)


def test_the_table_covers_every_method_that_takes_a_device_tensor():
    with_stream = {name for name, f in GtopContext.__dict__.items()
                   if isinstance(f, types.FunctionType) and "stream" in f.__code__.co_varnames[:f.__code__.co_argcount]}
    assert len(with_stream) == 18
    assert {c.method for c in CASES} == with_stream | {"set_sdf_device", "set_start_times_device"}


@pytest.mark.parametrize("case", CASES, **by_id)
def test_call_record(case, allocations):
    ctx = make_context()
    case.call(ctx, case.args())
    want = case.expect + ((STREAM,) if case.has_stream else ())
    assert ctx._L.calls == [(case.entry, want)]
    assert all(fn == "empty" and device == torch.device("cuda", 0) for fn, _, _, device in allocations)
    internal = {"edt_query_device": [((4,), F64), ((4, 3), F64)], "edt_coarse_query_device": [((4,), F64)],
                "optimize_device_ex": [((B,), F64), ((B,), I32), ((B,), I32)],
                "select_best_device": [((B,), U8)] if case.args().get("want_pass", True) else []}
    assert [(shape, dtype) for _, shape, dtype, _ in allocations] == internal.get(case.method, [])


@pytest.mark.parametrize("case", STREAM_CASES, **by_id)
def test_stream_rule(case, allocations):
    for given, arrives in ((STREAM, STREAM), (types.SimpleNamespace(cuda_stream=12345), 12345)):
        ctx = make_context()
        del allocations[:]
        case.call(ctx, case.args(), stream=given)
        (_, received), = ctx._L.calls
        assert received[-1] == arrives and received[:-1] == case.expect


@pytest.mark.parametrize("case", CASES, **by_id)
def test_refusals(case, allocations):
    tried = 0
    for name, value in case.args().items():
        if not isinstance(value, FakeTensor):
            continue
        for defect, spoil in DEFECTS.items():
            if (case.id, name, defect) in NOT_A_DEFECT:
                continue
            ctx = make_context()
            with pytest.raises(ValueError):
                case.call(ctx, dict(case.args(), **{name: spoil(value)}))
            assert ctx._L.calls == [], (name, defect)
            tried += 1
    assert tried >= 3


def test_what_is_not_a_defect_is_served(allocations):
    for case_id, name, defect in sorted(NOT_A_DEFECT):
        case = next(c for c in CASES if c.id == case_id)
        ctx = make_context()
        args = case.args()
        if case_id == "push_rows":
            args["src"] = t("src", (16,), torch.float32)        # another dtype, still the 64 bytes of nbytes
        else:
            args[name] = DEFECTS[defect](args[name])
        case.call(ctx, args)
        (entry, received), = ctx._L.calls
        assert entry == case.entry
        if name == "t0":
            assert received[1] == B - 1


@pytest.mark.parametrize("case", [c for c in CASES if c.outputs], **by_id)
def test_outputs_left_out_are_allocated(case, allocations):
    """Every output the caller may leave out: the function, shape and dtype of what is allocated in its place, and that
    the new tensor's address is what the library receives where the caller's would have stood."""
    for name, (fn, shape, dtype) in case.outputs.items():
        ctx = make_context()
        args = case.args()
        given = args.pop(name)
        del allocations[:]
        case.call(ctx, args)
        new = [(i, a) for i, a in enumerate(allocations) if a[:3] == (fn, shape, dtype)]
        assert len(new) >= 1, (name, allocations)
        (_, received), = ctx._L.calls
        place = case.expect.index(p(given.name))
        assert received[place] in [p(f"new{i}") for i, _ in new]
        assert received[:place] == case.expect[:place] and received[place + 1:-1] == case.expect[place + 1:]


def test_entry_point_table():
    later = {"gtop_set_moving_cost": 4, "gtop_get_moving_cost": 4, "gtop_set_start_times": 4,
             "gtop_set_start_times_device": 4, "gtop_validate_trajectories_device": 5, "gtop_select_best_device": 5,
             "gtop_validate_batch": 5, "gtop_set_gradient_mode": 6, "gtop_get_gradient_mode": 6,
             "gtop_group_set_gradient_mode": 6, "gtop_set_moving_box_polynomials": 7, "gtop_get_moving_box_kind": 7,
             "gtop_box_polynomial_centres": 7, "gtop_min_jerk_start_device": 8, "gtop_min_jerk_start": 8,
             "gtop_validate_segments_device": 9, "gtop_validate_segments": 9, "gtop_reallocate_times_device": 9,
             "gtop_reallocate_times": 9, "gtop_certify_trajectories_device": 10, "gtop_certify_batch": 10,
             "gtop_select_best_certified_device": 10, "gtop_certify_moving_device": 11, "gtop_certify_moving_batch": 11,
             "gtop_insert_waypoints_device": 12, "gtop_insert_waypoints": 12}
    for name, entry in _abi.ENTRY_POINTS.items():
        since, restype, argtypes = entry
        assert name.startswith("gtop_") and isinstance(since, int) and since >= 0 and isinstance(argtypes, list), name
        assert since == later.get(name, 0), name
    assert _abi.ABI_VERSION == 12
    assert set(_abi.ENTRY_POINTS) - set(_abi.entry_points(3)) == set(later)
    assert set(_abi.entry_points(_abi.ABI_VERSION)) == set(_abi.ENTRY_POINTS)
    assert set(_abi.ENTRY_POINTS) - set(_abi.entry_points(8)) == {n for n, v in later.items() if v >= 9}
    for k in (9, 10, 11):
        assert set(_abi.ENTRY_POINTS) - set(_abi.entry_points(k)) == {n for n, v in later.items() if v > k}


def test_entry_point_table_is_the_header(gtop):
    """One table: every function include/gtop.h declares and no other; one version: the library's own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gtop.h")).read()
    header = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    declared = set(re.findall(r"\b(gtop_[a-z0-9_]+)\(", header))
    assert declared - set(_abi.ENTRY_POINTS) == set() and set(_abi.ENTRY_POINTS) - declared == set()
    assert len(declared) == 108
    capi = open(os.path.join(root, "grad_traj_optimization_amd", "csrc", "gtop_capi.cpp")).read()
    defined, = re.findall(r"^#define GTOP_ABI_VERSION (\d+)", capi, flags=re.M)
    assert _abi.ABI_VERSION == int(defined)
    gtop.load_library()   # (the HIP runtime it maps first; with GTOP_HIP_LIB this is another build)
    in_tree = C.CDLL(os.path.join(root, "grad_traj_optimization_amd", "libgtop_hip.so"))
    in_tree.gtop_abi_version.restype = C.c_int
    assert in_tree.gtop_abi_version() == _abi.ABI_VERSION
