"""grad_traj_optimization_amd.certify against a recording stub library, without a GPU: the harness of
tests/test_binding_args.py (a GtopContext over a stub that records every call, stand-in tensors) applied to the
functions of the new module — the call that reaches the library argument by argument, the one stream rule, the refusals
of GtopContext._dev before anything is called, and what is allocated for an output the caller leaves out."""
import types

import numpy as np
import pytest
import torch

from grad_traj_optimization_amd import _abi, certify
from tests.test_binding_args import (B, DEFECTS, F64, HANDLE, I32, LIMITS, M, STREAM, T_FORMS, U8, FakeTensor,  # noqa: F401
                                     allocations, make_context, p, t)

OPTS = certify.GtopCertifyOpts(0.25, 2, 64)


def certify_args(t_shape=(B, M), **kw):
    return dict(dict(coeff=t("coeff", (B, M, 18)), T=t("T", t_shape), opts=OPTS, cert=t("cert", (B, 8))), **kw)


def select_args(**kw):
    return dict(dict(report=t("report", (B, 12)), cert=t("cert", (B, 8)), cost=t("cost", (B,)), limits=LIMITS,
                     require=certify.REQUIRE_NOT_UNSAFE, best=t("best", (2,), I32)), **kw)


def test_options_structure_and_constants():
    assert [(n, c) for n, c in certify.GtopCertifyOpts._fields_] == [
        ("margin", _abi.C.c_double), ("max_depth", _abi.C.c_int32), ("max_refine", _abi.C.c_int32)]
    o = certify.GtopCertifyOpts()
    assert (o.margin, o.max_depth, o.max_refine) == (0.0, 2, 256)
    assert (OPTS.margin, OPTS.max_depth, OPTS.max_refine) == (0.25, 2, 64)
    assert len(certify.CERT_REPORT) == 8 and (certify.REQUIRE_SAFE, certify.REQUIRE_NOT_UNSAFE) == (1, 2)
    names = {"gtop_certify_trajectories_device", "gtop_certify_batch", "gtop_select_best_certified_device"}
    assert {n for n, (since, _, _) in _abi.ENTRY_POINTS.items() if since == 10} == names
    assert all(_abi.ENTRY_POINTS[n][0] == 10 for n in names) and _abi.ABI_VERSION >= 10
    assert not names & set(_abi.entry_points(9)) and set(_abi.entry_points(10)) - set(_abi.entry_points(9)) == names


@pytest.mark.parametrize("t_shape,stride", T_FORMS)
def test_certify_device_call_record_and_stream_rule(t_shape, stride, allocations):
    for given, arrives in ((STREAM, STREAM), (types.SimpleNamespace(cuda_stream=12345), 12345)):
        ctx = make_context()
        out = certify.certify_device(ctx, stream=given, **certify_args(t_shape))
        assert out.name == "cert"
        assert ctx._L.calls == [("gtop_certify_trajectories_device",
                                 (HANDLE, B, M, p("coeff"), p("T"), stride, OPTS, p("cert"), arrives))]
    assert allocations == []


def test_select_best_certified_device_call_record(allocations):
    ctx = make_context()
    ok, best = certify.select_best_certified_device(ctx, stream=STREAM, **select_args())
    assert ctx._L.calls == [("gtop_select_best_certified_device",
                             (HANDLE, B, p("report"), p("cert"), p("cost"), LIMITS, 2, p("new0"), p("best"), STREAM))]
    assert [(fn, shape, dtype) for fn, shape, dtype, _ in allocations] == [("empty", (B,), U8)]
    assert ok.name == "new0" and best.name == "best"
    ctx = make_context()
    del allocations[:]
    ok, best = certify.select_best_certified_device(ctx, stream=STREAM, **select_args(want_pass=False, best=None,
                                                                                       require=certify.REQUIRE_SAFE))
    assert ctx._L.calls == [("gtop_select_best_certified_device",
                             (HANDLE, B, p("report"), p("cert"), p("cost"), LIMITS, 1, None, p("new0"), STREAM))]
    assert ok is None and [(fn, shape, dtype) for fn, shape, dtype, _ in allocations] == [("empty", (2,), I32)]


def test_an_output_left_out_is_allocated(allocations):
    ctx = make_context()
    out = certify.certify_device(ctx, stream=STREAM, **certify_args(cert=None))
    assert [(fn, shape, dtype, dev) for fn, shape, dtype, dev in allocations] == [
        ("empty", (B, 8), F64, torch.device("cuda", 0))]
    (_, received), = ctx._L.calls
    assert received[7] == p("new0") and out.name == "new0"


@pytest.mark.parametrize("fn,args", [(certify.certify_device, certify_args), (certify.select_best_certified_device,
                                                                             select_args)])
def test_refusals(fn, args, allocations):
    tried = 0
    for name, value in args().items():
        if not isinstance(value, FakeTensor):
            continue
        for defect, spoil in DEFECTS.items():
            ctx = make_context()
            with pytest.raises(ValueError):
                fn(ctx, stream=STREAM, **dict(args(), **{name: spoil(value)}))
            assert ctx._L.calls == [], (name, defect)
            tried += 1
    assert tried >= 15
    ctx = make_context()
    with pytest.raises(ValueError):
        certify.certify_device(ctx, t("coeff", (B, M, 17)), t("T", (B, M)), OPTS, stream=STREAM)
    assert ctx._L.calls == []


def test_certify_batch_call_record():
    ctx = make_context()
    x = np.arange(B * 18, dtype=np.float64).reshape(B, 18)
    out = certify.certify_batch(ctx, x, OPTS)
    (entry, received), = ctx._L.calls
    assert entry == "gtop_certify_batch" and received[:2] == (HANDLE, B) and received[3] is OPTS
    assert received[2] == (0.0, 1.0, 2.0) and out.shape == (B, 8)
