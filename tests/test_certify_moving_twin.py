"""The numpy restatement of the certificate against the moving boxes (tests/certify_moving_twin.py), checked without a
GPU:

(1) the symbols, their bindings and the ABI version;
(2) soundness: lo is at most the least of 20001 evenly spaced lookups edt_query(x(t), t0 + t, boxes) along each row —
    rows of 2, 3 and 7 segments on the esdf and the signed field, three constant-velocity and three polynomial boxes
    (one braking, one that stands after its t_range ends mid-trajectory, one unbounded), t0 = 0 and 2 — and a leaf's lb
    is at most a 5^3 x 5 grid of lookups over (its curve box) x (its range of box time);
(3) the moving tunnelling case: a plate that crosses the curve between two samples of the report;
(4) five mutants of the restatement, each caught;
(5) the binding's call records against the recording stub of tests/test_binding_args.py."""
import types

import numpy as np
import pytest
import torch

from grad_traj_optimization_amd import _abi, certify
from tests import certify_moving_twin as cm
from tests import certify_twin as ct
from tests import validate_twin as vt
from tests.test_binding_args import (B, DEFECTS, F64, HANDLE, M, STREAM, T_FORMS, FakeTensor, allocations,  # noqa: F401
                                     make_context, p, t)

EPS = np.finfo(np.float64).eps
OPTS = certify.GtopCertifyMovingOpts(0.25, 2, 64)
ROWS = ((2, 42), (3, 43), (7, 47))          # (segments, seed of certify_twin.make_rows)
MARGIN, DEPTH, REFINE = 0.2, 1, 4


def test_symbols_bindings_and_abi_constants(gtop):
    lib = gtop.load_library()
    assert lib.gtop_abi_version() >= 11
    assert _abi.ABI_VERSION >= 11
    names = {"gtop_certify_moving_device", "gtop_certify_moving_batch"}
    assert {n for n, (since, _, _) in _abi.ENTRY_POINTS.items() if since == 11} == names
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert all(_abi.ENTRY_POINTS[n][0] == 11 for n in names)
    assert not names & set(_abi.entry_points(10)) and set(_abi.entry_points(11)) - set(_abi.entry_points(10)) == names
    for name in ("certify_moving_device", "certify_moving_batch", "GtopCertifyMovingOpts"):
        assert hasattr(certify, name) and hasattr(gtop, name), name
    assert [n for n, _ in certify.GtopCertifyMovingOpts._fields_] == ["margin", "max_depth", "max_refine", "use_boxes",
                                                                      "reserved"]
    o = certify.GtopCertifyMovingOpts()
    assert (o.margin, o.max_depth, o.max_refine, o.use_boxes, o.reserved) == (0.0, 2, 256, 1, 0)


# ---- (2) soundness ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields(oracle_mod):
    return {kind: ct.make_field(oracle_mod, kind) for kind in ("esdf", "signed")}


@pytest.mark.parametrize("kind", ["esdf", "signed"])
@pytest.mark.parametrize("poly", [False, True], ids=["const_vel", "polynomial"])
def test_lo_is_below_every_dense_lookup_and_leaves_are_sound(oracle_mod, fields, kind, poly):
    field, mp = fields[kind]
    boxes = cm.shared_boxes(mp, poly)
    rng = np.random.default_rng(6)
    lowered = 0
    for m, seed in ROWS:
        coeff, T, _ = ct.make_rows(oracle_mod, mp, 1, m, seed)
        static, _ = ct.certify(field, coeff[0], T[0], MARGIN, DEPTH, REFINE)
        for t0 in (0.0, 2.0):
            cert, info = cm.certify(field, boxes, coeff[0], T[0], t0, MARGIN, DEPTH, REFINE)
            _, d = cm.dense_lookups(field, boxes, coeff[0], T[0], t0, 20001)
            print(f"{kind} poly={poly} m={m} t0={t0}: verdict {cert[0]:+.0f} lo {cert[1]:.6g} dense {d.min():.6g} "
                  f"hi {cert[2]:.6g} static lo {static[1]:.6g} tie {info['tie']:.3g}")
            assert cert[1] <= d.min(), (m, t0, cert, d.min())
            assert cert[1] <= cert[2] and cert[1] <= static[1], (m, t0, cert, static)
            assert cert[0] != 1 or cert[1] > MARGIN
            assert cert[0] != -1 or cert[2] <= MARGIN
            assert cert[6] <= REFINE and cert[7] == np.add.reduce(T[0])
            lowered += cert[1] < static[1]
            leaves = info["leaves"]
            for j in rng.choice(len(leaves), 4, replace=False):
                s, a, w, lb, _ = leaves[j]
                assert cm.leaf_is_sound(field, boxes, lb, *info["ranges"][(s, a, w)]), (m, t0, leaves[j])
    assert lowered >= 3          # the boxes matter on these rows


# ---- (3) the tunnelling case --------------------------------------------------------------------------------------
@pytest.mark.parametrize("poly", [False, True], ids=["const_vel", "polynomial"])
def test_a_plate_that_crosses_the_curve_between_two_samples(oracle_mod, poly):
    field, mp, coeff, T, b, margin, dt, boxes, t0 = cm.tunnel_case(oracle_mod, poly)
    assert (margin, dt, t0) == (0.1, 0.3, 2.0)
    plate = cm.tunnel_case(oracle_mod, False)[7]       # (the report's twin takes a constant-velocity list)
    rep, _ = vt.report(oracle_mod, coeff[0], T[0], field.osdf, margin, plate.p0, plate.vel, plate.scale, t0=t0,
                       use_boxes=True, dt=dt)
    assert rep[0] == 4 and rep[4] == 0 and rep[6] == 0 and rep[1] > 0.6, rep       # the sampled report passes the row
    static, _ = ct.certify(field, coeff[0], T[0], margin, 2, 64)
    assert static[0] == 1 and static[1] > 2.0, static                               # so does the static certificate
    t_in, t_out, least = cm.crossing(field, boxes, coeff[0], T[0], t0, margin)
    assert 0.3 < t_in < t_out < 0.6 and least < 0.01, (t_in, t_out, least)
    step = float(np.sum(T[0])) / 20000
    cert, info = cm.certify(field, boxes, coeff[0], T[0], t0, margin, 2, 64)
    print("moving certificate", cert, "crossing", t_in, t_out, least)
    assert cert[0] == -1 and t_in - step <= cert[4] <= t_out and cert[2] <= margin, cert
    assert cert[1] <= least and info["tie"] > 1e-9


# ---- (4) mutants ----------------------------------------------------------------------------------------------------
def leaves_near(info, s, lo, hi):
    return [leaf for leaf in info["leaves"] if leaf[0] == s and leaf[1] + leaf[2] > lo and leaf[1] < hi]


def all_sound(field, boxes, info, leaves):
    return all(cm.leaf_is_sound(field, boxes, leaf[3], *info["ranges"][leaf[:3]]) for leaf in leaves)


def test_every_mutant_is_caught(oracle_mod, fields):
    field, mp, coeff, T, b, margin, dt, plate, t0 = cm.tunnel_case(oracle_mod, False)
    # swept faces at the midpoint's time only: the plate moves 3.5 cm per level-0 interval, towards some corner
    for mutant, sound in ((None, True), ("mid_faces", False)):
        _, info = cm.certify(field, plate, coeff[0], T[0], t0, margin, 0, 0, mutant)
        near = leaves_near(info, 0, 0.40, 0.50)
        assert len(near) >= 10 and all_sound(field, plate, info, near) == sound, mutant
    # the radius without Aq: a plate that turns round over the curve, at the middle of level-0 interval 32 — there its
    # velocity is zero and it still moves 400 (w / 2)^2 = 7.7 mm towards the curve, from 0.12 m beside it
    w = T[0, 0] / 64
    ts = 32.5 * w
    coef = np.zeros((1, 3, 6))
    coef[0, :, 0] = ct.position(coeff[0], 0, ts) - (0.0, 0.12, 0.0)
    coef[0, 1, :3] = (coef[0, 1, 0] + 400.0 * (t0 + ts) ** 2, -800.0 * (t0 + ts), 400.0)
    turning = cm.Boxes.polynomial(coef, plate.scale)
    for mutant, sound in ((None, True), ("no_Aq", False)):
        _, info = cm.certify(field, turning, coeff[0], T[0], t0, margin, 0, 0, mutant)
        assert all_sound(field, turning, info, leaves_near(info, 0, ts - 0.1 * w, ts + 0.1 * w)) == sound, mutant
    # boxes dropped when tau_a < 0 instead of tau_b < 0: a negative start time (the twin only: the host setter refuses
    # one) that puts box time 0 inside level-0 interval 51 of segment 0, the plate over the curve just after it
    start = -(51.3 * w)
    vel = plate.vel[0]
    early = cm.Boxes.const_vel(ct.position(coeff[0], 0, 51.6 * w) - vel * (0.3 * w), vel, plate.scale)
    for mutant, sound in ((None, True), ("tau_a", False)):
        _, info = cm.certify(field, early, coeff[0], T[0], start, margin, 0, 0, mutant)
        straddling = leaves_near(info, 0, 51.2 * w, 51.4 * w)
        assert len(straddling) == 1 and all_sound(field, early, info, straddling) == sound, mutant
    # the t_range clamp ignored: the plate stops over the curve's point of local time 0.45 s at box time t0 + 0.2 and
    # stands there; unclamped it has flown on by the time the curve arrives
    coef = np.zeros((1, 3, 6))
    coef[0, :, 0] = ct.position(coeff[0], 0, 0.45) - vel * (t0 + 0.2)
    coef[0, :, 1] = vel
    standing = cm.Boxes.polynomial(coef, plate.scale, [[0.0, t0 + 0.2]])
    _, d = cm.dense_lookups(field, standing, coeff[0], T[0], t0, 20001)
    for mutant, sound in ((None, True), ("no_clamp", False)):
        cert, _ = cm.certify(field, standing, coeff[0], T[0], t0, margin, 1, 8, mutant)
        assert (cert[1] <= d.min()) == sound, (mutant, cert, d.min())
    # V taken after the min.  The allowance kappa V covers the rounding of the forms the QUERY evaluates, whose corner
    # values lie between the lowered and the static ones: 16 eps of the largest |static corner| (the bound
    # tests/test_certify_twin.py holds the form's rounding to).  Where the boxes lower every large corner of a cell —
    # here the signed field's cells with the plate inside them — the mutant's allowance falls short of that.
    sfield, smp = fields["signed"]
    cell = np.array([11, 9, 7])
    c0 = (cell + 0.5) * sfield.res + sfield.origin
    blo, bhi = c0 + 0.3 * sfield.res, c0 + 0.6 * sfield.res
    cover = cm.Boxes.const_vel(c0[None] + 0.5 * sfield.res, np.zeros((1, 3)), np.full((1, 3), 3 * sfield.res))
    V = np.abs(sfield.corners(cell)).max()
    assert V > 0.2
    good = cm.moving_lower_bound(sfield, cover, blo, bhi, 0.0, 0.1)
    bad = cm.moving_lower_bound(sfield, cover, blo, bhi, 0.0, 0.1, "V_after")
    form = min(good, bad) + sfield.kappa * V           # the vertex minimum itself: every corner lowered to 0 or below
    assert form <= 0.0
    assert form - good >= 16 * EPS * V and form - bad < 16 * EPS * V, (form, good, bad, V)


# ---- (5) the binding against the recording stub -----------------------------------------------------------------
def moving_args(t_shape=(B, M), **kw):
    return dict(dict(coeff=t("coeff", (B, M, 18)), T=t("T", t_shape), opts=OPTS, cert=t("cert", (B, 8))), **kw)


@pytest.mark.parametrize("t_shape,stride", T_FORMS)
def test_certify_moving_device_call_record_and_stream_rule(t_shape, stride, allocations):
    for given, arrives in ((STREAM, STREAM), (types.SimpleNamespace(cuda_stream=12345), 12345)):
        ctx = make_context()
        out = certify.certify_moving_device(ctx, stream=given, **moving_args(t_shape))
        assert out.name == "cert"
        assert ctx._L.calls == [("gtop_certify_moving_device",
                                 (HANDLE, B, M, p("coeff"), p("T"), stride, OPTS, p("cert"), arrives))]
    assert allocations == []


def test_an_output_left_out_is_allocated(allocations):
    ctx = make_context()
    out = certify.certify_moving_device(ctx, stream=STREAM, **moving_args(cert=None))
    assert [(fn, shape, dtype, dev) for fn, shape, dtype, dev in allocations] == [
        ("empty", (B, 8), F64, torch.device("cuda", 0))]
    (_, received), = ctx._L.calls
    assert received[7] == p("new0") and out.name == "new0"


def test_refusals_before_any_call(allocations):
    tried = 0
    for name, value in moving_args().items():
        if not isinstance(value, FakeTensor):
            continue
        for defect, spoil in DEFECTS.items():
            ctx = make_context()
            with pytest.raises(ValueError):
                certify.certify_moving_device(ctx, stream=STREAM, **dict(moving_args(), **{name: spoil(value)}))
            assert ctx._L.calls == [], (name, defect)
            tried += 1
    assert tried == 15
    ctx = make_context()
    with pytest.raises(ValueError):
        certify.certify_moving_device(ctx, t("coeff", (B, M, 17)), t("T", (B, M)), OPTS, stream=STREAM)
    assert ctx._L.calls == []


def test_certify_moving_batch_call_record():
    ctx = make_context()
    x = np.arange(B * 18, dtype=np.float64).reshape(B, 18)
    out = certify.certify_moving_batch(ctx, x, OPTS)
    (entry, received), = ctx._L.calls
    assert entry == "gtop_certify_moving_batch" and received[:2] == (HANDLE, B) and received[3] is OPTS
    assert received[2] == (0.0, 1.0, 2.0) and out.shape == (B, 8)
