"""The time pass of csrc/gtop_time_pass.h entry by entry at rounding-error level, on EVERY row: the cost, every gT_s,
every parts column, gt0 and every gx entry of gtop_time_gradient_device, gtop_time_gradient_moving_device and
gtop_joint_gradient_device, and the start cost of the three device optimizers' first evaluation, against
tests/time_entry_ref.py — the pass in vectorised numpy with the rounding-error magnitude of every entry, held against
40-digit arithmetic by tests/test_time_entrywise_bound.py:

    |entry - reference| <= KAPPA * u64 * magnitude + allowance,        KAPPA = 2^12 (the chain count is in
                                                                       tests/test_time_entrywise_bound.py)

The 1e-5 comparisons of tests/test_gpu_time.py, test_gpu_time_moving.py and test_gpu_joint.py look at six rows of a
batch, by the row's max-norm; the other rows met only the bit-level laws.  Here the smoothness share of gT does not hide
the collision share, R_s is held by its own magnitude, and a wrong store of one gx entry is one entry out of bound.

The cases are tests/time_entry_cases.CASES (built without a GPU; the CPU test asserts that at most ALLOWANCE_CAP of a
case's (row, entry) pairs rest on an allowance, that the moving cases lower corners in later segments and that R_s is
live).  gx is also held to oracle.eval_batch_ext(mode=1)'s gradient and magnitudes — a second reference that shares no
code with the first; its gradient carries the callback's constant +1e-5 per entry (tests/test_gpu_joint.py subtracts the
same), which is taken off before the comparison.  Where the reference overflows, the kernel must.  Each failure names
the case, the entry kind, the row and entry and the largest |err| / (u * magnitude).

Largest |err| / (u * mag) against the reference on the committed seeds (MI355X, KAPPA 4096), and the rows checked:
  gT  (10 cases, 229 rows): cost 0.034, gT 0.20, parts 1.26
  MOV (6 cases and the mode off, 90 rows): cost 0.12, gT 0.13, parts 1.34, gt0 0.0051
  GX  (15 cases, 495 rows): cost 0.034, gT 0.052, parts 1.76, gx 0.82; gx against eval_batch_ext(mode=1) 1.18 (493 rows)
  the optimizers' first evaluation (72 / 70 / 75 rows): cost 0.012 (times), 0.011 (moving), 0.021 (joint)
Headroom of three orders of magnitude is the price of a bound from the arithmetic; what it resolves all the same, on
single-line mutations of gtop_time_pass.h built apart ("old": failures among the 1e-5 tests of test_gpu_time.py,
test_gpu_time_moving.py and test_gpu_joint.py; "new": among the 40 tests here):
  fr formed in float                          old 1 (moving, step 1)          new 15
  qs = w without the live mask                old 12                          new 6
  the R loop started at m - 2                 old 17                          new 6
  end_carry taken before the store            old 16                          new 14
  s4[1] off by 1e-8                           old 0                           new 15 (every GX case)
  w, the delay weight, off by 1e-8            old 0                           new 6 (every MOV case)
  R accumulated through float                 old 11                          new 6
  the 1 / 30 of cd vn / 30 in float           old 2 (collision-only cases)    new 32
  the 576 of the jerk derivative off by 1e-8  old 1 (T_out against the twin)  new 24
  the 4 of c_4' off by 1e-9                   old 3 (collision-only cases)    new 31
GX and MOV each have a mutation that passes every earlier test and fails here (s4[1], w).  The plain gT family has none
among the five tried: the collision-only cases of the 1e-5 files, where [3] cancels, and the 1e-9 comparison of T_out
with the twin already see 1e-8 .. 1e-9 on the six rows they look at; for gT these tests add the other rows and every
entry, not resolution.
GTOP_ENTRYWISE_LOG=<file> appends one JSON line per check and one per family at the end of the module."""
import json
import os

import numpy as np
import pytest

from tests import time_entry_cases as cases
from tests import time_entry_ref as ref

pytestmark = pytest.mark.gpu

U64 = ref.U64
KAPPA = 2 ** 12
ALLOWANCE_CAP = 0.05       # tests/test_gpu_entrywise.py's
FAMILY = {}                # family -> {entry kind: largest ratio of this run}, [rows checked]
NONE3 = np.zeros((0, 3))


def _log(rec):
    path = os.environ.get("GTOP_ENTRYWISE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def check(got, r, entries, what, family):
    """The bound plus the allowance on every row and entry of `entries`; overflow where the reference overflows."""
    share = ref.allowance_share(r, KAPPA, entries)
    assert share <= ALLOWANCE_CAP, (what, "share of entries resting on their allowance", share)
    for k in entries:
        v = r["val"][k] if k != "parts" else r["val"][k][..., :np.shape(got[k])[-1]]
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == v.shape, (what, k, g.shape, v.shape)
        assert not np.isfinite(g[~np.isfinite(v)]).any(), (what, k, "the reference overflows, the kernel does not")
    ratios = ref.ratios({k: got[k] for k in entries}, r)
    worst = {}
    for k, a in ratios.items():
        a = np.nan_to_num(a, nan=0.0)
        worst[k] = float(a.max()) if a.size else 0.0
    rows = int(np.shape(got["cost"])[0])
    _log(dict(what=str(what), family=family, rows=rows, share=share, **{f"ratio_{k}": v for k, v in worst.items()}))
    cur = FAMILY.setdefault(family, [{}, 0])
    cur[1] += rows
    for k, v in worst.items():
        cur[0][k] = max(cur[0].get(k, 0.0), v)
    bad = {k: v for k, v in worst.items() if not v <= KAPPA}
    if bad:
        k = max(bad, key=bad.get)
        a = np.nan_to_num(ratios[k], nan=0.0)
        at = np.unravel_index(int(np.argmax(a)), a.shape)
        raise AssertionError(f"{what}: {k} row {at[0]} entry {at[1:]}: |err| / (u * mag) = {bad[k]:.3g} (kappa {KAPPA}); "
                             f"largest per kind {worst}")
    return worst


@pytest.fixture(scope="module", autouse=True)
def _family_log():
    yield
    for family, (worst, rows) in sorted(FAMILY.items()):
        _log(dict(what=f"family {family}", rows=rows, **{f"ratio_{k}": v for k, v in worst.items()}))
        print(f"TIME ENTRYWISE family {family}: {rows} rows; largest |err| / (u * mag): "
              + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.fixture(scope="module")
def maps(oracle_mod):
    return cases.Maps(oracle_mod)


@pytest.fixture(scope="module")
def contexts(gtop, maps):
    """(the library's own field — bit-equal to the oracle builder's —, the signed field uploaded as it is)."""
    mp = maps.mp
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    assert np.array_equal(ctx.get_sdf().reshape(-1), maps.sdf.dist)
    sgn = gtop.GtopContext(device=0)
    sgn.set_sdf(maps.sdf_signed.dist, maps.sdf_signed.grid, mp.origin, mp.resolution)
    yield ctx, sgn
    ctx.close()
    sgn.close()


def _dev(*arrays):
    import torch
    return [torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0") for a in arrays]


def _np(*tensors):
    import torch
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in tensors]


def _set_boxes(ctx, case):
    bx = case["bx"]
    if bx["poly"]:
        ctx.set_moving_box_polynomials(bx["coef"], bx["scale"], bx["t_range"])
    else:
        ctx.set_moving_boxes(bx["p0"], bx["vel"], bx["scale"])
    ctx.set_moving_cost(True)
    if np.min(case["t0"]) < 0.0:      # (the host setter refuses a start before the boxes' clock; the device form takes it)
        case["t0_device"] = _dev(case["t0"])[0]
        ctx.set_start_times_device(case["t0_device"])
    else:
        ctx.set_start_times(case["t0"])


def _clear_boxes(ctx):
    ctx.set_moving_cost(False)
    ctx.set_moving_boxes(NONE3, NONE3, NONE3)
    ctx.set_start_times(None)


def _run(gtop, ctx, case, x=None, T=None):
    """The case's entry point on the device -> dict of its outputs (numpy)."""
    b = case["b"]
    xt, Dft, Tt = _dev(b.x if x is None else x, b.Df.reshape(-1, 18), case["T"] if T is None else T)
    try:
        ctx.set_params(**case["extra"])
        if case["family"] == "gT":
            c, g, p = _np(*gtop.time_gradient_device(ctx, xt, Dft, Tt, want_parts=True))
            return dict(cost=c, gT=g, parts=p)
        if case["family"] == "GX":
            c, gx, g, p = _np(*gtop.joint_gradient_device(ctx, xt, Dft, Tt, want_parts=True))
            return dict(cost=c, gx=gx, gT=g, parts=p)
        try:
            _set_boxes(ctx, case)
            c, g, g0, p = _np(*gtop.time_gradient_moving_device(ctx, xt, Dft, Tt, want_parts=True))
        finally:
            _clear_boxes(ctx)
        return dict(cost=c, gT=g, gt0=g0, parts=p)
    finally:
        ctx.set_params()


def _second_reference(oracle_mod, maps, case, got, name):
    """gx against oracle.eval_batch_ext(mode=1): the consistent gradient less the callback's +1e-5, by its own
    magnitudes and flip allowances (m <= 100: the oracle's generator is cubic in m)."""
    b = case["b"]
    sdf = maps.sdf_signed if case["signed"] else maps.sdf
    Tb = np.ascontiguousarray(np.broadcast_to(case["T"], (len(b.x), b.m)))
    c_ref, g_ref, cm, gm, _, cf, gf, _ = oracle_mod.eval_batch_ext(Tb, b.Df, b.x, sdf, oracle_mod.make_params(**case["extra"]),
                                                                   mode=1, nthreads=8)
    fin = np.isfinite(g_ref) & np.isfinite(gm)
    with np.errstate(divide="ignore", invalid="ignore"):
        rg = np.where(fin, np.maximum(np.abs(got["gx"] - (g_ref - 1e-5)) - gf, 0.0) / (U64 * gm), 0.0)
        rc = np.maximum(np.abs(got["cost"] - c_ref) - cf, 0.0) / (U64 * cm)
    worst = float(rg.max())
    _log(dict(what=f"{name} against eval_batch_ext", ratio_gx=worst, ratio_cost=float(rc.max())))
    cur = FAMILY.setdefault("GX against eval_batch_ext(mode=1)", [{}, 0])
    cur[1] += len(b.x)
    cur[0]["gx"], cur[0]["cost"] = max(cur[0].get("gx", 0.0), worst), max(cur[0].get("cost", 0.0), float(rc.max()))
    at = np.unravel_index(int(np.argmax(rg)), rg.shape)
    assert worst <= KAPPA and rc.max() <= KAPPA, (
        f"{name} against eval_batch_ext(mode=1): gx row {at[0]} entry {at[1]}: |err| / (u * mag) = {worst:.3g}, cost "
        f"{rc.max():.3g} (kappa {KAPPA})")


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_row_every_entry(gtop, oracle_mod, maps, contexts, name):
    case = cases.build(maps, name)
    ctx = contexts[1] if case["signed"] else contexts[0]
    got = _run(gtop, ctx, case)
    check(got, case["ref"], case["entries"], name, case["family"])
    if case["family"] == "GX" and case["b"].m <= 100:
        _second_reference(oracle_mod, maps, case, got, name)


def test_moving_mode_off_is_the_static_entry(gtop, maps, contexts):
    """The moving entry with the mode off: the static entry's bits (q, R and gt0 zero), held to the static reference."""
    import torch
    case = cases.build(maps, "gT-5x13-plain")
    ctx = contexts[0]
    b = case["b"]
    xt, Dft, Tt = _dev(b.x, b.Df.reshape(-1, 18), case["T"])
    c, g, p = gtop.time_gradient_device(ctx, xt, Dft, Tt, want_parts=True)
    cm, gm, g0, pm = gtop.time_gradient_moving_device(ctx, xt, Dft, Tt, want_parts=True)
    torch.cuda.synchronize()
    assert torch.equal(c, cm) and torch.equal(g, gm) and torch.equal(p, pm[:, :, :4])
    assert torch.all(pm[:, :, 4:] == 0.0) and torch.all(g0 == 0.0)
    c, g, g0, pm = _np(cm, gm, g0, pm)
    check(dict(cost=c, gT=g, gt0=g0, parts=pm), case["ref"], ("cost", "gT", "parts", "gt0"), "moving entry, mode off", "MOV")


OPT_CASES = ["gT-65x7-plain", "gT-5x13-dyn", "gT-2x227-plain", "MOV-5x13-dyn-nbox32-poly0-per_row1",
             "MOV-65x7-plain-nbox32-poly1-per_row1", "GX-65x7-plain", "GX-5x13-dyn", "GX-5x4-plain"]


@pytest.mark.parametrize("name", OPT_CASES)
def test_optimizers_first_evaluation(gtop, maps, contexts, name):
    """optimize_times_device, its moving form and optimize_joint_device with max_evals = 1 and rho = 0: info's start
    cost (F_start = cost + 0) and cost column are the pass at the clamped input, held to the cost bound there."""
    case = cases.build(maps, name, reference=False)
    ctx = contexts[1] if case["signed"] else contexts[0]
    b, fam = case["b"], case["family"]
    B, m = b.x.shape[0], b.m
    T = np.ascontiguousarray(np.broadcast_to(case["T"], (B, m)))
    t_min, t_max = (0.0301, float(np.median(T))) if m > 100 else (0.6, 1.5)
    Tc = np.clip(T, t_min, t_max)
    assert np.any(Tc != T)
    x0 = b.x
    xt, Dft, Tt = _dev(x0, b.Df.reshape(-1, 18), T)
    try:
        ctx.set_params(**case["extra"])
        if fam == "GX":
            lb, ub = gtop.GtopContext.default_bounds(b.waypoints, bos=0.5, vos=1.0, aos=2.0)      # (tight: x0 leaves them)
            x0 = b.x + np.random.default_rng(m + B).normal(0.0, 0.5, size=b.x.shape)
            xc = np.clip(x0, lb, ub)
            assert np.any(xc != x0)
            xt, lbt, ubt = _dev(x0, lb, ub)
            _, T_out, info = gtop.optimize_joint_device(ctx, gtop.GtopJointOpt(rho=0.0, t_min=t_min, t_max=t_max, max_evals=1),
                                                        xt, Dft, Tt, lbt, ubt)
            T_out, info = _np(T_out, info)
            start, cost, evals = info[:, 2], info[:, 4], info[:, 1]
        else:
            xc = x0
            opts = gtop.GtopTimeOpt(rho=0.0, t_min=t_min, t_max=t_max, max_evals=1)
            if fam == "MOV":
                try:
                    _set_boxes(ctx, case)
                    T_out, info = _np(*gtop.optimize_times_moving_device(ctx, opts, xt, Dft, Tt))
                finally:
                    _clear_boxes(ctx)
            else:
                T_out, info = _np(*gtop.optimize_times_device(ctx, opts, xt, Dft, Tt))
            start, cost, evals = info[:, 3], info[:, 5], info[:, 2]
    finally:
        ctx.set_params()
    assert np.all(evals == 1) and (fam == "GX" or np.array_equal(T_out, Tc))
    r = ref.reference(Tc, b.Df, xc, maps.field_signed if case["signed"] else maps.field, case["params"], t0=case["t0"],
                      boxes=case["boxes"])
    check(dict(cost=start), r, ("cost",), (name, "optimizer, first evaluation, F_start"), fam + " optimizer")
    check(dict(cost=cost), r, ("cost",), (name, "optimizer, first evaluation, cost"), fam + " optimizer")
