"""The cost/gradient kernels entry by entry at rounding-error level: every row's cost and every gradient entry against
the oracle, within a multiple of the unit roundoff times the oracle's own rounding-error MAGNITUDES
(oracle.eval_batch_mag, oracle_cost_grad_mag in oracle/gtop_oracle.h) — the callback re-evaluated with absolute values
of its inputs, additions for subtractions and sums of products of magnitudes.  Two implementations that take the same
discrete decisions differ by at most a few rounding errors per operation along the longest chain, each of size
u * magnitude; the 1e-5 normwise contract (BASELINE.json, the rest of the suite) leaves seven orders of magnitude
below it in which one kernel body could be wrong without a failure.

    |c - c_ref| <= KAPPA * u * Cmag,    |g_k - g_ref_k| <= KAPPA * u * Gmag_k     (u = 2^-53 fp64, 2^-24 fp32)

KAPPA, from the arithmetic (not from a run):
  * fp64, KAPPA64 = 2^12 (tau64 = 4.5e-13 of the magnitude).  Per sample term the longest chain is about 60 roundings:
    the closed-form coefficients (fast_rcp's two Newton steps, 1/T^3..1/T^5 as products, P / V / A with their
    cancellation, which the magnitude carries as |L||d|), the sample polynomial, the lookup (its weights' error,
    (|pos| + |idx_pos|) / res, is in the magnitude), penalty_exp (2.7e-14 = 240 u relative: the largest single
    term; its argument's error is the magnitude's factor 1 + (dist + |d0|) / r), speed_sqrt (2 u), quick_rcp
    (1 u), A_s^-T (its cancellation is |L|^T in the magnitude).  The sample times differ by up to 30 u relative
    (t_i = 1e-3 + i dt against the reference's t += dt): 5 * 30 u on t^5.  The sums: up to 30 * 227 terms per entry
    (LONG, m = 227) — the oracle adds them in sequence, the kernels per lane and then across lanes; rounding errors
    of a long sum of same-signed terms are uncorrelated in practice and grow like sqrt(N) u (83 u at 6 810 terms), the
    deterministic worst case N u only for adversarial data.  240 + 150 + 60 + 2 * 83 ~ 620 u for the two
    implementations together: 2^12 leaves a factor of six.
  * fp32, KAPPA32 = 2^10 (tau32 = 6.1e-5): sample positions, velocities and coefficients are formed in double there as
    in the oracle (the same floats); the lookup (fp32 corner records: their rounding is the (|v1| + |v0|) of the
    magnitude), expf (2 ulp, argument error in the magnitude), the products and the per-lane and cross-lane sums are
    fp32: ~40 roundings per term plus sqrt(N) for sums of up to 30 * 64 terms (44) — under 2^7; 2^10 covers the
    chunked body's longer sums and the fp32 form of A_s^-T.

Decisions within rounding of their threshold.  The float rounding of a sample's position / velocity / acceleration
(the reference's float locals, grad_traj_optimizer.cpp:457-465, :477-485) is computed in double from differently-rounded
coefficients, so a pre-rounding double within 2^9 u64 of its magnitude from a rounding boundary (~25 u of the
coefficients and the polynomial plus the 150 u of the sample times) may round either way in a correct kernel.  That is
common — a velocity that cancels to 1e-5 of its magnitude has float steps finer than its own rounding error — so the
oracle does not excuse such rows: it returns an absolute allowance, Cflip / Gflip, twice the first-order effect of one
float step of each such coordinate, and the bound is KAPPA * u * mag + flip.  The cell choice and the sample count are
formed from the same floats / replayed with the same additions in every body, so they never differ.  What remains a
TIE ROW is an fp32 row whose in-map margin is below TIE_MAP32 * u32 (the fp32 bodies compare with the float-rounded map
box): counted, required to be rare (TIE_RATE), and held to the contract's normwise bound instead.

Largest |err| / (u * mag) seen (committed seeds, MI355X): fp64 — every body's cost <= 0.08 and gradient <= 1.5,
the fuzz draws 22 (cost) / 1.5, and 56 / 1.6 with GTOP_FUZZ_EXTRA=30; fp32 — <= 0.8 / 0.43.  No tie rows in 38 677.
Headroom of ~70x (fp64) is the price of a bound from the arithmetic.  What it does and does not catch, measured on
single-line kernel mutations: dropping round_through_float, the "+1e-5" of vn, penalty_exp's r^9 coefficient (2e-10 relative: the exp sweep and the fuzz draws)
and a 1e-7 change of the LONG body's cost constant (the exp sweep and the fuzz draws; the smoothness-dominated rows of
test_every_body carry the oracle's product-of-magnitudes bound for d'Rd, Cmag ~ 1e4 cost, and do not see it) all fail
here; a 3e-4 relative change of the fp32 speed_sqrt does not (6.1e-5 * Cmag, with Cmag >= 5 cost, is above it: the fp32
bodies stay guarded by the 2e-4 checks of test_gpu_wave.py / test_gpu_fuzz.py, which catch it).

Where the oracle's value overflows, the kernel's must too.  Each failure names the body and the largest ratio
|err| / (u * magnitude).  The fused optimizer bodies (MM = GtopMmaState) are held to Cmag on their first evaluation's
cost (optimize_batch_ex with max_evals = 1, at clip(x0, lb, ub)); their gradients are covered only through the
optimizer roads (test_optimizer.py / test_gpu_fuzz.py), not entrywise here.

The later bodies (second half of the file) against oracle.eval_batch_ext — the oracle with a gradient mode and a
time-aware lookup, its magnitudes held against 40-digit arithmetic by tests/test_entrywise_bound.py: the consistent
gradient in every geometry (ordinary, DYN, DYN with steep scale lengths; both precisions; the cost bit-equal to mode
0's), the moving-obstacle bodies in each of their geometries (ten lanes, five lanes with one or two trajectories per
wavefront, chunked; with and without DYN; gradient modes 0 and 1; constant-velocity lists of 1 and 32 boxes, polynomial
lists of 8 — degree five, two validity intervals ending inside the trajectories — and 32; per-row and shared start
times), the optimizer loop's moving bodies on their first evaluation, the edge batch and the signed field in the new
modes, and the 64-bit-index forms (DYN, five lanes with one trajectory per wavefront, two wavefronts per trajectory,
chunked, consistent at both pins, moving, optimizer loop).  The parametrisation ids name the body.  Every check first
asserts, from the oracle alone, that at most ALLOWANCE_CAP of its (row, entry) pairs rest on a flip or sign allowance
larger than KAPPA * u * magnitude (largest share on the committed seeds: 2.7 %, the 8-row wide moving case; 2.0 %
otherwise), and every moving case that at least half of its rows (an eighth with a single box) have a box-lowered
corner and a cost more than 1e-6 relative off the static one.  In fp32 the steep DYN block overflows past fp32's range
on most rows of the long-13 / long-40 / long-227 / spl30 batches (36, 5, 1 and 66 rows): those rows are held to
"overflows where the oracle does", as check() holds every such row.
Largest |err| / (u * mag), cost / gradient (committed seeds, MI355X; KAPPA 4096 fp64, 1024 fp32): consistent fp64
0.35 / 1.4, consistent fp32 0.67 / 0.043, moving constant-velocity 0.039 / 0.89, moving polynomial 0.037 / 0.89, moving
plus consistent 0.039 / 0.89, wide 0.0024 / 0.11.  No tie rows in 26 267.
Single-line kernel mutations, built apart and run against these tests (long-227 left out): mode 1's weight wds[] taken
from aw[] fails 57 of the 94 tests — 24 of the 27 fp64 and 4 fp32 checks of test_consistent_every_body (the packed fp32
bodies do not read it), all 24 of test_moving_every_body, both wide mode-1 cases, the edge batch and the signed field;
csum_dyn without one axis's ca fails 45 — 21 DYN checks of test_consistent_every_body (3 of them fp32) and all 24 of
test_moving_every_body (tests/test_gpu_consistent_gradient.py's four steep cases see it too); a box half extent off by
2^-36 fails NONE of the 94 — the 1e-12 normwise check of
tests/test_gpu_moving_cost.py sees it on one of three cases tried (m = 2, one box: 1.4e-12 / 1.5e-11; not m = 6 or 13
with 8 boxes).  tests/test_entrywise_bound.py says why: with Cmag >= 2.6 cost and Gmag_k some 1e4 |g_k| the bound
resolves about 1e-8 of an entry, far finer than the 1e-5 the mode-1 bodies were held to, coarser than the 1e-12 the
moving bodies already are; for those it adds the bodies no 1e-12 test launches, not resolution.

GTOP_ENTRYWISE_LOG=<file> appends one JSON line per check (body, precision, rows, ties, largest ratios), and one per
family of the later bodies at the end of the module."""
import json
import math
import os
import types

import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import test_gpu_fuzz

pytestmark = pytest.mark.gpu

U64, U32 = 2.0 ** -53, 2.0 ** -24
KAPPA64, KAPPA32 = 2 ** 12, 2 ** 10
TIE_MAP32 = 4              # x u32 of the map box (fp32 bodies)
TIE_RATE = 0.02            # at most this share of a check's rows may be ties
TOL64, TOL32 = 1e-5, 2e-4  # what tie rows are held to (the contract; test_gpu_wave.py's fp32 bound)

DYN = dict(enable_dyn=1, alpha_v=1.0, r_v=4.0, v0=2.5, alpha_a=1.0, r_a=15.0, a0=3.5)
VARIANTS = {"colli-free": dict(wc=0.0), "ordinary": dict(), "dyn": DYN}

# (name, waves, samples per lane, m, B): every geometry pick_geometry returns
GEOMETRIES = [
    ("long-13", 0, 0, 13, 40), ("long-40", 0, 0, 40, 5), ("long-227", 0, 0, 227, 1),
    ("spl30", 0, 30, 17, 70), ("spl10", 0, 10, 8, 50), ("nw2", 1, 0, 10, 40),
    ("spl3-2w", 0, 3, 5, 200), ("spl3-3w", 0, 3, 5, 3100),
    ("spl6-nt1", 0, 6, 9, 60), ("spl6-nt2", 0, 6, 5, 61),
]


def _log(rec):
    path = os.environ.get("GTOP_ENTRYWISE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def check(c, g, ref, dtype, what):
    """Entrywise bound on the non-tie rows, the contract on the tie rows, overflow where the oracle overflows."""
    c_ref, g_ref, cm, gm, mg, cf, gf = ref
    c, g = np.asarray(c, dtype=np.float64), np.asarray(g, dtype=np.float64)
    f32 = dtype == "f32"
    kappa, u = (KAPPA32, U32) if f32 else (KAPPA64, U64)
    over = ~np.isfinite(c_ref) | ~np.isfinite(g_ref).all(axis=1) | ~np.isfinite(cm) | ~np.isfinite(gm).all(axis=1)
    if f32:   # past fp32's range (3.4e38) a row may come back inf
        over |= (cm > 1e36) | (gm.max(axis=1) > 1e36)
    assert not np.isfinite(c[~np.isfinite(c_ref)]).any(), (what, "the oracle's cost overflows, the kernel's does not")
    tie = np.zeros(len(c), dtype=bool)
    if f32:
        tie |= mg[:, 2] < TIE_MAP32 * U32
    ok = ~over & ~tie
    assert np.isfinite(c[ok]).all() and np.isfinite(g[ok]).all(), (what, "non-finite result where the oracle's is finite")
    with np.errstate(divide="ignore", invalid="ignore"):
        rc = np.maximum(np.abs(c[ok] - c_ref[ok]) - cf[ok], 0) / (u * cm[ok])
        rg = np.maximum(np.abs(g[ok] - g_ref[ok]) - gf[ok], 0) / (u * gm[ok])
    worst_c = float(rc.max()) if rc.size else 0.0
    worst_g = float(rg.max()) if rg.size else 0.0
    ntie = int((tie & ~over).sum())
    _log(dict(what=str(what), dtype=dtype, rows=int(len(c)), checked=int(ok.sum()), ties=ntie,
              overflow=int(over.sum()), ratio_cost=worst_c, ratio_grad=worst_g))
    assert worst_c <= kappa and worst_g <= kappa, (
        f"{what} {dtype}: largest |err| / (u * mag): cost {worst_c:.3g}, gradient {worst_g:.3g} "
        f"(kappa {kappa}); worst row {int(np.argmax(rc)) if rc.size else -1} / entry "
        f"{np.unravel_index(int(np.argmax(rg)), rg.shape) if rg.size else -1}")
    assert ntie <= max(1, TIE_RATE * len(c)), (what, dtype, "too many tie rows", ntie, len(c))
    t = tie & ~over
    if t.any():
        tol = TOL32 if f32 else TOL64
        rel_c = np.abs(c[t] - c_ref[t]) / np.abs(c_ref[t])
        rel_g = np.max(np.abs(g[t] - g_ref[t]), axis=1) / np.max(np.abs(g_ref[t]), axis=1)
        assert rel_c.max() <= tol and rel_g.max() <= tol, (what, dtype, "tie rows", rel_c.max(), rel_g.max())
    return worst_c, worst_g, ntie


@pytest.fixture(scope="module")
def scene(gtop, oracle_mod):
    mp = problem.make_map((60, 50, 30), density=0.03, seed=11)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    assert np.array_equal(ctx.get_sdf().reshape(-1), sdf.dist)
    yield mp, ctx, sdf
    ctx.close()


def _f32_batch(b):
    """fp32 interfaces take fp32 inputs: the reference is the oracle on those same (representable) values."""
    x, Df, T = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (b.x, b.Df, b.T))
    return problem.Batch(b.waypoints, T, Df, x, b.m)


def _device(ctx, b, dtype, waves, spl, kw):
    import torch
    td = torch.float64 if dtype == "f64" else torch.float32
    dev = torch.device("cuda:0")
    x, Df, T = (torch.tensor(a, dtype=td, device=dev) for a in (b.x, b.Df.reshape(-1, 18), b.T))
    try:
        ctx.set_params(**kw)
        ctx.set_launch_geometry(waves, spl)
        c, g = ctx.eval_device(x, Df, T)
        torch.cuda.synchronize()
    finally:
        ctx.set_launch_geometry(0, 0)
        ctx.set_params()
    return c.double().cpu().numpy(), g.double().cpu().numpy()


def _ref(oracle_mod, b, sdf, kw):
    return oracle_mod.eval_batch_mag(b.T, b.Df, b.x, sdf, oracle_mod.make_params(**kw), nthreads=8)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_every_body(scene, oracle_mod, geo, variant, dtype):
    mp, ctx, sdf = scene
    name, waves, spl, m, B = geo
    b = problem.make_trajectories(B, m, mp, seed=7000 + m + B,
                                  step_len=(0.2, 0.5) if m > 12 else (0.5, 1.2) if m > 6 else (1.0, 2.0),
                                  boundary="random")
    if dtype == "f32":
        b = _f32_batch(b)
    kw = VARIANTS[variant]
    c, g = _device(ctx, b, dtype, waves, spl, kw)
    check(c, g, _ref(oracle_mod, b, sdf, kw), dtype, (name, variant, "eval_device"))


@pytest.mark.parametrize("geo", [g for g in GEOMETRIES if g[4] <= 200], ids=[g[0] for g in GEOMETRIES if g[4] <= 200])
def test_host_entry_points(scene, oracle_mod, geo):
    """eval_batch (host arrays) on the same bodies, and cost_nlopt at B = 1."""
    mp, ctx, sdf = scene
    name, waves, spl, m, B = geo
    b = problem.make_trajectories(B, m, mp, seed=7100 + m, step_len=(0.2, 0.5) if m > 12 else (0.5, 1.2))
    ctx.set_params()
    ctx.set_launch_geometry(waves, spl)
    try:
        ctx.set_problem(b.T, b.Df)
        c, g = ctx.eval_batch(b.x)
        ref = _ref(oracle_mod, b, sdf, {})
        check(c, g, ref, "f64", (name, "ordinary", "eval_batch"))
        ctx.set_problem(b.T[:1], b.Df[:1])
        c1, g1 = ctx.cost_nlopt(b.x[0])
        check(np.array([c1]), g1[None, :], tuple(a[:1] for a in ref), "f64", (name, "ordinary", "cost_nlopt"))
    finally:
        ctx.set_launch_geometry(0, 0)


@pytest.fixture(scope="module")
def wide(gtop, oracle_mod):
    """The 4097 x 4097 x 6 field of test_gpu_parity.test_parity_wide_index_field (past 2^31 bytes: every body on it is
    a 64-bit-index one), generated and uploaded once: (map extents, context, oracle Sdf)."""
    grid, res = (4097, 4097, 6), 0.2
    origin = np.array([-grid[0] * res / 2, -grid[1] * res / 2, 0.0])
    dist = np.random.default_rng(5).uniform(0.0, 2.0, size=grid[0] * grid[1] * grid[2])
    ms = types.SimpleNamespace(origin=origin, map_size=np.array(grid) * res)
    ctx = gtop.GtopContext(device=0)
    ctx.set_sdf(dist, grid, origin, res)
    sdf = oracle_mod.Sdf(origin, res, grid, dist)
    yield ms, ctx, sdf
    ctx.close()


def test_wide_index_bodies(wide, oracle_mod):
    """The 64-bit-index bodies at six segments, every samples-per-lane pin, both precisions."""
    ms, ctx, sdf = wide
    b = problem.make_trajectories(96, 6, ms, seed=77, margin=0.15, step_len=(0.5, 1.5))
    ref = _ref(oracle_mod, b, sdf, {})
    for spl in (3, 6, 10, 30):
        c, g = _device(ctx, b, "f64", 0, spl, {})
        check(c, g, ref, "f64", ("wide", spl))
    b32 = _f32_batch(b)
    ref32 = _ref(oracle_mod, b32, sdf, {})
    for spl in (3, 6):
        c, g = _device(ctx, b32, "f32", 0, spl, {})
        check(c, g, ref32, "f32", ("wide", spl))


@pytest.mark.parametrize("seed", test_gpu_fuzz.seeds(0, 40))
def test_fuzz_draws(gtop, oracle_mod, seed):
    """The draws of test_gpu_fuzz._draw (GTOP_FUZZ_EXTRA adds seeds), fp64 through eval_device at the launch rule."""
    mp, b, kw, _ = test_gpu_fuzz._draw(seed)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        ctx.update_sdf_map(mp.obstacle_points())
        c, g = _device(ctx, b, "f64", 0, 0, kw)
        ref = _ref(oracle_mod, b, sdf, kw)
        if (~np.isfinite(ref[0])).mean() >= 0.1 and seed >= test_gpu_fuzz.BASE:
            pytest.skip("an extra draw that is degenerate (most rows overflow in the reference itself)")
        check(c, g, ref, "f64", ("fuzz", seed, b.m, len(b.x)))
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", test_gpu_fuzz.seeds(1000, 20))
def test_fuzz_draws_fp32(gtop, oracle_mod, seed):
    """The fp32 bodies on the draws of test_random_draw_fp32 (fp32-representable inputs, ordinary rows)."""
    mp, b, kw, shared_T = test_gpu_fuzz._draw(seed)
    bb = problem.make_trajectories(len(b.x), b.m, mp, seed=seed,
                                   step_len=(0.15 * min(mp.map_size) / 2, 0.4 * min(mp.map_size) / 2),
                                   margin=min(1.0, float(min(mp.map_size)) / 4), boundary="random" if seed % 2 else None)
    T = bb.T[0].copy() if shared_T else bb.T
    kw = {k: v for k, v in kw.items() if k not in ("alpha", "r", "d0")}
    bb = _f32_batch(problem.Batch(bb.waypoints, T, bb.Df, bb.x, b.m))
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        ctx.update_sdf_map(mp.obstacle_points())
        c, g = _device(ctx, bb, "f32", 0, 0, kw)
        check(c, g, _ref(oracle_mod, bb, sdf, kw), "f32", ("fuzz32", seed, b.m, len(bb.x)))
    finally:
        ctx.close()


def _edge_batches(mp, sdf_box):
    m = 6
    b = problem.make_trajectories(64, m, mp, seed=91, step_len=(0.5, 1.2), boundary="random")
    x, T = b.x.copy(), b.T.copy()
    T[1:8, 2] = 0.0009
    T[8:16, 3] = 0.0299
    T[16:24, 1] = 0.0301
    T[24:28, 0] = 0.03
    x[28:32, 0] += 40.0                       # rows that leave the map
    x[32:34, 3 * m - 3 + 1] -= 40.0
    return problem.Batch(b.waypoints, T, b.Df, x, m)


@pytest.mark.parametrize("kw", [dict(), dict(step=1), dict(ws=0.0), dict(wc=5e-5), DYN],
                         ids=["default", "step1", "ws0", "wc5e-5", "dyn"])
@pytest.mark.parametrize("spl", [0, 3, 6, 10, 30])
def test_edges(gtop, oracle_mod, kw, spl):
    """A far-off map origin (-500, 300, 0); segments of 0.0009 / 0.0299 / 0.03 / 0.0301 s; rows leaving the map."""
    mp = problem.make_map((50, 40, 24), density=0.03, seed=12)
    mp = problem.MapSpec(mp.grid, mp.resolution, np.array([-500.0, 300.0, 0.0]), mp.occupancy)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    b = _edge_batches(mp, sdf)
    if kw.get("enable_dyn"):
        b = problem.Batch(b.waypoints, np.maximum(b.T, 0.3), b.Df, b.x, b.m)   # (exp(v / r_v) of a 1 ms segment overflows)
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        ctx.update_sdf_map(mp.obstacle_points())
        assert np.array_equal(ctx.get_sdf().reshape(-1), sdf.dist)
        c, g = _device(ctx, b, "f64", 0, spl, kw)
        check(c, g, _ref(oracle_mod, b, sdf, kw), "f64", ("far origin / short segments", spl, kw))
    finally:
        ctx.close()


@pytest.mark.parametrize("spl", [0, 3, 6, 10, 30])
def test_signed_field(gtop, oracle_mod, spl):
    """A signed field (negative inside obstacles): the exp's argument grows past d0 / r from the other side."""
    mp = problem.make_map((48, 40, 24), density=0.05, seed=13)
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.set_field_sign(True, 1.0)
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        ctx.update_sdf_map(mp.obstacle_points())
        dist = ctx.get_sdf().reshape(-1).astype(np.float64)
        assert (dist < 0).any()
        sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
        sdf.dist[:] = dist
        b = problem.make_trajectories(64, 6, mp, seed=14, step_len=(0.5, 1.2))
        for dtype in ("f64", "f32"):
            bb = b if dtype == "f64" else _f32_batch(b)
            c, g = _device(ctx, bb, dtype, 0, spl, {})
            check(c, g, _ref(oracle_mod, bb, sdf, {}), dtype, ("signed field", spl))
    finally:
        ctx.close()


def _exp_points():
    grid = list(np.linspace(-700.0, 709.5, 113))
    ln2 = math.log(2.0)
    halves = [(k + 0.5) * ln2 + e for k in (-1009, -300, -40, -2, -1, 0, 1, 2, 40, 300, 1022)
              for e in (-1e-12, 1e-12)]
    edge = [709.78, 709.782, 709.7827, 709.79, 710.0, -708.4, -745.0]
    return sorted(set(float(v) for v in grid + halves + edge + [0.0, 0.17, -0.34, 0.3466]))


# (the sweep leaves out the two bodies whose oracle side is slow per launch: LONG at 227 segments — long-13 / long-40
# are the same body — and spl 3 on the three-wavefront budget, the same penalty_exp as on the two-wavefront one)
SWEEP = [g for g in GEOMETRIES if g[0] not in ("long-227", "spl3-3w")]


@pytest.mark.parametrize("geo", SWEEP, ids=[g[0] for g in SWEEP])
def test_exp_sweep(gtop, oracle_mod, geo):
    """penalty_exp in every fp64 body: a zero field (dist = 0 exactly), r = 1, so the exp's argument is d0 itself, over
    a dense grid of [-700, 709.8], at (k + 1/2) ln 2 +- 1e-12 and past the overflow edge; alpha = exp(-d0) (within
    [e^-690, e^690]) makes the collision term dominate the +1e-3 wherever it can.  Cost only, against libm's exp."""
    name, waves, spl, m, B = geo
    grid, res = (24, 24, 12), 0.25
    origin = np.array([-3.0, -3.0, 0.0])
    ms = types.SimpleNamespace(origin=origin, map_size=np.array(grid) * res)
    dist = np.zeros(grid[0] * grid[1] * grid[2])
    b = problem.make_trajectories(min(B, 8), m, ms, seed=15, margin=0.5, step_len=(0.1, 0.2))
    sdf = oracle_mod.Sdf(origin, res, grid, dist)
    ctx = gtop.GtopContext(device=0)
    worst = 0.0
    try:
        ctx.set_sdf(dist, grid, origin, res)
        for x in _exp_points():
            kw = dict(ws=0.0, wc=1.0, r=1.0, d0=x, alpha=math.exp(min(690.0, max(-690.0, -x))))
            c, _ = _device(ctx, b, "f64", waves, spl, kw)
            c_ref, _, cm, _, _, cf, _ = _ref(oracle_mod, b, sdf, kw)
            inf = ~np.isfinite(c_ref)
            assert not np.isfinite(c[inf]).any(), (name, x, "the oracle overflows, the kernel does not")
            assert np.isfinite(c[~inf]).all(), (name, x, "the kernel overflows, the oracle does not")
            if (~inf).any():
                r = float(np.max(np.maximum(np.abs(c[~inf] - c_ref[~inf]) - cf[~inf], 0) / (U64 * cm[~inf])))
                worst = max(worst, r)
                assert r <= KAPPA64, f"{name}: exp argument {x!r}: |err| / (u * Cmag) = {r:.3g} (kappa {KAPPA64})"
    finally:
        ctx.close()
    _log(dict(what=f"exp sweep {name}", dtype="f64", ratio_cost=worst))


@pytest.mark.parametrize("m,B", [(5, 1), (5, 64), (9, 1), (9, 64), (13, 3), (5, 3100)])
def test_fused_optimizer_first_evaluation(scene, oracle_mod, m, B):
    """The optimizer-loop bodies (MM = GtopMmaState): their first evaluation's cost, at clip(x0, lb, ub), to Cmag."""
    mp, ctx, sdf = scene
    b = problem.make_trajectories(B, m, mp, seed=7200 + m + B, step_len=(0.5, 1.2))
    lb, ub = ctx.default_bounds(b.waypoints)
    x0 = b.x + np.random.default_rng(m + B).normal(0.0, 0.5, size=b.x.shape)
    ctx.set_params()
    ctx.set_problem(b.T, b.Df)
    _, cost, nev, _ = ctx.optimize_batch_ex(x0, lb, ub, 1)
    assert (nev == 1).all()
    xc = np.clip(x0, lb, ub)
    ref = oracle_mod.eval_batch_mag(b.T, b.Df, xc, sdf, oracle_mod.make_params(), nthreads=8)
    # (the gradient is not returned: the check is on the cost; the gradient columns are the oracle's own)
    check(cost, ref[1], ref, "f64", ("optimizer loop, first evaluation", m, B))


# ---------------------------------------------------------------------------------------------------------------------
# The bodies added since: the consistent gradient (GtopConsistent<MM>, gtop_set_gradient_mode), the moving-obstacle
# lookup (GtopMoving<MM> / GtopMovingPoly<MM>, gtop_set_moving_cost) and the 64-bit-index forms of each — against
# oracle.eval_batch_ext, whose magnitudes tests/test_entrywise_bound.py holds against 40-digit arithmetic.
# ---------------------------------------------------------------------------------------------------------------------
ALLOWANCE_CAP = 0.05       # at most this share of a check's (row, entry) pairs may rest on their flip / sign allowance
STEEP = dict(enable_dyn=1, alpha_v=2.0, r_v=0.5, v0=2.5, alpha_a=1.5, r_a=1.0, a0=3.5)   # test_gpu_consistent_gradient.py's
FAMILY = {}                # family -> [largest cost ratio, largest gradient ratio] of this run (logged at module teardown)


def ref_ext(oracle_mod, b, sdf, kw, mode=0, boxes=None, t0=None):
    """oracle.eval_batch_ext's seven arrays (what check() takes) and the rows' lowered-sample counts."""
    *ref, lowered = oracle_mod.eval_batch_ext(b.T, b.Df, b.x, sdf, oracle_mod.make_params(**kw), mode=mode, boxes=boxes,
                                              t0=t0, nthreads=8)
    return tuple(ref), lowered


def allowance_share(ref, dtype):
    """Share of the (row, entry) pairs of a reference, cost included, whose flip-plus-sign allowance is larger than
    KAPPA * u * magnitude: there the check says little.  From the oracle alone."""
    _, _, cm, gm, _, cf, gf = ref
    kappa, u = (KAPPA32, U32) if dtype == "f32" else (KAPPA64, U64)
    fin = np.isfinite(cm) & np.isfinite(gm).all(axis=1)
    if not fin.any():
        return 0.0
    big = np.concatenate([(cf[fin] > kappa * u * cm[fin])[:, None], gf[fin] > kappa * u * gm[fin]], axis=1)
    return float(big.mean())


def check_family(family, c, g, ref, dtype, what):
    """check() behind the condition that keeps it from passing on allowances; the family's largest ratios kept."""
    share = allowance_share(ref, dtype)
    assert share <= ALLOWANCE_CAP, (what, dtype, "share of entries resting on their allowance", share)
    wc_, wg_, _ = check(c, g, ref, dtype, what)
    cur = FAMILY.setdefault(family, [0.0, 0.0])
    cur[0], cur[1] = max(cur[0], wc_), max(cur[1], wg_)
    return wc_, wg_


@pytest.fixture(scope="module", autouse=True)
def _family_log():
    yield
    for family, (rc, rg) in sorted(FAMILY.items()):
        _log(dict(what=f"family {family}", ratio_cost=rc, ratio_grad=rg))
        print(f"ENTRYWISE family {family}: largest |err| / (u * mag): cost {rc:.3g}, gradient {rg:.3g}")


def _device_mode(ctx, b, dtype, waves, spl, kw, mode):
    try:
        ctx.set_gradient_mode(bool(mode))
        return _device(ctx, b, dtype, waves, spl, kw)
    finally:
        ctx.set_gradient_mode(False)


def every_body_batch(mp, geo, dtype):
    """test_every_body's batch of a geometry."""
    name, waves, spl, m, B = geo
    b = problem.make_trajectories(B, m, mp, seed=7000 + m + B,
                                  step_len=(0.2, 0.5) if m > 12 else (0.5, 1.2) if m > 6 else (1.0, 2.0),
                                  boundary="random")
    return _f32_batch(b) if dtype == "f32" else b


CONS_VARIANTS = {"ordinary": dict(), "dyn": DYN, "dyn-steep": STEEP}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("variant", list(CONS_VARIANTS))
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[f"GtopConsistent-{g[0]}" for g in GEOMETRIES])
def test_consistent_every_body(scene, oracle_mod, geo, variant, dtype):
    """Mode 1 in every geometry of GEOMETRIES (the bodies of gtop_kernels_consistent.o), with and without the DYN block
    and with its steep scale lengths; the cost bit-equal to mode 0's."""
    mp, ctx, sdf = scene
    name, waves, spl, m, B = geo
    b = every_body_batch(mp, geo, dtype)
    kw = CONS_VARIANTS[variant]
    c0, g0 = _device_mode(ctx, b, dtype, waves, spl, kw, 0)
    c, g = _device_mode(ctx, b, dtype, waves, spl, kw, 1)
    assert np.array_equal(c0, c, equal_nan=True), "the cost differs between the gradient modes"
    assert not np.array_equal(g0, g, equal_nan=True)
    ref, _ = ref_ext(oracle_mod, b, sdf, kw, mode=1)
    check_family(f"consistent {dtype}", c, g, ref, dtype, (name, variant, "mode 1"))


# ---- moving bodies: the `world` of tests/test_gpu_moving_cost.py ----
MOVING_PARAMS = dict(ws=1.0, wc=5.0, alpha=10.0, r=0.5, d0=0.8)        # tests/test_moving_cost.py's PARAMS (set fields)
# (body, samples-per-lane pin, m, B)
MOVING_GEOMETRIES = [
    ("ten-lanes-m2", 3, 2, 40), ("ten-lanes-m5", 3, 5, 40), ("five-lanes-two-per-wave-m5", 6, 5, 41),
    ("five-lanes-one-per-wave-m9", 6, 9, 40), ("chunked-m13", 0, 13, 24), ("chunked-m40", 0, 40, 4),
]
BOX_LISTS = ["cv1", "cv32", "poly8-clamped", "poly32"]


@pytest.fixture(scope="module")
def world(gtop, oracle_mod):
    mp = problem.make_map((64, 56, 40), density=0.05, seed=5)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    yield mp, sdf, ctx
    ctx.close()


def aimed_boxes(b, t0, rng, kind, rows=None):
    """tests/test_gpu_moving_cost.py::_aimed_boxes — box k is at a random waypoint of a random trajectory when that
    trajectory is — as the dict oracle.eval_batch_ext takes.  The polynomial lists (tests/box_poly_twin.coefficients,
    then cubic .. quintic terms that leave the rendezvous where it is): `poly8-clamped` is of degree five, and its
    first two boxes carry a validity interval that ends 0.05 s after their rendezvous, inside the trajectory's span.
    rows: the trajectory each box is aimed at (default: random ones)."""
    from tests import box_poly_twin
    nbox = int("".join(ch for ch in kind.split("-")[0] if ch.isdigit()))
    t0 = np.broadcast_to(np.asarray(t0, dtype=np.float64), (len(b.x),))
    j = rng.integers(0, len(b.x), nbox) if rows is None else np.asarray(rows)
    w = rng.integers(0, b.m + 1, nbox)
    vel = rng.uniform(-2.0, 2.0, (nbox, 3)) * np.array([1.0, 1.0, 0.2])
    when = np.array([t0[jj] + b.T[jj][:ww].sum() for jj, ww in zip(j, w)])
    scale = rng.uniform(1.0, 2.0, (nbox, 3))
    if kind.startswith("cv"):
        return dict(p0=b.waypoints[j, w] - vel * when[:, None], vel=vel, scale=scale)
    coef = box_poly_twin.coefficients(b.waypoints[j, w], vel, rng.uniform(-1.0, 1.0, (nbox, 3)), when)
    coef[:, :, 3:] = rng.normal(0.0, 1.0, (nbox, 3, 3)) * np.array([2e-2, 3e-3, 4e-4])
    coef[:, :, 0] -= sum(coef[:, :, i] * when[:, None] ** i for i in (3, 4, 5))
    t_range = None
    if kind.endswith("clamped"):
        t_range = np.tile([-np.inf, np.inf], (nbox, 1))
        t_range[:2] = np.stack([when[:2] - 0.3, when[:2] + 0.05], axis=1)
    return dict(coef=coef, scale=scale, t_range=t_range)


def set_boxes(ctx, boxes, t0):
    if "coef" in boxes:
        ctx.set_moving_box_polynomials(boxes["coef"], boxes["scale"], boxes.get("t_range"))
    else:
        ctx.set_moving_boxes(boxes["p0"], boxes["vel"], boxes["scale"])
    ctx.set_moving_cost(True)
    ctx.set_start_times(t0)


def clear_boxes(ctx):
    ctx.set_moving_cost(False)
    ctx.set_start_times(None)
    ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))


def moving_case(oracle_mod, mp, sdf, geo, kind, seed=0):
    """Batch, start times (per row in every second case, one shared scalar in the others), boxes, and — from the oracle
    alone — the condition of tests/test_gpu_moving_cost.py::_share_changed: at least half of the rows (an eighth with
    one box) have a box-lowered corner and a cost more than 1e-6 relative off the static cost."""
    name, spl, m, B = geo
    case = MOVING_GEOMETRIES.index(geo) * len(BOX_LISTS) + BOX_LISTS.index(kind)
    b = problem.make_trajectories(B, m, mp, seed=40 + m + seed, step_len=(0.5, 1.2) if m > 12 else (1.0, 2.0))
    rng = np.random.default_rng(9000 + 10 * case + seed)
    t0 = rng.uniform(0.0, 5.0, B) if case % 2 == 0 else float(rng.uniform(0.0, 5.0))
    boxes = aimed_boxes(b, t0, rng, kind)
    ref, lowered = ref_ext(oracle_mod, b, sdf, MOVING_PARAMS, boxes=boxes, t0=t0)
    c_static = oracle_mod.eval_batch(b.T, b.Df, b.x, sdf, oracle_mod.make_params(**MOVING_PARAMS), nthreads=8)[0]
    share = float(np.mean((lowered > 0) & (np.abs(ref[0] - c_static) > 1e-6 * np.abs(c_static))))
    assert share >= (1 / 8 if kind == "cv1" else 1 / 2), (name, kind, "share of rows the boxes change", share)
    if kind.endswith("clamped"):    # the two validity intervals end inside the span of the row they are aimed at
        span = np.broadcast_to(t0, (B,)) + b.T.sum(axis=1)
        assert np.all(boxes["t_range"][:2, 1] < span.max()) and np.all(boxes["t_range"][:2, 1] > np.min(t0))
    return b, t0, boxes, ref, share


@pytest.mark.parametrize("kind", BOX_LISTS)
@pytest.mark.parametrize("geo", MOVING_GEOMETRIES, ids=[f"GtopMoving-{g[0]}-spl{g[1]}" for g in MOVING_GEOMETRIES])
def test_moving_every_body(world, oracle_mod, geo, kind):
    """GtopMoving<MM> (cv*) / GtopMovingPoly<MM> (poly*) in each geometry, with and without DYN, gradient modes 0 and 1
    (the consistent forms of the moving bodies)."""
    mp, sdf, ctx = world
    name, spl, m, B = geo
    b, t0, boxes, ref, share = moving_case(oracle_mod, mp, sdf, geo, kind)
    fam = "moving polynomial" if "coef" in boxes else "moving constant-velocity"
    try:
        set_boxes(ctx, boxes, t0)
        for dyn in (False, True):
            kw = dict(MOVING_PARAMS, **(DYN if dyn else {}))
            c0 = None
            for mode in (0, 1):
                r = ref if (not dyn and mode == 0) else ref_ext(oracle_mod, b, sdf, kw, mode=mode, boxes=boxes, t0=t0)[0]
                c, g = _device_mode(ctx, b, "f64", 0, spl, kw, mode)
                check_family("moving plus consistent" if mode else fam, c, g, r, "f64",
                             (name, kind, "dyn" if dyn else "ordinary", f"mode {mode}", f"share {share:.2f}"))
                assert c0 is None or np.array_equal(c0, c), "the cost differs between the gradient modes"
                c0 = c
    finally:
        clear_boxes(ctx)


@pytest.mark.parametrize("kind", ["cv32", "poly8-clamped"])
@pytest.mark.parametrize("m", [5, 9, 13])
def test_moving_fused_optimizer_first_evaluation(world, oracle_mod, m, kind):
    """The optimizer-loop bodies with the moving term (MM = GtopMoving<GtopMmaState> and its polynomial form): the first
    evaluation's cost, at clip(x0, lb, ub), to Cmag — as test_fused_optimizer_first_evaluation."""
    mp, sdf, ctx = world
    B = 3
    b = problem.make_trajectories(B, m, mp, seed=7300 + m, step_len=(0.5, 1.2))
    rng = np.random.default_rng(7310 + m)
    t0 = rng.uniform(0.0, 5.0, B)
    boxes = aimed_boxes(b, t0, rng, kind)
    lb, ub = ctx.default_bounds(b.waypoints)
    x0 = b.x + rng.normal(0.0, 0.5, size=b.x.shape)
    xc = problem.Batch(b.waypoints, b.T, b.Df, np.clip(x0, lb, ub), m)
    ref, lowered = ref_ext(oracle_mod, xc, sdf, MOVING_PARAMS, boxes=boxes, t0=t0)
    assert (lowered > 0).any()
    try:
        ctx.set_params(**MOVING_PARAMS)
        set_boxes(ctx, boxes, t0)
        ctx.set_problem(b.T, b.Df)
        _, cost, nev, _ = ctx.optimize_batch_ex(x0, lb, ub, 1)
    finally:
        clear_boxes(ctx)
        ctx.set_params()
    assert (nev == 1).all()
    check_family("moving polynomial" if "coef" in boxes else "moving constant-velocity", cost, ref[1], ref, "f64",
                 ("optimizer loop + moving, first evaluation", m, kind))


# ---- edges ----
@pytest.fixture(scope="module")
def far_scene(gtop, oracle_mod):
    """test_edges' map (origin (-500, 300, 0)) and batch (segments of 0.0009 / 0.0299 / 0.03 / 0.0301 s, rows leaving
    the map), built once."""
    mp = problem.make_map((50, 40, 24), density=0.03, seed=12)
    mp = problem.MapSpec(mp.grid, mp.resolution, np.array([-500.0, 300.0, 0.0]), mp.occupancy)
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    yield mp, sdf, ctx, _edge_batches(mp, sdf)
    ctx.close()


@pytest.mark.parametrize("spl", [3, 6, 0], ids=["GtopMoving-ten-lanes", "GtopMoving-five-lanes-two-per-wave", "GtopMoving-auto"])
def test_edges_moving(far_scene, oracle_mod, spl):
    """The edge batch through the moving geometries that serve six segments, 8 constant-velocity boxes."""
    mp, sdf, ctx, b = far_scene
    rng = np.random.default_rng(93)
    t0 = rng.uniform(0.0, 5.0, len(b.x))
    boxes = aimed_boxes(b, t0, rng, "cv8")
    ref, lowered = ref_ext(oracle_mod, b, sdf, {}, boxes=boxes, t0=t0)
    assert np.mean(lowered > 0) >= 0.5
    try:
        set_boxes(ctx, boxes, t0)
        c, g = _device(ctx, b, "f64", 0, spl, {})
    finally:
        clear_boxes(ctx)
    check_family("moving constant-velocity", c, g, ref, "f64", ("far origin / short segments, moving", spl))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edges_consistent(far_scene, oracle_mod, dtype):
    mp, sdf, ctx, b = far_scene
    bb = b if dtype == "f64" else _f32_batch(b)
    c, g = _device_mode(ctx, bb, dtype, 0, 0, {}, 1)
    check_family(f"consistent {dtype}", c, g, ref_ext(oracle_mod, bb, sdf, {}, mode=1)[0], dtype,
                 ("far origin / short segments, mode 1",))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_signed_field_consistent(gtop, oracle_mod, dtype):
    """test_signed_field's field in mode 1."""
    mp = problem.make_map((48, 40, 24), density=0.05, seed=13)
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.set_field_sign(True, 1.0)
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        ctx.update_sdf_map(mp.obstacle_points())
        dist = ctx.get_sdf().reshape(-1).astype(np.float64)
        assert (dist < 0).any()
        sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
        sdf.dist[:] = dist
        b = problem.make_trajectories(64, 6, mp, seed=14, step_len=(0.5, 1.2))
        bb = b if dtype == "f64" else _f32_batch(b)
        c, g = _device_mode(ctx, bb, dtype, 0, 0, {}, 1)
        check_family(f"consistent {dtype}", c, g, ref_ext(oracle_mod, bb, sdf, {}, mode=1)[0], dtype,
                     ("signed field, mode 1",))
    finally:
        ctx.close()


# ---- the 64-bit-index forms ----
# id: the body; (m, B, waves, samples-per-lane pin, parameters, gradient mode, box list or None)
WIDE_CASES = {
    "WIDE-DYN-spl3-m6": (6, 96, 0, 3, DYN, 0, None),
    "WIDE-five-lanes-one-per-wave-spl6-m9": (9, 60, 0, 6, {}, 0, None),
    "WIDE-two-wavefronts-m10": (10, 40, 1, 0, {}, 0, None),
    "WIDE-chunked-m13": (13, 40, 0, 0, {}, 0, None),
    "WIDE-consistent-spl3-m6": (6, 96, 0, 3, {}, 1, None),
    "WIDE-consistent-spl6-m6": (6, 96, 0, 6, {}, 1, None),
    "WIDE-moving-cv8-spl6-m6": (6, 8, 0, 6, {}, 0, "cv8"),      # (the map is 819 m wide: one box per row)
}


def wide_batch(ms, m, B):
    return problem.make_trajectories(B, m, ms, seed=77 + m, margin=0.15, step_len=(0.5, 1.5) if m <= 6 else (0.3, 0.8))


@pytest.mark.parametrize("case", list(WIDE_CASES))
def test_wide_index_more_bodies(wide, oracle_mod, case):
    ms, ctx, sdf = wide
    m, B, waves, spl, kw, mode, kind = WIDE_CASES[case]
    b = wide_batch(ms, m, B)
    boxes = t0 = None
    if kind:
        rng = np.random.default_rng(78)
        t0 = rng.uniform(0.0, 5.0, B)
        boxes = aimed_boxes(b, t0, rng, kind, rows=np.arange(B))
    ref, lowered = ref_ext(oracle_mod, b, sdf, kw, mode=mode, boxes=boxes, t0=t0)
    try:
        if kind:
            assert np.mean(lowered > 0) >= 0.5
            set_boxes(ctx, boxes, t0)
        c, g = _device_mode(ctx, b, "f64", waves, spl, kw, mode)
    finally:
        if kind:
            clear_boxes(ctx)
    check_family("wide", c, g, ref, "f64", (case,))


def test_wide_index_fused_optimizer_first_evaluation(wide, oracle_mod):
    """The fp64 optimizer loop's 64-bit-index body at five segments: its first evaluation's cost to Cmag."""
    ms, ctx, sdf = wide
    m, B = 5, 3
    b = wide_batch(ms, m, B)
    lb, ub = ctx.default_bounds(b.waypoints)
    x0 = b.x + np.random.default_rng(79).normal(0.0, 0.5, size=b.x.shape)
    ctx.set_params()
    ctx.set_problem(b.T, b.Df)
    _, cost, nev, _ = ctx.optimize_batch_ex(x0, lb, ub, 1)
    assert (nev == 1).all()
    xc = problem.Batch(b.waypoints, b.T, b.Df, np.clip(x0, lb, ub), m)
    ref, _ = ref_ext(oracle_mod, xc, sdf, {})
    check_family("wide", cost, ref[1], ref, "f64", ("WIDE optimizer loop, first evaluation", m, B))
