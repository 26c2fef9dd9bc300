"""The continuous-time clearance certificate on the device (gtop_certify_trajectories_device, gtop_certify_batch,
gtop_select_best_certified_device; csrc/gtop_certify.hip) through grad_traj_optimization_amd.certify.

(1) Device = twin (tests/certify_twin.py) on the shared cases, whose decisions lie further than 1e-9 from a tie:
    verdict and entries 3 .. 7 exactly; hi is, bit for bit, the query's distance at the midpoint behind entry 3; lo within
    LO_BOUND.  The kernel and the twin differ in one place, the velocity (poly_vel has fmas, numpy has none): two
    evaluations of a derivative differ by at most 18 eps of the sum of the absolute values of its terms
    (tests/validate_twin.py), times h <= T / 128 that is under eps P_k, P_k = sum_j |c_j| T^j.  The radius and the box
    ends then round differently, each by at most eps of a coordinate: a box end moves by at most 4 eps (P + C), C the
    map's coordinate scale, a local coordinate by that over res plus its own rounding, the trilinear value — whose
    partial derivative in a local coordinate is a difference of corner values, at most 2 V, V the largest |corner| —
    by at most 6 V times that, plus 16 eps V for the form's own roundings.  LO_BOUND = eps V (24 (P + C) / res + 16).
    Measured worst on the MI355X: 0 (lo came out bit for bit on every row of every case).
(2) Soundness on the device, four kinds of field: lo <= every lookup of gtop_edt_query_device at the points
    gtop_sample_trajectories_device stores at dt = 0.0005; lo <= hi; SAFE => lo > margin; UNSAFE => hi <= margin.
(3) The tunnelling case: a one-voxel wall crossed between two samples of the report at dt_sample = 0.3.
(4) Tightness as a condition; the edge cases; the interface (row independence, host = device, guard words, one graph,
    refusals)."""
import numpy as np
import pytest

from grad_traj_optimization_amd import certify as gc
from tests import certify_twin as ct
from tests import validate_twin as vt

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
EPS = np.finfo(np.float64).eps


def make_ctx(gtop, field, mp):
    ctx = gtop.GtopContext(device=0)
    ctx.set_sdf(field.val, ct.GRID, mp.origin, ct.RES, mp.map_size)
    return ctx


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0", dtype=dtype)


def run_device(ctx, coeff, T, margin, depth, refine):
    import torch
    cert = gc.certify_device(ctx, dev(coeff), dev(T), gc.GtopCertifyOpts(margin, depth, refine))
    torch.cuda.synchronize()
    return cert.cpu().numpy()


@pytest.fixture(scope="module")
def worlds(gtop, oracle_mod):
    """kind -> (Field, MapSpec, context); the twin's certificates of every case, computed once."""
    out = {}
    for kind in ct.FIELDS:
        field, mp = ct.make_field(oracle_mod, kind)
        out[kind] = (field, mp, make_ctx(gtop, field, mp))
    yield out
    for _, _, ctx in out.values():
        ctx.close()


@pytest.fixture(scope="module")
def runs(worlds, oracle_mod):
    out = {}
    for name, (kind, m, B, seed, margin, depth, refine) in ct.CASES.items():
        field, mp, ctx = worlds[kind]
        coeff, T, b = ct.make_rows(oracle_mod, mp, B, m, seed)
        twin = [ct.certify(field, coeff[i], T[i], margin, depth, refine) for i in range(B)]
        out[name] = (field, mp, ctx, coeff, T, b, margin, depth, refine, twin)
    return out


def lo_bound(field, coeff, T):
    c = np.abs(np.asarray(coeff).reshape(-1, 3, 6))
    P = max(np.polyval(c[s, k, ::-1], T[s]) for s in range(len(T)) for k in range(3))
    C = field.e_map / ct.SLACK
    return EPS * np.abs(field.val).max() * (24.0 * (P + C) / field.res + 16.0)


def dense_on_device(ctx, coeff, T, dt=0.0005):
    """The least lookup per row at the stored getTraj samples (static: time -1)."""
    import torch
    c, t = dev(coeff), dev(T)
    cap = int(np.ceil(np.sum(T, axis=-1).max() / dt)) + 2
    stats, samples = ctx.sample_trajectories_device(c, t, dt_sample=dt, max_samples=cap)
    n = stats[:, 8].long()
    assert int(n.max()) <= cap
    pos = samples.reshape(-1, 3)
    dist, _ = ctx.edt_query_device(pos, torch.full((pos.shape[0],), -1.0, dtype=torch.float64, device=pos.device))
    dist = dist.reshape(samples.shape[0], cap)
    live = torch.arange(cap, device=pos.device)[None, :] < n[:, None]
    return torch.where(live, dist, torch.full_like(dist, np.inf)).min(dim=1).values.cpu().numpy()


@pytest.mark.parametrize("name", list(ct.CASES))
def test_device_equals_twin_and_is_sound(runs, name):
    import torch
    field, mp, ctx, coeff, T, b, margin, depth, refine, twin = runs[name]
    got = run_device(ctx, coeff, T, margin, depth, refine)
    dense = dense_on_device(ctx, coeff, T)
    worst = 0.0
    for i, (want, info) in enumerate(twin):
        assert info["tie"] > 1e-9, (i, info["tie"])
        print(f"{name}[{i}] device {got[i]} twin {want} dense {dense[i]:.6g}")
        assert np.array_equal(got[i, [0, 3, 4, 5, 6, 7]], want[[0, 3, 4, 5, 6, 7]]), (i, got[i], want)
        s, tc = info["hi_at"]
        p = ct.position(coeff[i], s, tc)
        d, _ = ctx.edt_query_device(dev(p[None, :]), dev([-1.0]))
        assert got[i, 2] == float(d.cpu()[0]), (i, got[i, 2], d)
        bound = lo_bound(field, coeff[i], T[i])
        err = abs(got[i, 1] - want[1]) if np.isfinite(want[1]) else float(got[i, 1] != want[1])
        worst = max(worst, err / bound)
        assert err <= bound, (i, got[i, 1], want[1], bound)
        # soundness, on the device's own lookups
        assert got[i, 1] <= dense[i] and got[i, 1] <= got[i, 2], (i, got[i], dense[i])
        assert got[i, 0] != 1 or got[i, 1] > margin
        assert got[i, 0] != -1 or got[i, 2] <= margin
    print(f"{name}: worst |lo - twin| / bound = {worst:.3g}")
    torch.cuda.synchronize()


def test_soundness_at_65_rows_per_kind_of_field(worlds, oracle_mod):
    """More rows than one wavefront's worth of workgroups, every kind of field, zero exceptions; and row independence:
    the 65 rows are 5 distinct ones, repeated and permuted, and equal rows give equal bits."""
    for kind, (field, mp, ctx) in worlds.items():
        coeff5, T5, _ = ct.make_rows(oracle_mod, mp, 5, 3, 31)
        perm = np.random.default_rng(2).permutation(65) % 5
        coeff, T = coeff5[perm], T5[perm]
        margin = {"esdf": 0.2, "window": 0.2, "signed": 0.0, "random": 0.3}[kind]
        got = run_device(ctx, coeff, T, margin, 2, 32)
        few = run_device(ctx, coeff5, T5, margin, 2, 32)
        assert np.array_equal(got, few[perm], equal_nan=True), kind
        dense = dense_on_device(ctx, coeff5, T5)
        print(kind, few[:, :3], dense)
        assert np.all(few[:, 1] <= dense) and np.all(few[:, 1] <= few[:, 2]), (kind, few, dense)
        assert np.all(few[few[:, 0] == 1, 1] > margin) and np.all(few[few[:, 0] == -1, 2] <= margin), (kind, few)
        assert np.all(few[:, 6] <= 32)


def test_a_wall_crossed_between_two_samples(gtop, oracle_mod):
    """The sampled report at dt_sample = 0.3 sees nothing (samples at 0, 0.3, 0.6, 0.9 s; the wall is crossed between
    0.496 and 0.557 s) and the plain selection picks the row.  The certificate at max_depth 2, max_refine 64 says
    UNSAFE, entry 4 inside the crossing, and the certified selection refuses the row.  On the CPU first."""
    import torch
    field, mp, coeff, T, b, margin, dt = ct.wall_case(oracle_mod)
    assert dt == 0.3
    t_in, t_out = ct.crossing(field, coeff[0], T[0], margin)
    assert 0.3 < t_in < t_out < 0.6, (t_in, t_out)
    step = float(np.sum(T[0])) / 20000      # the scan's spacing: its first hit is at most that late
    rep_twin, _ = vt.report(oracle_mod, coeff[0], T[0], field.osdf, margin, dt=dt)
    cert_twin, info = ct.certify(field, coeff[0], T[0], margin, 2, 64)
    assert rep_twin[4] == 0 and rep_twin[6] == 0 and cert_twin[0] == -1 and t_in - step <= cert_twin[4] <= t_out
    assert info["tie"] > 1e-9
    ctx = make_ctx(gtop, field, mp)
    try:
        c, t = dev(coeff), dev(T)
        lim = gtop.GtopLimits(margin=margin)
        rep = ctx.validate_device(c, t, lim, dt_sample=dt)
        cert = gc.certify_device(ctx, c, t, gc.GtopCertifyOpts(margin, 2, 64))
        cost = dev([1.0])
        ok, best = ctx.select_best_device(rep, cost, lim)
        ok_c, best_c = gc.select_best_certified_device(ctx, rep, cert, cost, lim, gc.REQUIRE_SAFE)
        ok_n, best_n = gc.select_best_certified_device(ctx, rep, cert, cost, lim, gc.REQUIRE_NOT_UNSAFE)
        torch.cuda.synchronize()
        rep, cert = rep.cpu().numpy()[0], cert.cpu().numpy()[0]
        print("report", rep, "certificate", cert)
        assert rep[4] == 0 and rep[1] > margin                       # the report passes the row
        assert cert[0] == -1 and t_in - step <= cert[4] <= t_out and cert[2] <= margin
        assert np.array_equal(cert[[0, 3, 4, 5, 6, 7]], cert_twin[[0, 3, 4, 5, 6, 7]])
        assert best.tolist() == [0, 1] and ok.tolist() == [1]
        assert best_c.tolist() == [-1, 0] and ok_c.tolist() == [0]
        assert best_n.tolist() == [-1, 0] and ok_n.tolist() == [0]
    finally:
        ctx.close()


def test_rows_with_room_are_safe_without_undecided_leaves(runs):
    """Every row of the shared cases whose dense clearance is at least margin + 0.05 m is SAFE with no undecided leaf at
    max_depth 2, max_refine 256 — on the CPU by the twin first, then on the device."""
    checked = 0
    for name, (field, mp, ctx, coeff, T, b, margin, depth, refine, twin) in runs.items():
        dense = np.array([ct.dense_clearance(field, coeff[i], T[i], 2001)[0] for i in range(len(T))])
        rows = np.flatnonzero(dense >= margin + 0.05)
        if not len(rows):
            continue
        for i in rows:
            want, _ = ct.certify(field, coeff[i], T[i], margin, 2, 256)
            assert want[0] == 1 and want[5] == 0, (name, i, want)
        got = run_device(ctx, coeff[rows], T[rows], margin, 2, 256)
        assert np.all(got[:, 0] == 1) and np.all(got[:, 5] == 0), (name, got)
        checked += len(rows)
    assert checked >= 4, checked


def test_edge_cases(runs, worlds, oracle_mod):
    field, mp, ctx, coeff, T, b, margin, depth, refine, twin = runs["esdf_m3"]
    # a curve that leaves the map: lo = -inf, UNSAFE for any margin >= -1
    out = coeff[:1].copy().reshape(1, 3, 3, 6)
    out[0, 1, 0, 0] += 6.0                                    # the middle segment, 6 m along x: beyond max_range
    out = out.reshape(1, 3, 18)
    for mg in (-1.0, 0.3):
        got = run_device(ctx, out, T[:1], mg, 2, 16)[0]
        assert got[0] == -1 and got[1] == -np.inf and got[2] == -1.0 and got[4] >= 0, got
    # max_refine = 0 and max_depth = 0: level 0 alone, 64 m midpoints, against the twin
    for d, r in ((2, 0), (0, 256)):
        got = run_device(ctx, coeff, T, margin, d, r)
        for i in range(len(T)):
            want, info = ct.certify(field, coeff[i], T[i], margin, d, r)
            assert info["tie"] > 1e-9 and want[6] == 0
            assert np.array_equal(got[i, [0, 3, 4, 5, 6, 7]], want[[0, 3, 4, 5, 6, 7]]), (d, r, i, got[i], want)
    # a zero segment time: the segment is one point, 64 times
    Tz, cz = T[1:2].copy(), coeff[1:2].copy()
    Tz[0, 1] = 0.0
    got = run_device(ctx, cz, Tz, margin, 2, 64)[0]
    want, _ = ct.certify(field, cz[0], Tz[0], margin, 2, 64)
    assert np.array_equal(got[[0, 3, 4, 5, 6, 7]], want[[0, 3, 4, 5, 6, 7]]) and got[7] == Tz[0, 0] + Tz[0, 2], (got, want)
    # a shared T (time stride 0): every row flown with row 0's times
    shared = run_device(ctx, coeff, T[0], margin, depth, refine)
    tiled = run_device(ctx, coeff, np.tile(T[0], (len(T), 1)), margin, depth, refine)
    assert np.array_equal(shared, tiled, equal_nan=True) and np.array_equal(shared[0], run_device(
        ctx, coeff[:1], T[:1], margin, depth, refine)[0], equal_nan=True)


def test_host_form_guard_words_and_row_independence(gtop, runs):
    import torch
    field, mp, ctx, coeff, T, b, margin, depth, refine, twin = runs["esdf_m7"]
    opts = gc.GtopCertifyOpts(margin, depth, refine)
    ctx.set_problem(b.T, b.Df)
    x, Df, Td = dev(b.x), dev(b.Df.reshape(-1, 18)), dev(b.T)
    c = ctx.coefficients_device(x, Df, Td)
    B = len(b.x)
    guard = -12345.0
    buf = torch.full((B + 2, 8), guard, dtype=torch.float64, device=x.device)
    gc.certify_device(ctx, c, Td, opts, cert=buf[1:B + 1])
    torch.cuda.synchronize()
    assert torch.all(buf[0] == guard) and torch.all(buf[B + 1] == guard)
    host = gc.certify_batch(ctx, b.x, opts)
    assert np.array_equal(host, buf[1:B + 1].cpu().numpy(), equal_nan=True)
    assert np.array_equal(gc.certify_batch(ctx, b.x[:1], opts), host[:1], equal_nan=True)      # a prefix of the rows
    # permutation and another B: the same rows, the same bits
    perm = np.array([1, 0, 1, 1, 0, 0, 1])
    again = gc.certify_device(ctx, c[dev(perm)].contiguous(), Td[dev(perm)].contiguous(), opts)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy(), host[perm], equal_nan=True)


def test_one_graph_follows_a_field_update(gtop, oracle_mod):
    """coefficients -> certificate -> certified selection, captured once; replayed after the map was rebuilt from other
    points, it gives what an eager run on the new field gives."""
    import torch
    from grad_traj_optimization_amd import problem
    mp = problem.make_map(ct.GRID, ct.RES, density=0.04, seed=5, box_vox=(2, 5))
    b = problem.make_trajectories(9, 3, mp, seed=11, step_len=(0.6, 1.2), margin=0.5)
    ctx = gtop.GtopContext(device=0)
    try:
        ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        pts = mp.obstacle_points()
        ctx.update_sdf_map(pts)
        x, Df, T = dev(b.x), dev(b.Df.reshape(-1, 18)), dev(b.T)
        lim, opts = gtop.GtopLimits(margin=0.2), gc.GtopCertifyOpts(0.2, 2, 64)
        cost = dev(np.arange(9, 0, -1.0))
        coeff = torch.empty(9, 3, 18, dtype=torch.float64, device=x.device)
        rep = torch.zeros(9, 12, dtype=torch.float64, device=x.device)
        cert = torch.zeros(9, 8, dtype=torch.float64, device=x.device)
        best = torch.zeros(2, dtype=torch.int32, device=x.device)

        def chain():
            ctx.coefficients_device(x, Df, T, coeff=coeff)
            ctx.validate_device(coeff, T, lim, report=rep)
            gc.certify_device(ctx, coeff, T, opts, cert=cert)
            gc.select_best_certified_device(ctx, rep, cert, cost, lim, gc.REQUIRE_SAFE, want_pass=False, best=best)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # warm-up outside the capture
            chain()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        eager = cert.clone(), best.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        cert.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cert, eager[0]) and torch.equal(best, eager[1])
        first = cert.cpu().numpy().copy()
        safe = (first[:, 0] == 1) & (rep.cpu().numpy()[:, 4] == 0) & (rep.cpu().numpy()[:, 6] == 0)
        assert best.tolist() == [int(np.flatnonzero(safe)[-1]) if safe.any() else -1, int(safe.sum())]
        ctx.update_sdf_map(pts[::3] + (0.4, 0.2, 0.0))          # another map, the same buffers
        graph.replay()
        torch.cuda.synchronize()
        second, best2 = cert.cpu().numpy().copy(), best.clone()
        chain()
        torch.cuda.synchronize()
        assert np.array_equal(second, cert.cpu().numpy(), equal_nan=True) and torch.equal(best2, best)
        assert not np.array_equal(first[:, 1], second[:, 1], equal_nan=True)
    finally:
        ctx.close()


def test_refusals_launch_nothing_and_an_empty_batch_is_accepted(gtop, runs):
    import torch
    field, mp, ctx, coeff, T, b, margin, depth, refine, twin = runs["esdf_m3"]
    c, t = dev(coeff), dev(T)
    B, m = coeff.shape[:2]
    guard = -12345.0
    cert = torch.full((B, 8), guard, dtype=torch.float64, device=c.device)
    L, h = ctx._L, ctx._h
    good = gc.GtopCertifyOpts(margin, 2, 16)

    def refused(code, fn):
        with pytest.raises(gtop.GtopError) as ei:
            fn()
        assert ei.value.code == code, ei.value

    for bad in ((np.nan, 2, 16), (np.inf, 2, 16), (0.1, -1, 16), (0.1, 4, 16), (0.1, 2, -1)):
        refused(ERR_INVALID, lambda: gc.certify_device(ctx, c, t, gc.GtopCertifyOpts(*bad), cert=cert))
    ctx.set_problem(b.T, b.Df)
    refused(ERR_INVALID, lambda: gc.certify_batch(ctx, b.x, gc.GtopCertifyOpts(np.nan, 2, 16)))
    refused(ERR_INVALID, lambda: gc.certify_batch(ctx, np.tile(b.x, (2, 1)), good))         # more rows than the problem
    vp = lambda a: a.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (("B", B), ("m", m), ("coeff", vp(c)), ("T", vp(t)), ("stride", m),
                                                     ("opt", good), ("cert", vp(cert)), ("stream", None))]
    for kw in (dict(coeff=None), dict(T=None), dict(cert=None), dict(opt=None), dict(B=-1), dict(m=1), dict(m=228),
               dict(stride=1), dict(stride=m + 1)):
        assert L.gtop_certify_trajectories_device(h, *args(**kw)) == ERR_INVALID, kw
    rep = torch.zeros(B, 12, dtype=torch.float64, device=c.device)
    cost = torch.zeros(B, dtype=torch.float64, device=c.device)
    best = torch.full((2,), 7, dtype=torch.int32, device=c.device)
    lim = gtop.GtopLimits(margin=margin)
    for require in (0, 3):
        refused(ERR_INVALID, lambda: gc.select_best_certified_device(ctx, rep, cert, cost, lim, require, best=best))
    refused(ERR_INVALID, lambda: gc.select_best_certified_device(ctx, rep, cert, cost, gtop.GtopLimits(margin=np.nan),
                                                                 best=best))
    assert L.gtop_select_best_certified_device(h, B, vp(rep), None, vp(cost), lim, 1, None, vp(best), None) == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(cert == guard) and best.tolist() == [7, 7]
    # no field resident: GTOP_ERR_STATE
    bare = gtop.GtopContext(device=0)
    try:
        refused(ERR_STATE, lambda: gc.certify_device(bare, c, t, good, cert=cert))
    finally:
        bare.close()
    # B = 0: nothing launched; the selection writes {-1, 0}
    e3, e2 = (torch.empty(0, m, 18, dtype=torch.float64, device=c.device),
              torch.empty(0, m, dtype=torch.float64, device=c.device))
    assert gc.certify_device(ctx, e3, e2, good).shape == (0, 8)
    e = torch.empty(0, dtype=torch.float64, device=c.device)
    _, best0 = gc.select_best_certified_device(ctx, e.reshape(0, 12), e.reshape(0, 8), e, lim, want_pass=False)
    torch.cuda.synchronize()
    assert best0.tolist() == [-1, 0] and torch.all(cert == guard)
