"""The certificate against the moving boxes on the device (gtop_certify_moving_device, gtop_certify_moving_batch;
csrc/gtop_certify.hip, traj_certify_moving_kernel) through grad_traj_optimization_amd.certify.

(1) Device = twin (tests/certify_moving_twin.py) on cases whose decisions lie further than 1e-9 from a tie: verdict and
    entries 3 .. 7 exactly; hi is, bit for bit, the query's distance at (the midpoint behind entry 3, t0 + entry 3); lo
    within LO_BOUND of tests/test_gpu_certify.py plus MOVING_BOUND.  Beside the velocity (LO_BOUND) the kernel has fmas
    where numpy has none in three places, all in the shared lookup.  With C the map's coordinate scale, Cb the largest
    |face coordinate| a box reaches (|p0| + |vel| tau + scale / 2; for a polynomial list the sum of |c_j| tau^j), and
    D <= C + Cb the largest distance from a corner voxel's centre to a face:
      the centre p0 + vel tau of a constant-velocity box: one rounding of the product less, at most eps Cb; each face
        c +- scale / 2 then rounds from another c: at most 2 eps Cb on a face (a polynomial box's centre is the same
        fma Horner on both sides, its radius unfused on both: nothing);
      the corner voxel's centre (i + 0.5) res + origin: at most eps C;
      so a per-axis distance |centre - face| differs by at most 2 eps Cb + eps C + 2 eps D (its own subtraction rounds
        on both sides), the vector of three by sqrt(3) times that in norm;
      the squared sum: three products and two additions with or without intermediate roundings, at most 3 eps of the
        sum, 1.5 eps D on its root, and the root's own rounding on both sides: under 4 eps D.
    A corner value min(static, distance) therefore moves by at most eps (sqrt(3) (2 Cb + C + 2 D) + 4 D) <=
    eps (12 Cb + 10 C), and the trilinear form, a convex combination of corner values, by no more.
    MOVING_BOUND = eps (12 Cb + 10 C).  The measured worst ratio is printed.
(2) Soundness on the device: lo <= every gtop_edt_query_device value at the points gtop_sample_trajectories_device
    stores at dt = 0.0005, each at box time t0 + its sample time; lo <= hi; SAFE => lo > margin; UNSAFE => hi <= margin;
    equal rows give equal bits whatever their place, with per-row start times.
(3) Lists one box past a chunk (33 polynomial, 65 constant-velocity boxes), the decisive box last.
(4) The tunnelling case.  (5) Equivalences with the static certificate.  (6) The interface."""
import numpy as np
import pytest

from grad_traj_optimization_amd import certify as gc
from tests import certify_moving_twin as cm
from tests import certify_twin as ct
from tests.test_gpu_certify import dev, lo_bound, make_ctx

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
EPS = np.finfo(np.float64).eps
COLS = [0, 3, 4, 5, 6, 7]

# name: (field kind, m, rows, seed, polynomial list, boxes of shared_boxes, t0, margin, max_depth, max_refine)
CASES = {
    "esdf_m2_cv3": ("esdf", 2, 3, 42, False, [0, 1, 2], 0.0, 0.2, 2, 16),
    "esdf_m3_poly3": ("esdf", 3, 2, 43, True, [0, 1, 2], 2.0, 0.2, 2, 16),
    "signed_m7_cv1": ("signed", 7, 2, 47, False, [1], 2.0, 0.1, 1, 8),
    "signed_m3_poly1": ("signed", 3, 3, 43, True, [0], 0.5, 0.15, 2, 12),
}


def opts(margin, depth, refine, use_boxes=True, reserved=0):
    return gc.GtopCertifyMovingOpts(margin, depth, refine, use_boxes, reserved)


def run_moving(ctx, coeff, T, o):
    import torch
    cert = gc.certify_moving_device(ctx, dev(coeff), dev(T), o)
    torch.cuda.synchronize()
    return cert.cpu().numpy()


def run_static(ctx, coeff, T, margin, depth, refine):
    import torch
    cert = gc.certify_device(ctx, dev(coeff), dev(T), gc.GtopCertifyOpts(margin, depth, refine))
    torch.cuda.synchronize()
    return cert.cpu().numpy()


def moving_bound(field, boxes, tau_max):
    C = field.e_map / ct.SLACK
    if boxes.poly:
        a = np.abs(boxes.coef)
        reach = sum(a[..., j] * tau_max ** j for j in range(6)).max()
    else:
        reach = (np.abs(boxes.p0) + np.abs(boxes.vel) * tau_max).max()
    Cb = reach + 0.5 * boxes.scale.max()
    return EPS * (12.0 * Cb + 10.0 * C)


def dense_on_device(ctx, coeff, T, t0, dt=0.0005):
    """The least lookup per row at the stored getTraj samples, sample k at box time t0[row] + (k additions of dt)."""
    import torch
    c, t = dev(coeff), dev(T)
    cap = int(np.ceil(np.sum(T, axis=-1).max() / dt)) + 2
    stats, samples = ctx.sample_trajectories_device(c, t, dt_sample=dt, max_samples=cap)
    n = stats[:, 8].long()
    assert int(n.max()) <= cap
    times = np.concatenate([[0.0], np.cumsum(np.full(cap - 1, dt))])
    tau = dev((np.asarray(t0, dtype=np.float64).reshape(-1, 1) + times[None, :]).reshape(-1))
    dist, _ = ctx.edt_query_device(samples.reshape(-1, 3), tau)
    dist = dist.reshape(samples.shape[0], cap)
    live = torch.arange(cap, device=dist.device)[None, :] < n[:, None]
    return torch.where(live, dist, torch.full_like(dist, np.inf)).min(dim=1).values.cpu().numpy()


@pytest.fixture(scope="module")
def worlds(gtop, oracle_mod):
    """kind -> (Field, MapSpec, context)"""
    out = {}
    for kind in ("esdf", "signed"):
        field, mp = ct.make_field(oracle_mod, kind)
        out[kind] = (field, mp, make_ctx(gtop, field, mp))
    yield out
    for _, _, ctx in out.values():
        ctx.close()


@pytest.fixture
def clean(worlds):
    """The worlds with no boxes and no start times, before and after."""
    def reset():
        for _, _, ctx in worlds.values():
            ctx.set_moving_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
            ctx.set_start_times(None)
    reset()
    yield worlds
    reset()


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_twin_and_is_sound(clean, oracle_mod, name):
    kind, m, B, seed, poly, pick, t0, margin, depth, refine = CASES[name]
    field, mp, ctx = clean[kind]
    boxes = cm.shared_boxes(mp, poly).take(pick)
    coeff, T, _ = ct.make_rows(oracle_mod, mp, B, m, seed)
    boxes.set_on(ctx)
    ctx.set_start_times(t0)
    got = run_moving(ctx, coeff, T, opts(margin, depth, refine))
    dense = dense_on_device(ctx, coeff, T, np.full(B, t0))
    worst = 0.0
    for i in range(B):
        want, info = cm.certify(field, boxes, coeff[i], T[i], t0, margin, depth, refine)
        assert info["tie"] > 1e-9, (i, info["tie"])
        print(f"{name}[{i}] device {got[i]} twin {want} dense {dense[i]:.6g}")
        assert np.array_equal(got[i, COLS], want[COLS]), (i, got[i], want)
        s, tc = info["hi_at"]
        pos = ct.position(coeff[i], s, tc)
        d, _ = ctx.edt_query_device(dev(pos[None, :]), dev([t0 + got[i, 3]]))
        assert got[i, 2] == float(d.cpu()[0]), (i, got[i, 2], d)
        bound = lo_bound(field, coeff[i], T[i]) + moving_bound(field, boxes, abs(t0) + want[7])
        err = abs(got[i, 1] - want[1]) if np.isfinite(want[1]) else float(got[i, 1] != want[1])
        worst = max(worst, err / bound)
        assert err <= bound, (i, got[i, 1], want[1], bound)
        assert got[i, 1] <= dense[i] and got[i, 1] <= got[i, 2], (i, got[i], dense[i])
        assert got[i, 0] != 1 or got[i, 1] > margin
        assert got[i, 0] != -1 or got[i, 2] <= margin
    print(f"{name}: worst |lo - twin| / bound = {worst:.3g}")


@pytest.mark.parametrize("poly", [False, True], ids=["const_vel", "polynomial"])
def test_soundness_and_row_independence_at_65_rows(clean, oracle_mod, poly):
    """65 rows made of 5 distinct ones, permuted, each with its own start time (one per row of the batch)."""
    import torch
    for kind, (field, mp, ctx) in clean.items():
        cm.shared_boxes(mp, poly).set_on(ctx)
        coeff5, T5, _ = ct.make_rows(oracle_mod, mp, 5, 3, 31)
        start5 = np.array([0.0, 0.5, 1.0, 2.0, 3.0])
        perm = np.random.default_rng(2).permutation(65) % 5
        margin = {"esdf": 0.2, "signed": 0.0}[kind]
        t65, t5 = dev(start5[perm]), dev(start5)
        ctx.set_start_times_device(t65)
        got = run_moving(ctx, coeff5[perm], T5[perm], opts(margin, 2, 32))
        ctx.set_start_times_device(t5)
        few = run_moving(ctx, coeff5, T5, opts(margin, 2, 32))
        static = run_static(ctx, coeff5, T5, margin, 2, 32)
        dense = dense_on_device(ctx, coeff5, T5, start5)
        torch.cuda.synchronize()
        ctx.set_start_times(None)
        print(kind, few[:, :3], dense)
        assert np.array_equal(got, few[perm], equal_nan=True), kind
        assert np.all(few[:, 1] <= dense) and np.all(few[:, 1] <= few[:, 2]), (kind, few, dense)
        assert np.all(few[few[:, 0] == 1, 1] > margin) and np.all(few[few[:, 0] == -1, 2] <= margin), (kind, few)
        assert np.all(few[:, 1] <= static[:, 1]) and np.all(few[:, 6] <= 32)


@pytest.mark.parametrize("poly,count", [(True, 33), (False, 65)], ids=["polynomial_33", "const_vel_65"])
def test_a_list_one_box_past_a_chunk(clean, oracle_mod, poly, count):
    """The decisive box is the last of the list, alone in its chunk; the others stand 60 m away, further than any value
    of the field: the list gives what the decisive box alone gives."""
    field, mp, ctx = clean["esdf"]
    coeff, T, _ = ct.make_rows(oracle_mod, mp, 3, 3, 43)
    one = cm.shared_boxes(mp, poly).take([0])
    rng = np.random.default_rng(9)
    far = np.array([60.0, 0.0, 0.0]) + rng.uniform(-1.0, 1.0, (count - 1, 3))
    scale = np.concatenate([np.full((count - 1, 3), 0.5), one.scale])
    if poly:
        coef = np.zeros((count, 3, 6))
        coef[:-1, :, 0], coef[:-1, :, 1] = far, rng.uniform(-0.1, 0.1, (count - 1, 3))
        coef[-1] = one.coef[0]
        many = cm.Boxes.polynomial(coef, scale)
    else:
        many = cm.Boxes.const_vel(np.concatenate([far, one.p0]),
                                  np.concatenate([rng.uniform(-0.1, 0.1, (count - 1, 3)), one.vel]), scale)
    one.set_on(ctx)
    alone = run_moving(ctx, coeff, T, opts(0.2, 2, 16))
    static = run_static(ctx, coeff, T, 0.2, 2, 16)
    many.set_on(ctx)
    got = run_moving(ctx, coeff, T, opts(0.2, 2, 16))
    print(got, alone)
    assert np.array_equal(got, alone, equal_nan=True)
    assert not np.array_equal(alone[:, 1], static[:, 1])          # the decisive box decides something


def test_the_plate_crosses_between_two_samples(gtop, oracle_mod):
    """The report with use_boxes passes the row at dt_sample = 0.3, the static certificate says SAFE; the moving
    certificate says UNSAFE and the certified selection refuses the row under both `require` values."""
    import torch
    for poly in (False, True):
        field, mp, coeff, T, b, margin, dt, boxes, t0 = cm.tunnel_case(oracle_mod, poly)
        want, info = cm.certify(field, boxes, coeff[0], T[0], t0, margin, 2, 64)
        assert want[0] == -1 and info["tie"] > 1e-9
        ctx = make_ctx(gtop, field, mp)
        try:
            boxes.set_on(ctx)
            ctx.set_start_times(t0)
            c, t = dev(coeff), dev(T)
            lim = gtop.GtopLimits(margin=margin, use_boxes=True)
            rep = ctx.validate_device(c, t, lim, dt_sample=dt)
            static = gc.certify_device(ctx, c, t, gc.GtopCertifyOpts(margin, 2, 64))
            moving = gc.certify_moving_device(ctx, c, t, opts(margin, 2, 64))
            cost = dev([1.0])
            picks = {}
            for name, cert in (("static", static), ("moving", moving)):
                for require in (gc.REQUIRE_SAFE, gc.REQUIRE_NOT_UNSAFE):
                    ok, best = gc.select_best_certified_device(ctx, rep, cert, cost, lim, require)
                    picks[name, require] = (ok, best)
            torch.cuda.synchronize()
            rep, static, moving = rep.cpu().numpy()[0], static.cpu().numpy()[0], moving.cpu().numpy()[0]
            print("report", rep, "static", static, "moving", moving)
            assert rep[0] == 4 and rep[4] == 0 and rep[1] > margin           # the report passes the row
            assert static[0] == 1 and static[1] > 2.0
            assert moving[0] == -1 and moving[2] <= margin and np.array_equal(moving[COLS], want[COLS])
            for require in (gc.REQUIRE_SAFE, gc.REQUIRE_NOT_UNSAFE):
                ok, best = picks["static", require]
                assert best.tolist() == [0, 1] and ok.tolist() == [1]
                ok, best = picks["moving", require]
                assert best.tolist() == [-1, 0] and ok.tolist() == [0]
        finally:
            ctx.close()


def test_equivalences_with_the_static_certificate(clean, oracle_mod):
    import torch
    field, mp, ctx = clean["esdf"]
    coeff, T, _ = ct.make_rows(oracle_mod, mp, 3, 3, 43)
    static = run_static(ctx, coeff, T, 0.2, 2, 16)
    # an empty list, with and without use_boxes
    for use in (False, True):
        assert np.array_equal(run_moving(ctx, coeff, T, opts(0.2, 2, 16, use)), static, equal_nan=True), use
    # a list that is not asked for
    boxes = cm.shared_boxes(mp, False)
    boxes.set_on(ctx)
    assert np.array_equal(run_moving(ctx, coeff, T, opts(0.2, 2, 16, False)), static, equal_nan=True)
    with_boxes = run_moving(ctx, coeff, T, opts(0.2, 2, 16))
    assert not np.array_equal(with_boxes, static, equal_nan=True)
    # a shared start time is that value per row
    ctx.set_start_times(1.5)
    shared = run_moving(ctx, coeff, T, opts(0.2, 2, 16))
    ctx.set_start_times(np.full(3, 1.5))
    assert np.array_equal(run_moving(ctx, coeff, T, opts(0.2, 2, 16)), shared, equal_nan=True)
    assert not np.array_equal(shared, with_boxes, equal_nan=True)
    # box times that stay negative: static only, as the query has it
    early = dev(-(np.sum(T, axis=1) + 1.0))
    ctx.set_start_times_device(early)
    assert np.array_equal(run_moving(ctx, coeff, T, opts(0.2, 2, 16)), static, equal_nan=True)
    torch.cuda.synchronize()
    ctx.set_start_times(None)
    # boxes far from every row: the static verdicts, lo no larger
    for poly in (False, True):
        near = cm.shared_boxes(mp, poly)
        if poly:
            coef = near.coef.copy()
            coef[:, 0, 0] += 60.0
            cm.Boxes.polynomial(coef, near.scale, near.t_range).set_on(ctx)
        else:
            cm.Boxes.const_vel(near.p0 + (60.0, 0.0, 0.0), near.vel, near.scale).set_on(ctx)
        far = run_moving(ctx, coeff, T, opts(0.2, 2, 16))
        assert np.array_equal(far[:, 0], static[:, 0]) and np.all(far[:, 1] <= static[:, 1]), (poly, far, static)


def test_host_form_guard_rows_and_one_graph(gtop, oracle_mod):
    """Host = device form; the rows either side of cert stay untouched; coefficients -> moving certificate -> certified
    selection, captured once and replayed after the boxes' values and the start-time buffer changed, gives what an
    eager run gives."""
    import torch
    field, mp = ct.make_field(oracle_mod, "esdf")
    _, _, b = ct.make_rows(oracle_mod, mp, 4, 3, 43)
    B = len(b.x)
    ctx = make_ctx(gtop, field, mp)
    try:
        boxes = cm.shared_boxes(mp, True)
        boxes.set_on(ctx)
        ctx.set_problem(b.T, b.Df)
        x, Df, T = dev(b.x), dev(b.Df.reshape(-1, 18)), dev(b.T)
        start = dev(np.array([0.0, 0.7, 1.4, 2.1]))
        ctx.set_start_times_device(start)
        o = opts(0.2, 2, 16)
        coeff = ctx.coefficients_device(x, Df, T)
        guard = -12345.0
        buf = torch.full((B + 2, 8), guard, dtype=torch.float64, device=x.device)
        gc.certify_moving_device(ctx, coeff, T, o, cert=buf[1:B + 1])
        torch.cuda.synchronize()
        assert torch.all(buf[0] == guard) and torch.all(buf[B + 1] == guard)
        host = gc.certify_moving_batch(ctx, b.x, o)
        assert np.array_equal(host, buf[1:B + 1].cpu().numpy(), equal_nan=True)
        assert np.array_equal(gc.certify_moving_batch(ctx, b.x[:2], o), host[:2], equal_nan=True)   # the problem's batch serves

        lim = gtop.GtopLimits(margin=0.2, use_boxes=True)
        cost = dev(np.arange(B, 0, -1.0))
        rep = torch.zeros(B, 12, dtype=torch.float64, device=x.device)
        cert = torch.zeros(B, 8, dtype=torch.float64, device=x.device)
        best = torch.zeros(2, dtype=torch.int32, device=x.device)

        def chain():
            ctx.coefficients_device(x, Df, T, coeff=coeff)
            ctx.validate_device(coeff, T, lim, report=rep)
            gc.certify_moving_device(ctx, coeff, T, o, cert=cert)
            gc.select_best_certified_device(ctx, rep, cert, cost, lim, gc.REQUIRE_NOT_UNSAFE, want_pass=False, best=best)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # warm-up outside the capture
            chain()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        first = cert.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        cert.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cert, first)
        coef = boxes.coef.copy()                 # the same kind and length, other values; other start times
        coef[:, :, 0] += (0.3, -0.2, 0.1)
        cm.Boxes.polynomial(coef, boxes.scale, boxes.t_range).set_on(ctx)
        start.copy_(dev(np.array([1.0, 0.2, 0.0, 2.6])))
        graph.replay()
        torch.cuda.synchronize()
        second, best2 = cert.cpu().numpy().copy(), best.clone()
        chain()
        torch.cuda.synchronize()
        assert np.array_equal(second, cert.cpu().numpy(), equal_nan=True) and torch.equal(best2, best)
        assert not np.array_equal(first.cpu().numpy()[:, 1], second[:, 1], equal_nan=True)
    finally:
        ctx.close()


def test_refusals_launch_nothing_and_an_empty_batch_is_accepted(gtop, clean, oracle_mod):
    import torch
    field, mp, ctx = clean["esdf"]
    coeff, T, b = ct.make_rows(oracle_mod, mp, 3, 3, 43)
    cm.shared_boxes(mp, False).set_on(ctx)
    c, t = dev(coeff), dev(T)
    B, m = coeff.shape[:2]
    guard = -12345.0
    cert = torch.full((B, 8), guard, dtype=torch.float64, device=c.device)
    L, h = ctx._L, ctx._h
    good = opts(0.2, 2, 16)

    def refused(code, fn):
        with pytest.raises(gtop.GtopError) as ei:
            fn()
        assert ei.value.code == code, ei.value

    for bad in ((np.nan, 2, 16), (np.inf, 2, 16), (0.1, -1, 16), (0.1, 4, 16), (0.1, 2, -1), (0.1, 2, 16, True, 1),
                (0.1, 2, 16, False, 7)):
        refused(ERR_INVALID, lambda: gc.certify_moving_device(ctx, c, t, opts(*bad), cert=cert))
    vp = lambda a: a.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (("B", B), ("m", m), ("coeff", vp(c)), ("T", vp(t)), ("stride", m),
                                                     ("opt", good), ("cert", vp(cert)), ("stream", None))]
    for kw in (dict(coeff=None), dict(T=None), dict(cert=None), dict(opt=None), dict(B=-1), dict(m=1), dict(m=228),
               dict(stride=1), dict(stride=m + 1)):
        assert L.gtop_certify_moving_device(h, *args(**kw)) == ERR_INVALID, kw
    # a start-time count that is neither 0, 1 nor B; for the batch form the problem's batch serves too
    ctx.set_start_times(np.array([0.0, 1.0]))
    refused(ERR_INVALID, lambda: gc.certify_moving_device(ctx, c, t, good, cert=cert))
    ctx.set_problem(b.T, b.Df)
    refused(ERR_INVALID, lambda: gc.certify_moving_batch(ctx, b.x, good))
    ctx.set_start_times(np.array([0.0, 1.0, 2.0]))
    assert gc.certify_moving_batch(ctx, b.x[:2], good).shape == (2, 8)
    refused(ERR_INVALID, lambda: gc.certify_moving_batch(ctx, b.x, opts(np.nan, 2, 16)))
    refused(ERR_INVALID, lambda: gc.certify_moving_batch(ctx, np.tile(b.x, (2, 1)), good))
    ctx.set_start_times(None)
    torch.cuda.synchronize()
    assert torch.all(cert == guard)
    bare = gtop.GtopContext(device=0)           # no field resident
    try:
        refused(ERR_STATE, lambda: gc.certify_moving_device(bare, c, t, good, cert=cert))
    finally:
        bare.close()
    e3, e2 = (torch.empty(0, m, 18, dtype=torch.float64, device=c.device),
              torch.empty(0, m, dtype=torch.float64, device=c.device))
    assert gc.certify_moving_device(ctx, e3, e2, good).shape == (0, 8)
    torch.cuda.synchronize()
    assert torch.all(cert == guard)
