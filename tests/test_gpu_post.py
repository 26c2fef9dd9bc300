"""gtop_setup.hip (setup_paths_kernel, coefficients_kernel, eval_trajectories_kernel: rows f3 / f4 of DESIGN section 0)
against the exact twin of tests/post_twin.py, through the device entries gtop_setup_paths_device,
gtop_coefficients_device, gtop_eval_trajectories_device and gtop_sample_trajectories_device.

DECISIONS are compared with ==: time_sum (stats[0]), the sample count (stats[8]), the segment and the local time of
every sample (read back bit for bit through the segment probe: x = the segment's index, y = t), T / Df / x0 of the
set-up, the zeros behind a trajectory's count or cap.  The kernel performs the reference's own additions (lane l adds
dt l times to the carried base, the base advances by 64 additions), so nothing is excused.

VALUES are held to |gpu - exact| <= K * u * magnitude, u = 2^-53, the magnitude being the twin's (the expression with
absolute values, sums for differences).  K counts the roundings of gtop_setup.hip / poly_eval along the longest chain;
every rounding is at most u of a partial result, which the magnitude bounds.  Second-order terms (n^2 u^2) are far
below one unit of any K.

  * points, K_POINT = 16.  poly_eval: t2 (1), t4 = t2 * t2 (3), t5 = t4 * t (4), times c5 (5): every term within 5 u
    of |c_i| |t|^i; the six additions (the first, to 0, is exact) add at most 5 u of the magnitude: 10 u.
  * length, K_LENGTH(n) = 26 + ceil(n / 64).  The two endpoint errors of a piece pass through the norm undiminished:
    16 u of the piece's magnitude (the norm of mag_k + mag_{k-1} per axis).  The norm itself: three differences (1 u
    each), squares and two additions (3 u of the sum of squares), halved by the square root, which rounds once: 4 u of
    the piece.  The sum: the 64-lane tree (6 levels) per chunk, then a serial sum over the ceil(n / 64) chunks, each
    rounding within u of the length.
  * jerk, K_JERK = 24.  Tp[5] = (T T)(T T) T is 4 roundings; the integer factors are exact; times Tp and the division:
    6; times c_i: 7; the column's three additions (first exact): 9; times c_j: 10; three columns: 12; three axes: 14;
    the 64-lane tree: 20; the sum over at most four passes of 64 segments: 23.
  * acc cost, K_ACC = 16.  2 c exact, squares (1), two additions (3), times T (4), tree (10), passes (13).
  * max velocity / acceleration, K_MAX = 12.  A term Tp[i] ((i+1) c_{i+1}): Tp[4] 3 roundings, the factor 1, the
    product 1: 5 u; five additions, the first exact: 9 u of the axis magnitude, which the norm passes on; the norm's
    own squares, additions and root: 2.5 u.  (Acceleration: a term 4 u, three additions, 9.5 u in all.)  A maximum
    moves by no more than its largest element's error: the magnitude is the largest of the segments' magnitudes.
  * mean velocity / acceleration, K_MEAN(c) = 22 + c with c the largest per-segment step count: the norm's 11.5 u,
    c - 1 roundings of the repeated `+= vn`, the tree (6), the passes (3), the division (1).
  * coefficients, K_COEF = 256.  c0, c1, c2 are exact (0.5 a0 is).  P = pT - p0 - v0 T - a0 T^2 / 2: T^2 (1), the
    products (2 on the a0 term), three subtractions: 5 u of Pm = |pT| + |p0| + |v0| T + |a0| T^2 / 2; V: 4 u of Vm,
    A: 3 u of Am.  c5 = (6 P - 3 V + A / 2) (iT^3 iT iT): the factor 6 rounds once (6), two additions (8); iT = fl(1 / T)
    enters the power five times, so its one rounding counts five times, and the power has four products: 9; the last
    product: 18 u of the CLOSED FORM's magnitude (6 Pm + 3 Vm + Am / 2) / T^5.  (c3: 8 + 5 + 1 = 14, c4: 8 + 7 + 1
    = 16.)  That magnitude counts |a0| T^2 with weight 3 + 3 + 1/2 where |A^-1| |d| has 1/2, since the closed form's
    a0 terms cancel: a factor 13, the largest over the inputs and over c3..c5 (c3: 9.5 / 1.5, c4: 15.5 / 1.5; v0: at
    most 3; the others 1).  18 * 13 = 234 for a segment whose a0 term dominates everything else.

An implementation that adds its sums term by term in sequence (the oracle, which tests/test_post_twin.py holds to
the same bounds) has the number of terms where the kernel has the tree's six levels plus the passes: `serial=True`
in tests/post_bounds.py changes that summand of K and nothing else.

Largest |err| / (u * magnitude) seen against the exact twin (MI355X, the committed inputs; GTOP_POST_LOG=<file> appends
one JSON line per check): points 2.1 (K 16), length 0.59 (K 27 to 31), jerk 1.6 (K 24), acc cost 2.9 (K 16), max
velocity 1.8 and max acceleration 1.6 (K 12), mean velocity 4.4 and mean acceleration 3.8 (K 23 to 92 with the step
count), coefficients 4.6 (K 256: the factor 13 is the worst case of an a0-dominated segment, which these inputs are
not).  The oracle on the same inputs: points 1.7, length 2.9, jerk 10.7, acc cost 12.6, the means 25.9 (serial K 263).
Headroom of 4 to 40 is the price of bounds from the arithmetic; the mutants of tests/test_post_twin.py (each beyond
four times its bound, or an exact quantity changed) show what they still catch.

What each test is there for: the segment a sample is evaluated in (`<` for `<=`, an off-by-one in the walk, the last
segment at t == time_sum, k * dt for the accumulated time) — test_segment_probe; sample counts 64 k and 64 k +- 1, the
carried point, a chunk with lane 0 alone, the cap at a chunk boundary — test_chunk_edges; the second and later passes
of the per-segment loop — test_segment_counts; rows, shared times (time_stride = 0), a caller's stream —
test_batch_rows, test_shared_times; a dropped term or a wrong power in the closed form — test_coefficients_entrywise;
the second element of a lane in the grid-stride loops — test_grid_stride_setup, test_grid_stride_coefficients; the
argument checks of the entries — test_refusals.

The shapes are the smallest that reach the code in question; no test provokes a fault: every buffer is sized for what
the call may write, the refusals are argument checks made on the host."""
import ctypes as C

import numpy as np
import pytest

from tests import post_cases as cases
from tests import post_twin as twin
from tests.post_bounds import (K_COEF, log, compare_coefficients, hold_coefficients, hold_samples, hold_stats,
                               twin_of)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(gtop):
    c = gtop.GtopContext(device=0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def _run(ctx, coeff, T, dt, cap=None, stream=None):
    """One call of the sampling entry (cap given) or the statistics entry on host arrays: numpy (stats, samples)."""
    import torch
    c, t = _dev(np.asarray(coeff).reshape(-1, T.shape[-1], 18)), _dev(T)
    if cap is None:
        st, sm = ctx.eval_trajectories_device(c, t, dt, stream=stream), None
    else:
        st, sm = ctx.sample_trajectories_device(c, t, dt, max_samples=cap, stream=stream)
    torch.cuda.synchronize()
    return st.cpu().numpy(), None if sm is None else sm.cpu().numpy()


@pytest.mark.parametrize("family", cases.PROBES)
def test_segment_probe(ctx, family):
    """Which segment a sample is evaluated in and at which local time, read back exactly: `<` for `<=` in the walk, an
    off-by-one, k * dt for the accumulated time or a last segment that is not extended change x or y of a sample."""
    T, dt, coeff = cases.probe(family)
    smp, ref = twin_of(("probe", family), coeff, T, dt)
    cap = smp["n"] + 3
    stats, samples = _run(ctx, coeff, T, dt, cap)
    hold_samples(("probe", family), samples[0], smp, cap, probe=True)
    hold_stats(("probe", family), stats[0], ref)
    if family == "binary":   # the expectation by integer arithmetic, without the twin's replay
        edges = np.cumsum(cases.PROBE_BIN_STEPS)
        assert smp["n"] == edges[-1] + 1 == stats[0, 8]
        for k in range(smp["n"]):
            s = min(int(np.searchsorted(edges, k, side="right")), len(edges) - 1)   # on a boundary: the NEXT segment
            start = 0 if s == 0 else edges[s - 1]
            assert samples[0, k, 0] == s and samples[0, k, 1] == (k - start) * dt, (k, samples[0, k])
        assert samples[0, smp["n"] - 1, 0] == len(T) - 1 and samples[0, smp["n"] - 1, 1] == T[-1]   # t == time_sum
    if family == "short":
        assert min(ref[2]["counts"]) == 1 and len(set(smp["idx"])) < len(T)   # segments skipped by one step


@pytest.mark.parametrize("n", cases.CHUNK_COUNTS)
def test_chunk_edges(ctx, n):
    """Sample counts at and around the multiples of the 64 lanes, each with caps at and around the chunk boundary and
    the count: the carried point between chunks (the length), a chunk in which lane 0 alone is live (65, 129, 257),
    the cap cutting at a chunk boundary."""
    T, dt, coeff = cases.chunk_case(n)
    smp, ref = twin_of(("chunk", n), coeff, T, dt)
    assert smp["n"] == n
    stats0, _ = _run(ctx, coeff, T, dt)
    hold_stats(("chunk", n, "stats only"), stats0[0], ref)
    for cap in cases.chunk_caps(n):
        stats, samples = _run(ctx, coeff, T, dt, cap)
        assert stats[0, 8] == n                                  # the true count, also beyond the cap
        assert stats.tobytes() == stats0.tobytes(), (n, cap, "statistics differ with the sample output on")
        hold_samples(("chunk", n, cap), samples[0], smp, cap)


@pytest.mark.parametrize("m", cases.SEGMENT_COUNTS)
def test_segment_counts(ctx, m):
    """Every pass of the per-segment loop (64 segments each): all eight statistics with the largest velocity in
    segment 0, in the last segment, and in between: in segment 64, the first lane of the second pass (m > 65), in
    segment 63, the last lane of the first (m = 65; for m = 64 that is the last segment: two arrangements), in the
    middle of a trajectory of one pass (m <= 63; m = 1 has one arrangement).  The largest acceleration sits elsewhere."""
    for seg_v, seg_a in cases.arrangements(m):
        T, dt, coeff = cases.segment_case(m, seg_v, seg_a)
        smp, ref = twin_of(("segments", m, seg_v, seg_a), coeff, T, dt)
        assert ref[2]["arg_v"] == seg_v and ref[2]["arg_a"] == seg_a and smp["n"] < 400
        stats, _ = _run(ctx, coeff, T, dt)
        hold_stats(("segments", m, seg_v, seg_a), stats[0], ref)
        if seg_v == 0:   # the sampling entry on the same trajectory (m = 1: the walk never moves)
            cap = smp["n"] + 1
            stats_s, samples = _run(ctx, coeff, T, dt, cap)
            assert stats_s.tobytes() == stats.tobytes()
            hold_samples(("segments", m, "samples"), samples[0], smp, cap)


@pytest.mark.parametrize("B", cases.BATCHES)
def test_batch_rows(ctx, B):
    """Row b of a batch is the bits of the same row launched alone (1 025 rows: more blocks than any other test), on
    the caller's stream too.  Every row's decisions are compared with the twin's; the VALUES of rows 0, 1, 2 and every
    97th row are (the exact twin of all 1 025 rows would take half a minute) — the other rows are held to them through
    the bit-identity with their own solo launch, which runs the code the value checks of this module pin."""
    import torch
    T, dt, coeff = cases.batch_case(B)
    cap = 160
    stats, samples = _run(ctx, coeff, T, dt, cap)
    stats_e, _ = _run(ctx, coeff, T, dt)
    assert stats.tobytes() == stats_e.tobytes()
    c, t = _dev(coeff), _dev(T)
    alone_st = torch.empty(B, 9, dtype=torch.float64, device="cuda:0")
    alone_sm = torch.zeros(B, cap, 3, dtype=torch.float64, device="cuda:0")
    for b in range(B):
        ctx.sample_trajectories_device(c[b:b + 1], t[b:b + 1], dt, max_samples=cap, stats=alone_st[b:b + 1],
                                       samples=alone_sm[b:b + 1])
    torch.cuda.synchronize()
    assert alone_st.cpu().numpy().tobytes() == stats.tobytes()
    assert alone_sm.cpu().numpy().tobytes() == samples.tobytes()
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st_s, sm_s = ctx.sample_trajectories_device(c, t, dt, max_samples=cap, stream=side.cuda_stream)
        st_e = ctx.eval_trajectories_device(c, t, dt, stream=side.cuda_stream)
    side.synchronize()
    assert st_s.cpu().numpy().tobytes() == stats.tobytes() and st_e.cpu().numpy().tobytes() == stats.tobytes()
    assert sm_s.cpu().numpy().tobytes() == samples.tobytes()
    for b in range(B):                                           # decisions on every row
        assert stats[b, 0] == twin.time_sum(T[b]) and stats[b, 8] == len(twin.sample_times(T[b], dt)) <= cap
    for b in sorted(set(range(min(B, 3))) | set(range(0, B, 97))):   # values (rows 0, 7, 14, ... are long ones)
        smp, ref = twin_of(("batch", B, b), coeff[b], T[b], dt)
        hold_samples(("batch", B, b), samples[b], smp, cap)
        hold_stats(("batch", B, b), stats[b], ref)


@pytest.mark.parametrize("B", cases.BATCHES)
def test_shared_times(ctx, B):
    """time_stride = 0 (one T[m] for the batch) is the bits of the same times replicated per row: through the device
    entries, and through set_problem(T[m]) + trajectory_stats / trajectory_samples."""
    T, dt, coeff = cases.batch_case(B, shared_times=True)
    Trep = np.tile(T, (B, 1))
    cap = 96
    st0, sm0 = _run(ctx, coeff, T, dt, cap)
    st1, sm1 = _run(ctx, coeff, Trep, dt, cap)
    assert st0.tobytes() == st1.tobytes() and sm0.tobytes() == sm1.tobytes()
    assert _run(ctx, coeff, T, dt)[0].tobytes() == st0.tobytes()
    smp, ref = twin_of(("shared", B), coeff[0], T, dt)
    hold_samples(("shared", B), sm0[0], smp, cap)
    hold_stats(("shared", B), st0[0], ref)
    # the host entries: coefficients, statistics and samples of a problem with shared times
    rng = np.random.default_rng(B)
    Df = rng.normal(0.0, 1.0, (B, 18))
    x = rng.normal(0.0, 1.0, (B, 9 * (len(T) - 1)))
    out = []
    for times in (T, Trep):
        ctx.set_problem(times, Df)
        cf, st = ctx.trajectory_stats(x, dt_sample=dt)
        st2, sm = ctx.trajectory_samples(x, dt_sample=dt, max_samples=cap)
        assert st.tobytes() == st2.tobytes()
        out.append((cf, st, sm))
    for a, b in zip(out[0], out[1]):
        assert a.tobytes() == b.tobytes()
    cf, st, sm = out[0]
    dst, dsm = _run(ctx, cf, T, dt, cap)                         # ... and are what the device entries give
    assert dst.tobytes() == st.tobytes() and dsm.tobytes() == sm.tobytes()
    hold_coefficients(("shared", B, "host"), cf[B - 1], twin.coefficients(T, Df[B - 1], x[B - 1]))


@pytest.mark.parametrize("shared", [False, True], ids=["per-row-times", "shared-times"])
@pytest.mark.parametrize("m", cases.COEF_M)
def test_coefficients_entrywise(ctx, m, shared):
    """Every coefficient of every row against the rational solve of the Hermite system."""
    import torch
    T, Df, x = cases.coef_case(m, shared)
    coeff = ctx.coefficients_device(_dev(x), _dev(Df), _dev(T))
    torch.cuda.synchronize()
    coeff = coeff.cpu().numpy()
    for b in range(cases.COEF_B):
        hold_coefficients(("coefficients", m, shared, b), coeff[b], twin.coefficients(T if shared else T[b], Df[b], x[b]))


def test_grid_stride_setup(ctx):
    """286 300 outputs on 262 144 lanes: T, Df and x0 of all 700 rows, bit for bit."""
    import torch
    wp = cases.grid_setup_case()
    T, Df, x0 = ctx.setup_paths_device(_dev(wp), mean_v=1.8, init_time=0.3)
    torch.cuda.synchronize()
    T, Df, x0 = T.cpu().numpy(), Df.cpu().numpy(), x0.cpu().numpy()
    for b in range(cases.GRID_B):
        Df_ref, x0_ref = twin.initial_d(wp[b])
        assert T[b].tobytes() == twin.segment_time(wp[b], 1.8, 0.3).tobytes(), b
        assert Df[b].tobytes() == Df_ref.tobytes() and x0[b].tobytes() == x0_ref.tobytes(), b
    assert T[3, 0] > T[3, 1:].max() - 0.3 and T[0, 0] == twin.segment_time(wp[0], 1.8, 0.0)[0] + 0.3   # segment 0 alone


def test_grid_stride_coefficients(ctx):
    """273 000 (trajectory, segment, axis) elements on 262 144 lanes: the bits of the same rows launched in batches of
    one pass each, and the exact twin on every element of the second pass plus every 509th of the first (rational
    solves of all 273 000 would take minutes)."""
    import torch
    T, Df, x = cases.grid_coef_case()
    m, B = cases.GRID_COEF_M, cases.GRID_B
    xd, dfd, td = _dev(x), _dev(Df), _dev(T)
    coeff = ctx.coefficients_device(xd, dfd, td)
    half = B // 2
    assert half * m * 3 <= cases.LANES
    parts = [ctx.coefficients_device(xd[a:a + half], dfd[a:a + half], td) for a in (0, half)]
    torch.cuda.synchronize()
    coeff = coeff.cpu().numpy()
    assert coeff.tobytes() == torch.cat(parts).cpu().numpy().tobytes()
    qs = list(range(cases.LANES, B * m * 3)) + list(range(0, cases.LANES, 509))
    rows = {}
    for q in qs:
        b, r = divmod(q, 3 * m)
        rows.setdefault(b, []).append(divmod(r, 3))
    worst = 0.0
    for b, keys in rows.items():
        worst = max(worst, compare_coefficients(coeff[b], twin.coefficients(T, Df[b], x[b], only=keys)))
    log(dict(what="grid-stride coefficients", quantity="coefficient", ratio=worst, K=K_COEF))
    assert worst <= K_COEF, worst


def test_refusals(ctx):
    """Bad arguments are refused on the host: nothing is launched, the outputs keep what they held.  B = 0 is a no-op."""
    import torch
    L, h, vp = ctx._L, ctx._h, C.c_void_p
    m, B, cap = 3, 2, 8
    T, dt, coeff = cases.batch_case(3)
    c, t = _dev(coeff[:B]), _dev(T[:B])
    mark = 12345.0
    st = torch.full((B, 9), mark, dtype=torch.float64, device="cuda:0")
    sm = torch.full((B, cap, 3), mark, dtype=torch.float64, device="cuda:0")
    s = vp(torch.cuda.current_stream().cuda_stream)
    P = lambda x: vp(x.data_ptr())

    def sample(B_=B, m_=m, c_=P(c), t_=P(t), stride=m, dt_=dt, st_=P(st), sm_=P(sm), cap_=cap):
        return L.gtop_sample_trajectories_device(h, B_, m_, c_, t_, stride, dt_, st_, sm_, cap_, s)

    def stat(B_=B, m_=m, c_=P(c), t_=P(t), stride=m, dt_=dt, st_=P(st)):
        return L.gtop_eval_trajectories_device(h, B_, m_, c_, t_, stride, dt_, st_, s)

    for f in (sample, stat):
        for kw in (dict(B_=-1), dict(m_=0), dict(m_=-3), dict(stride=1), dict(stride=m + 1), dict(stride=-m), dict(dt_=0.0),
                   dict(dt_=-0.01), dict(dt_=float("nan")), dict(c_=None), dict(t_=None), dict(st_=None)):
            assert f(**kw) == 1, (f.__name__, kw)
        assert f(B_=0) == 0 and f(B_=0, c_=None, t_=None, st_=None) == 0
    assert sample(cap_=-1) == 1 and sample(sm_=None) == 1       # a cap with nowhere to store the points
    assert sample(sm_=None, cap_=0) == 0                         # cap 0: the statistics alone, as the other entry gives
    torch.cuda.synchronize()
    assert not bool((st == mark).any()) and bool((sm == mark).all())
    only_stats = st.clone()
    st.fill_(mark)
    assert stat() == 0
    torch.cuda.synchronize()
    assert torch.equal(st, only_stats)
    st.fill_(mark)
    # the coefficient entry
    Tc, Dfc, xc = cases.coef_case(2, False)
    xd, dfd, tcd = _dev(xc), _dev(Dfc), _dev(Tc)
    co = torch.full((cases.COEF_B, 2, 18), mark, dtype=torch.float64, device="cuda:0")

    def coef(B_=cases.COEF_B, m_=2, x_=P(xd), df_=P(dfd), t_=P(tcd), stride=2, co_=P(co)):
        return L.gtop_coefficients_device(h, B_, m_, x_, df_, t_, stride, co_, s)

    for kw in (dict(B_=-1), dict(m_=1), dict(m_=0), dict(stride=1), dict(stride=3), dict(x_=None), dict(df_=None),
               dict(t_=None), dict(co_=None)):
        assert coef(**kw) == 1, kw
    assert coef(B_=0) == 0
    # the set-up entry
    wp = _dev(cases.grid_setup_case()[:2, :4])
    outs = [torch.full((2, k), mark, dtype=torch.float64, device="cuda:0") for k in (3, 18, 18)]

    def setup(B_=2, m_=3, wp_=P(wp), v=1.8, T_=P(outs[0]), Df_=P(outs[1]), x0_=P(outs[2])):
        return L.gtop_setup_paths_device(h, B_, m_, wp_, v, 0.3, T_, Df_, x0_, s)

    for kw in (dict(B_=-1), dict(m_=1), dict(v=0.0), dict(v=-1.0), dict(wp_=None), dict(T_=None), dict(Df_=None),
               dict(x0_=None)):
        assert setup(**kw) == 1, kw
    assert setup(B_=0) == 0
    torch.cuda.synchronize()
    for out in [st, sm, co] + outs:
        assert bool((out == mark).all()), "a refused call wrote to its output"
    with pytest.raises(Exception):                               # and the wrapper reports the refusal
        ctx.eval_trajectories_device(c, t, dt_sample=0.0)
    assert sample() == 0 and stat() == 0 and coef() == 0 and setup() == 0   # the same arguments, unaltered, are served
    torch.cuda.synchronize()
    assert not bool((st == mark).any()) and not bool((co == mark).any()) and not bool((outs[0] == mark).any())
