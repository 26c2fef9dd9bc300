"""The continuous-time certificate of pairwise separation on the device (include/gtop_separation_certificate.h;
csrc/gtop_separation_certificate.hip) through grad_traj_optimization_amd.separation_certificate.

(1) Device = twin (tests/sepcert_twin.py), bit for bit, for pairs and rows on the committed cases (sepcert_twin.CASES:
    tests/test_sepcert_twin.py holds each of them to deciding at max_depth = 2).
(2) A pair's row depends on neither B nor the rows' places.  (3) cull = 1 against cull = 0.  (4) Host form = device
form.  (5) One graph, the start times read at replay.  (6) Guard words, refusals, B = 0, NaN coefficients."""
import numpy as np
import pytest

from grad_traj_optimization_amd import separation_certificate as gc
from tests import sepcert_twin as ct

pytestmark = pytest.mark.gpu
bits, same_bits = ct.bits, ct.same_bits

ERR_INVALID, ERR_STATE = 1, 4
GUARD = -12345.0


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0", dtype=dtype)


@pytest.fixture(scope="module")
def ctx(gtop):
    c = gtop.GtopContext(device=0)       # no field: the certificate reads none
    yield c
    c.set_start_times(None)
    c.close()


def opts_of(kw):
    return gc.GtopSepCertOpts(**kw)


def run_device(ctx, coeff, T, kw, t0=None):
    """(pairs, rows) as host arrays, under start times t0 (None, a scalar, or one per row)."""
    import torch
    ctx.set_start_times(t0)
    try:
        out = gc.certify_separation_device(ctx, dev(coeff), dev(T), opts_of(kw))
        torch.cuda.synchronize()
    finally:
        ctx.set_start_times(None)
    return tuple(o.cpu().numpy() for o in out)


@pytest.mark.parametrize("case", range(len(ct.CASES)))
def test_device_equals_twin_bit_for_bit(ctx, case):
    coeff, T, t0, kw = ct.case_inputs(ct.CASES[case])
    B = coeff.shape[0]
    pairs, rows = run_device(ctx, coeff, T, kw, t0)
    want_pairs, want_rows, _ = ct.certify(coeff, T, t0, **kw)
    print(ct.CASES[case], "verdicts", {v: int(np.sum(pairs[..., 0] == v)) for v in (-1, 0, 1)}, "refined",
          pairs[..., 6].sum() / 2, "open", pairs[..., 5].sum() / 2, "boxed", int(np.sum(pairs[..., 7] == -1)) // 2)
    assert same_bits(pairs, want_pairs), np.argwhere(bits(pairs) != bits(want_pairs))[:5]
    assert same_bits(rows, want_rows), (rows[:3], want_rows[:3])
    # every pair is present and mirrored, the diagonal is the diagonal's row
    assert same_bits(pairs, pairs.transpose(1, 0, 2))
    assert all(same_bits(pairs[i, i], ct.DIAGONAL) for i in range(B))
    assert pairs.shape == (B, B, 8) and not np.any(np.isnan(pairs))


def test_every_breakpoint_inside_a_held_window(ctx):
    """2 m + 3 pieces: the last one, where both rows stand after their ends, is walked — there alone the rows of
    sepcert_twin.closing_rows() are at their least distance, 0.375 exactly."""
    c, T, t0 = ct.closing_rows()
    for min_sep, verdict in ((0.3, 1.0), (0.376, -1.0)):
        kw = dict(min_sep=min_sep, t_lo=0.0, t_hi=2.0, hold_ends=True)
        pairs, rows = run_device(ctx, c, T, kw, t0)
        want_pairs, want_rows, _ = ct.certify(c, T, t0, **kw)
        assert same_bits(pairs, want_pairs) and same_bits(rows, want_rows)
        r = pairs[0, 1]
        assert r[0] == verdict and r[7] == 7.0 and r[2] == 0.375 and r[3] == 0.75 + 1.25 / 128, r


def test_a_pair_depends_on_neither_the_batch_nor_its_place(ctx):
    coeff, T, t0, kw = ct.case_inputs(ct.CASES[-1])         # B = 67
    B = coeff.shape[0]
    pairs, rows = run_device(ctx, coeff, T, kw, t0)
    sub = [3, 64, 17, 66, 0]                                  # a subset, out of order
    spairs, _ = run_device(ctx, coeff[sub], T[sub], kw, t0[sub])
    assert same_bits(spairs, pairs[np.ix_(sub, sub)])
    perm = np.random.default_rng(9).permutation(B)
    ppairs, prows = run_device(ctx, coeff[perm], T[perm], kw, t0[perm])
    assert same_bits(ppairs, pairs[np.ix_(perm, perm)])
    assert same_bits(prows[:, [0, 1, 3, 5, 6, 7, 8, 9]], rows[perm][:, [0, 1, 3, 5, 6, 7, 8, 9]])
    # the index columns name the same rows: an index of the permuted batch goes back through the permutation; compared
    # where the least figure is attained by one pair only (on a tie the least j depends on the order)
    checked = 0
    for col, entry in ((2, 1), (4, 2)):
        for k in range(B):
            i = perm[k]
            if rows[i, col] >= 0 and np.count_nonzero(np.delete(pairs[i, :, entry], i) == rows[i, col - 1]) == 1:
                assert perm[int(prows[k, col])] == rows[i, col], (col, k)
                checked += 1
    assert checked > B
    again = run_device(ctx, coeff, T, kw, t0)
    assert same_bits(again[0], pairs) and same_bits(again[1], rows)


@pytest.mark.parametrize("case", [2, 5, 8])
def test_cull_against_no_cull(ctx, case):
    coeff, T, t0, kw = ct.case_inputs(ct.CASES[case])
    with_cull, _ = run_device(ctx, coeff, T, dict(kw, cull=True), t0)
    without, _ = run_device(ctx, coeff, T, dict(kw, cull=False), t0)
    culled = with_cull[..., 7] == -1.0
    assert same_bits(with_cull[~culled], without[~culled])
    assert not np.any(without[culled][:, 0] == -1.0) and np.all(with_cull[culled][:, 0] == 1.0)
    assert np.all(with_cull[culled][:, 1] >= kw["min_sep"] * ct.SHRINK)
    assert not np.any(without[..., 7] == -1.0)
    if case != 5:
        assert culled.any() and not culled.all()


def test_host_form_equals_device_form(gtop, ctx):
    import torch
    from grad_traj_optimization_amd import problem
    from tests import scenes
    B = 6
    rng = np.random.default_rng(71)
    wp = scenes.OPTI_NODE_PATH[None, :5] + rng.uniform(-0.6, 0.6, (B, 5, 3))
    T = problem.segment_times(wp)
    Df, Dp = problem.initial_derivatives(wp)
    x = Dp.reshape(B, -1) + rng.normal(0.0, 0.05, (B, Dp[0].size))
    t0 = rng.uniform(0.0, 1.0, B)
    kw = dict(min_sep=0.3, max_depth=2, max_refine=8, cull=True)
    coeff = ctx.coefficients_device(dev(x), dev(Df.reshape(B, 18)), dev(T))
    torch.cuda.synchronize()
    pairs, rows = run_device(ctx, coeff.cpu().numpy(), T, kw, t0)
    want_pairs, want_rows, _ = ct.certify(coeff.cpu().numpy(), T, t0, **kw)
    assert same_bits(pairs, want_pairs) and same_bits(rows, want_rows)
    assert np.any(pairs[..., 0] == -1.0)                       # the rows follow one path: they are close
    ctx.set_problem(T, Df)
    ctx.set_start_times(t0)
    try:
        hpairs, hrows = gc.certify_separation_batch(ctx, x, opts_of(kw))
    finally:
        ctx.set_start_times(None)
    fewer = gc.certify_separation_batch(ctx, x[:3], opts_of(kw))      # the problem's first rows, no start times
    assert same_bits(hpairs, pairs) and same_bits(hrows, rows)
    assert fewer[0].shape == (3, 3, 8) and fewer[1].shape == (3, 10)


def test_one_graph_reads_the_start_times_at_replay(ctx):
    import torch
    coeff, T, _, kw = ct.case_inputs(ct.CASES[5])            # B = 5, m = 7, held, cull
    B = coeff.shape[0]
    rng = np.random.default_rng(303)
    t0_a, t0_b = rng.uniform(0.0, 0.75, B), rng.uniform(0.0, 1.5, B)
    c, t, t0 = dev(coeff), dev(T), dev(t0_a)
    f64 = dict(dtype=torch.float64, device=c.device)
    pairs, rows = torch.zeros(B, B, 8, **f64), torch.zeros(B, 10, **f64)
    work = torch.zeros(gc.sepcert_workspace_bytes(B), dtype=torch.uint8, device=c.device)
    opts = opts_of(kw)
    ctx.set_start_times_device(t0)

    def call():
        gc.certify_separation_device(ctx, c, t, opts, pairs, rows, work=work)

    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # warm-up outside the capture
            call()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        want_a = ct.certify(coeff, T, t0_a, **kw)
        assert same_bits(pairs.cpu().numpy(), want_a[0]) and same_bits(rows.cpu().numpy(), want_a[1])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        pairs.zero_()
        rows.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(pairs.cpu().numpy(), want_a[0]) and same_bits(rows.cpu().numpy(), want_a[1])
        t0.copy_(dev(t0_b))             # the buffer rewritten in place: the replay gives the new result
        graph.replay()
        torch.cuda.synchronize()
        want_b = ct.certify(coeff, T, t0_b, **kw)
        assert same_bits(pairs.cpu().numpy(), want_b[0]) and same_bits(rows.cpu().numpy(), want_b[1])
        assert not same_bits(want_a[0], want_b[0])
    finally:
        ctx.set_start_times_device(None)


def test_guard_words_around_every_output_and_the_workspace(ctx):
    import torch
    coeff, T, t0, kw = ct.case_inputs(ct.CASES[-1])         # B = 67, cull: the workspace is written
    B = coeff.shape[0]
    f64 = dict(dtype=torch.float64, device="cuda:0")
    pbuf = torch.full((B * B * 8 + 16,), GUARD, **f64)
    rbuf = torch.full((B * 10 + 16,), GUARD, **f64)
    need = gc.sepcert_workspace_bytes(B)
    wbuf = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ctx.set_start_times(t0)
    try:
        gc.certify_separation_device(ctx, dev(coeff), dev(T), opts_of(kw), pbuf[8:-8].reshape(B, B, 8),
                                     rbuf[8:-8].reshape(B, 10), work=wbuf[128:128 + need])
        torch.cuda.synchronize()
    finally:
        ctx.set_start_times(None)
    for buf in (pbuf, rbuf):
        assert torch.all(buf[:8] == GUARD) and torch.all(buf[-8:] == GUARD) and not torch.any(buf[8:-8] == GUARD)
    assert torch.all(wbuf[:128] == 0xA5) and torch.all(wbuf[128 + need:] == 0xA5)
    want_pairs, want_rows, _ = ct.certify(coeff, T, t0, **kw)
    assert same_bits(pbuf[8:-8].cpu().numpy().reshape(B, B, 8), want_pairs)
    assert same_bits(rbuf[8:-8].cpu().numpy().reshape(B, 10), want_rows)


def test_refusals_launch_nothing(gtop, ctx):
    import torch
    B, m = 3, 3
    coeff, T, _, _ = ct.case_inputs((B, m, 5, False, "none", False, False, 2, 4))
    c, t = dev(coeff), dev(T)
    f64 = dict(dtype=torch.float64, device=c.device)
    pairs, rows = torch.full((B, B, 8), GUARD, **f64), torch.full((B, 10), GUARD, **f64)
    need = gc.sepcert_workspace_bytes(B)
    work = torch.full((need,), 0xA5, dtype=torch.uint8, device=c.device)
    L, h = gc.sepcert_library(), ctx._h
    base = dict(min_sep=0.5, t_lo=0.0, t_hi=2.0, max_depth=2, max_refine=4)
    o = lambda **kw: gc.GtopSepCertOpts(**{**base, **kw})
    good = o()

    def refused(code, fn):
        with pytest.raises(gtop.GtopError) as ei:
            fn()
        assert ei.value.code == code, ei.value

    bad_opts = [o(min_sep=0.0), o(min_sep=-1.0), o(min_sep=np.nan), o(min_sep=np.inf), o(t_lo=np.nan), o(t_hi=np.nan),
                o(t_lo=2.5), o(t_lo=-np.inf, hold_ends=True), o(t_hi=np.inf, hold_ends=True), o(max_depth=-1),
                o(max_depth=4), o(max_refine=-1), o(reserved=(1, 0)), o(reserved=(0, 1))]
    for field in ("hold_ends", "cull"):
        for v in (2, -1):
            b = o()
            setattr(b, field, v)
            bad_opts.append(b)
    for bad in bad_opts:
        refused(ERR_INVALID, lambda: gc.certify_separation_device(ctx, c, t, bad, pairs, rows, work=work))
    vp = lambda a: a.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (
        ("B", B), ("m", m), ("coeff", vp(c)), ("T", vp(t)), ("stride", m), ("opt", good), ("pairs", vp(pairs)),
        ("rows", vp(rows)), ("work", vp(work)), ("bytes", need), ("stream", None))]
    for kw in (dict(opt=None), dict(B=-1), dict(B=2049), dict(m=1), dict(m=228), dict(stride=1), dict(stride=m + 1),
               dict(coeff=None), dict(T=None), dict(pairs=None), dict(rows=None), dict(work=None),
               dict(bytes=need - 1), dict(bytes=0)):
        assert L.gtop_certify_separation_device(h, *args(**kw)) == ERR_INVALID, kw
    assert L.gtop_certify_separation_device(None, *args()) == ERR_INVALID
    # a start-time count that is not 0, 1 or B
    ctx.set_start_times([0.0, 1.0])
    try:
        refused(ERR_INVALID, lambda: gc.certify_separation_device(ctx, c, t, good, pairs, rows, work=work))
    finally:
        ctx.set_start_times(None)
    # the host form: no problem, then too many rows, bad options, missing buffers
    x = np.zeros((B, 9 * (m - 1)))
    bare = gtop.GtopContext(device=0)
    try:
        refused(ERR_STATE, lambda: gc.certify_separation_batch(bare, x, good))
    finally:
        bare.close()
    ctx.set_problem(np.asarray(T), np.zeros((B, 3, 6)))
    refused(ERR_INVALID, lambda: gc.certify_separation_batch(ctx, np.tile(x, (2, 1)), good))
    refused(ERR_INVALID, lambda: gc.certify_separation_batch(ctx, x, bad_opts[0]))
    dp = lambda a: a.ctypes.data_as(gc._dp)
    hp, hr = np.full((B, B, 8), GUARD), np.full((B, 10), GUARD)
    assert L.gtop_certify_separation_batch(h, 0, dp(x), good, dp(hp), dp(hr)) == ERR_INVALID
    assert L.gtop_certify_separation_batch(h, B, None, good, dp(hp), dp(hr)) == ERR_INVALID
    assert L.gtop_certify_separation_batch(h, B, dp(x), None, dp(hp), dp(hr)) == ERR_INVALID
    assert L.gtop_certify_separation_batch(h, B, dp(x), good, None, dp(hr)) == ERR_INVALID
    assert L.gtop_certify_separation_batch(h, B, dp(x), good, dp(hp), None) == ERR_INVALID
    assert np.all(hp == GUARD) and np.all(hr == GUARD)
    torch.cuda.synchronize()
    assert torch.all(pairs == GUARD) and torch.all(rows == GUARD) and torch.all(work == 0xA5)
    # an infinite window without hold_ends is the default, not a refusal
    got = gc.certify_separation_device(ctx, c, t, o(t_lo=-np.inf, t_hi=np.inf))
    torch.cuda.synchronize()
    assert got[0].shape == (B, B, 8)


def test_an_empty_batch_and_a_single_row(ctx):
    import torch
    e = torch.empty(0, dtype=torch.float64, device="cuda:0")
    p0, r0 = gc.certify_separation_device(ctx, e.reshape(0, 3, 18), e.reshape(0, 3), gc.GtopSepCertOpts())
    assert p0.shape == (0, 0, 8) and r0.shape == (0, 10)
    assert gc.sepcert_library().gtop_certify_separation_device(ctx._h, 0, 3, None, None, 3, gc.GtopSepCertOpts(), None,
                                                               None, None, 0, None) == 0
    coeff, T, _, kw = ct.case_inputs((1, 2, 3, False, "none", False, True, 2, 4))
    pairs, rows = run_device(ctx, coeff, T, kw)
    assert same_bits(pairs[0, 0], ct.DIAGONAL) and rows[0].tolist() == [1, np.inf, -1, np.inf, -1, -1, -1, 0, 0, 0]


@pytest.mark.parametrize("cull", [False, True])
def test_nan_coefficients_certify_nothing(ctx, cull):
    """The call stays bounded, and a pair that touches the NaN row is never SAFE."""
    coeff, T, t0, kw = ct.case_inputs(ct.CASES[3])          # B = 5, held
    coeff = coeff.copy()
    coeff[2, :, 3] = np.nan                                   # row 2: a NaN coefficient in every segment
    pairs, rows = run_device(ctx, coeff, T, dict(kw, cull=cull, max_depth=3, max_refine=4), t0)
    touched = np.delete(pairs[2], 2, axis=0)
    assert not np.any(touched[:, 0] == 1.0) and rows[2, 0] != 1.0
    assert np.all(touched[:, 6] <= 4) and np.all(touched[:, 1] == -np.inf)
    clean = [0, 1, 3, 4]
    want, _, _ = ct.certify(coeff[clean], T if T.ndim == 1 else T[clean], t0[clean], **dict(kw, cull=cull, max_depth=3,
                                                                                              max_refine=4))
    assert same_bits(pairs[np.ix_(clean, clean)], want)
