"""The lone-wavefront fp64 bodies of gtop_eval_wave_kernel (csrc/gtop_wave_kernel.h: ten lanes per segment on the
two-wavefront register budget, one wavefront per trajectory up to 6 segments and two from 7) after their prologue was
reordered: the group arithmetic and the rows' byte strides come from the launcher (launch_wave, csrc/gtop_kernels.hip),
the waypoint addresses are formed another way, and the free-variable offsets, every remaining kernel argument and the
launch constants' product are held in front of the first wait for the inputs.  None of that touches an arithmetic
expression, so every output bit must be what it was.

Shapes: m = 2 (both ends of both segments' neighbours come from Df), 3 (one shared waypoint), 6 (a full wavefront);
B = 1 (a lone group, seven padding workgroups), 7 and 9 (the padding groups of the 8-way XCD split on either side of
8); T shared by the rows (stride 0) and per row (stride m); row 0 has a segment of T = 0.02 s (the replay of `t += dt`,
20 samples) and row 1 — row 0 when there is only one — leaves the map (the rare out-of-map branch).  m = 7 at B = 1 and
9 is the two-wavefront sibling.

What the results are held to:
  * up to 6 segments — bit for bit (array_equal) the same rows through a body this change leaves as it was: tiled into a
    3 072-row batch they go to the three-wavefront-budget body (one sample at a time, compiler-issued loads, no held
    prologue), the identity tests/test_gpu_wave.py::test_rows_do_not_depend_on_their_place holds between the two;
  * 7 segments — no other body adds a row's terms in the same order (five lanes per segment sum six samples per lane),
    so the rows are compared bit for bit with themselves inside a 1 024-row batch of the same body (another grid, other
    groups per XCD, no padding), which the launcher's new arguments must not disturb;
  * every case — the oracle, entry by entry, at the bound of tests/test_gpu_entrywise.py (its check(): KAPPA64 = 2^12
    unit roundoffs of the oracle's own error magnitudes)."""
import numpy as np
import pytest

from grad_traj_optimization_amd import problem
from tests import test_gpu_entrywise as ew

pytestmark = pytest.mark.gpu

TILED_ROWS = 3072    # csrc/gtop_kernels.hip kWaveMinw3From: from here ten lanes per segment run on the three-wavefront budget
NW2_ROWS = 1024      # the two-wavefront body's largest batch under the launch rule


@pytest.fixture(scope="module")
def scene(gtop, oracle_mod):
    mp = problem.make_map((60, 50, 30), density=0.03, seed=11)
    ctx = gtop.GtopContext(device=0)
    ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
    ctx.update_sdf_map(mp.obstacle_points())
    sdf = oracle_mod.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
    sdf.build_from_occupancy(mp.occupancy)
    yield mp, ctx, sdf
    ctx.close()


def _rows(mp, m, B, shared_T):
    """B rows of m segments; row 0 with a 0.02 s segment, row min(1, B - 1) leaving the map."""
    b = problem.make_trajectories(9, m, mp, seed=4100 + m, step_len=(0.5, 1.2) if m > 6 else (1.0, 2.0), boundary="random")
    x, T, Df, wp = b.x[:B].copy(), b.T[:B].copy(), b.Df[:B].copy(), b.waypoints[:B]
    if shared_T:
        T = T[0].copy()
        T[m - 1] = 0.02                   # (every row replays: the times are the rows' common ones)
    else:
        T[0, m - 1] = 0.02
    x[min(1, B - 1), 0] += 40.0           # first interior waypoint, x position: tens of metres outside the map
    return problem.Batch(wp, T, Df, x, m)


def _tile(b, rows):
    k = -(-rows // len(b.x))
    T = b.T if b.T.ndim == 1 else np.tile(b.T, (k, 1))[:rows]
    return problem.Batch(np.tile(b.waypoints, (k, 1, 1))[:rows], T, np.tile(b.Df, (k, 1, 1))[:rows],
                         np.tile(b.x, (k, 1))[:rows], b.m)


def _oracle(oracle_mod, b, sdf):
    T = b.T if b.T.ndim == 2 else np.tile(b.T, (len(b.x), 1))
    return ew._ref(oracle_mod, problem.Batch(b.waypoints, T, b.Df, b.x, b.m), sdf, {})


@pytest.mark.parametrize("shared_T", [True, False], ids=["stride0", "stride-m"])
@pytest.mark.parametrize("B", [1, 7, 9])
@pytest.mark.parametrize("m", [2, 3, 6])
def test_lone_wavefront_equals_three_wavefront_body(scene, oracle_mod, m, B, shared_T):
    mp, ctx, sdf = scene
    b = _rows(mp, m, B, shared_T)
    c, g = ew._device(ctx, b, "f64", 0, 3, {})                       # below 3 072 rows: the lone-wavefront body
    ct, gt = ew._device(ctx, _tile(b, TILED_ROWS), "f64", 0, 3, {})  # the same rows on the three-wavefront budget
    k = -(-TILED_ROWS // B)
    assert np.array_equal(ct, np.tile(c, k)[:TILED_ROWS]), "cost bits differ from the three-wavefront body's"
    assert np.array_equal(gt, np.tile(g, (k, 1))[:TILED_ROWS]), "gradient bits differ from the three-wavefront body's"
    assert np.isfinite(c).all() and np.isfinite(g).all()
    ew.check(c, g, _oracle(oracle_mod, b, sdf), "f64", ("lone wavefront", m, B, "stride 0" if shared_T else "stride m"))


@pytest.mark.parametrize("shared_T", [True, False], ids=["stride0", "stride-m"])
@pytest.mark.parametrize("B", [1, 9])
def test_two_wavefront_sibling(scene, oracle_mod, B, shared_T):
    mp, ctx, sdf = scene
    m = 7
    b = _rows(mp, m, B, shared_T)
    c, g = ew._device(ctx, b, "f64", 0, 0, {})                       # the launch rule: two wavefronts per trajectory
    ct, gt = ew._device(ctx, _tile(b, NW2_ROWS), "f64", 0, 0, {})
    k = -(-NW2_ROWS // B)
    assert np.array_equal(ct, np.tile(c, k)[:NW2_ROWS]) and np.array_equal(gt, np.tile(g, (k, 1))[:NW2_ROWS])
    assert np.isfinite(c).all() and np.isfinite(g).all()
    ew.check(c, g, _oracle(oracle_mod, b, sdf), "f64", ("two wavefronts", m, B, "stride 0" if shared_T else "stride m"))
