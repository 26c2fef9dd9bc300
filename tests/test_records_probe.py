"""The probe of tests/records_probe.py can see what it claims to see (CPU only, the oracle).

Containment: every sample of row r has row r's base index — the row reads its cell's two records and nothing else.
Sensitivity: one wrong voxel in one of a row's clamped corners — the value of a face neighbour in its place, which is
what a record wired one row, one column or one level off holds — moves the row's cost or gradient by more than four
times the bound tests/test_gpu_records.py applies to that row.  With the fp64 bound that holds for every such error;
with the fp32 bound for at least 95 % of them per field seed (measured, oracle, grid (9, 7, 5), ws = 0, all 480 rows,
field seeds 0 .. 3: 1.000 and 0.962-0.973), which is why every fp32 check of test_gpu_records.py runs on two field
seeds: a wrongly wired record does not depend on the values stored in it."""
import numpy as np
import pytest

from tests import records_probe as rp
from tests.test_gpu_entrywise import KAPPA32, KAPPA64, U32, U64

SAMPLES_PER_SEGMENT = 200
ROWS = 240                # rows per field seed of the sensitivity test


@pytest.mark.parametrize("grid", rp.GRIDS, ids=[str(g) for g in rp.GRIDS])
@pytest.mark.parametrize("m", [2, 6])
def test_rows_stay_in_their_cell(oracle_mod, grid, m):
    origin, map_size = rp.geometry(grid)
    assert np.array_equal(np.ceil(map_size / rp.RES).astype(int), grid)
    cl = rp.cells(grid)
    assert len(cl) == (grid[0] + 1) * (grid[1] + 1) * (grid[2] + 1) and len(np.unique(cl, axis=0)) == len(cl)
    assert cl.min(axis=0).tolist() == [-1, -1, -1] and (cl.max(axis=0) == np.array(grid) - 1).all()
    T, Df, x = rp.probe_rows(grid, origin, rp.RES, m=m, seed=3)
    assert T.shape == (len(cl), m) and Df.shape == (len(cl), 3, 6) and x.shape == (len(cl), 9 * (m - 1))
    # (the rows share their segment times: one L serves them all)
    L = oracle_mod.generator(T[0])["L"]
    t = np.linspace(0.0, rp.SEG_T, SAMPLES_PER_SEGMENT)
    pw = t[:, None] ** np.arange(6)[None, :]                                  # (200, 6), ascending powers
    lo, hi = origin + 1e-4, origin + map_size - 1e-4
    for r in range(len(cl)):
        coe = oracle_mod.coefficients(T[r], Df[r], x[r], L=L).reshape(m, 3, 6)
        pos = np.einsum("tk,sak->sta", pw, coe).reshape(-1, 3)
        # the lookup's position is a float (grad_traj_optimizer.cpp:457-465): both must sit in the cell
        for p in (pos, pos.astype(np.float32).astype(np.float64)):
            assert (rp.base_index(p, origin, rp.RES) == cl[r]).all(), (grid, m, r, cl[r])
            assert (p >= lo).all() and (p <= hi).all(), (grid, m, r, cl[r], "leaves the map")


def test_repeated_cells_and_queries(oracle_mod):
    grid = (9, 7, 5)
    origin, map_size = rp.geometry(grid)
    cl = rp.cells(grid)
    T, Df, x = rp.probe_rows(grid, origin, rp.RES, m=6, seed=1, count=1024)
    assert len(x) == 1024
    wp = np.concatenate([Df[:, None, :, 0], x.reshape(1024, 3, 5, 3)[:, :, :, 0].transpose(0, 2, 1), Df[:, None, :, 3]], axis=1)
    assert (rp.base_index(wp, origin, rp.RES) == cl[np.arange(1024) % len(cl)][:, None, :]).all()
    assert not np.array_equal(wp[0], wp[len(cl)])                  # a repeated cell: waypoints of its own
    pos, pc = rp.probe_queries(grid, origin, rp.RES, per_cell=4, seed=2)
    assert pos.shape == (4 * len(cl), 3) and (rp.base_index(pos, origin, rp.RES) == pc).all()
    sdf = oracle_mod.Sdf(origin, rp.RES, grid, rp.probe_field(grid, 0).reshape(-1))
    for i in range(len(pos)):
        assert sdf.query(pos[i])[0] > 0, (i, pc[i])                # in the map: never -1


def _moves(base, mut, kappa, u):
    """Does the mutated row leave 4x the bound check() holds the base row to, in the cost or in a gradient entry?"""
    c0, g0, cm, gm, _, cf, gf = base
    c1, g1 = mut[0], mut[1]
    return bool(abs(c1 - c0) > 4 * (kappa * u * cm + cf) or (np.abs(g1 - g0) > 4 * (kappa * u * gm + gf)).any())


@pytest.mark.parametrize("field_seed", [0, 1])
def test_one_wrong_corner_moves_the_row(oracle_mod, field_seed):
    grid = (9, 7, 5)
    origin, _ = rp.geometry(grid)
    cl = rp.cells(grid)
    T, Df, x = rp.probe_rows(grid, origin, rp.RES, m=2, seed=0)
    rows = np.sort(np.random.default_rng(40 + field_seed).permutation(len(cl))[:ROWS])   # of the 480 cells, border cells among them
    assert len(rows) >= 150 and (cl[rows].min(axis=0) == -1).all() and (cl[rows].max(axis=0) == np.array(grid) - 1).all()
    sdf = oracle_mod.Sdf(origin, rp.RES, grid, rp.probe_field(grid, field_seed).reshape(-1))
    prm = oracle_mod.make_params(ws=0.0)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)       # noqa: E731
    hit = {"f64": 0, "f32": 0}
    total = 0
    for r in rows:
        ins = {"f64": (T[r], Df[r], x[r]), "f32": (f32(T[r]), f32(Df[r]), f32(x[r]))}
        base = {k: oracle_mod.cost_grad_mag(*v, sdf, prm) for k, v in ins.items()}
        for vox in rp.clamped_corners(grid, cl[r]):
            at = np.ravel_multi_index(vox, grid)
            keep = sdf.dist[at]
            for nb in rp.face_neighbours(grid, vox):
                sdf.dist[at] = sdf.dist[np.ravel_multi_index(nb, grid)]
                total += 1
                hit["f64"] += _moves(base["f64"], oracle_mod.cost_grad_mag(*ins["f64"], sdf, prm), KAPPA64, U64)
                hit["f32"] += _moves(base["f32"], oracle_mod.cost_grad_mag(*ins["f32"], sdf, prm), KAPPA32, U32)
                sdf.dist[at] = keep
    share64, share32 = hit["f64"] / total, hit["f32"] / total
    print(f"field seed {field_seed}: {total} single-voxel errors, seen with the fp64 bound {share64:.4f}, fp32 {share32:.4f}")
    assert share64 == 1.0, (field_seed, share64)
    assert share32 >= 0.95, (field_seed, share32)
