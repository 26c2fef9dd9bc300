"""The numpy restatement of the continuous-time clearance certificate (tests/certify_twin.py), checked without a GPU:

(1) the symbols, their bindings and the library's ABI version;
(2) soundness on the shared cases, four kinds of field: lo is at most the least of 20001 evenly spaced lookups along
    the curve, no exceptions; lo <= hi; SAFE => lo > margin; UNSAFE => hi <= margin; and no decision of a case lies
    within 1e-9 (relative) of a tie, so the device can be held to the same decisions;
(3) the claim the bound rests on: over a sub-box of a cell the trilinear form's minimum is at a vertex (a brute-force
    9^3 grid finds nothing lower), and a box's lb is below every lookup inside the box, also across cells;
(4) five mutants of the restatement, each caught by one of these checks."""
import numpy as np
import pytest

from tests import certify_twin as ct

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def fields(oracle_mod):
    return {kind: ct.make_field(oracle_mod, kind) for kind in ct.FIELDS}


@pytest.fixture(scope="module")
def runs(oracle_mod, fields):
    """name -> (field, coeff, T, margin, depth, refine, [(cert, info)] per row), computed once."""
    out = {}
    for name, (kind, m, B, seed, margin, depth, refine) in ct.CASES.items():
        field, mp = fields[kind]
        coeff, T, _ = ct.make_rows(oracle_mod, mp, B, m, seed)
        out[name] = (field, coeff, T, margin, depth, refine,
                     [ct.certify(field, coeff[i], T[i], margin, depth, refine) for i in range(B)])
    return out


def test_symbols_bindings_and_abi_version_exist(gtop):
    from grad_traj_optimization_amd import _abi, certify
    lib = gtop.load_library()
    assert lib.gtop_abi_version() >= 10 and _abi.ABI_VERSION >= 10
    for name in ("gtop_certify_trajectories_device", "gtop_certify_batch", "gtop_select_best_certified_device"):
        assert _abi.ENTRY_POINTS[name][0] == 10 and getattr(lib, name).argtypes is not None, name
    for name in ("certify_device", "select_best_certified_device", "certify_batch", "GtopCertifyOpts", "CERT_REPORT"):
        assert hasattr(certify, name) and hasattr(gtop, name), name
    assert len(certify.CERT_REPORT) == ct.N_CERT


@pytest.mark.parametrize("name", list(ct.CASES))
def test_lo_is_below_every_dense_lookup(runs, name):
    field, coeff, T, margin, depth, refine, rows = runs[name]
    for i, (cert, info) in enumerate(rows):
        dense, _ = ct.dense_clearance(field, coeff[i], T[i], 20001)
        print(f"{name}[{i}] verdict {cert[0]:+.0f} lo {cert[1]:.6g} dense {dense:.6g} hi {cert[2]:.6g} "
              f"undecided {cert[5]:.0f} refinements {cert[6]:.0f} tie {info['tie']:.3g}")
        assert cert[1] <= dense, (i, cert, dense)
        assert cert[1] <= cert[2], (i, cert)
        assert cert[0] != 1 or cert[1] > margin, (i, cert)
        assert cert[0] != -1 or cert[2] <= margin, (i, cert)
        assert cert[6] <= refine and cert[7] == np.add.reduce(T[i]), (i, cert)
        assert info["tie"] > 1e-9, (i, info["tie"])


def test_the_cases_cover_every_verdict_and_spend_refinements(runs):
    certs = np.array([c for run in runs.values() for c, _ in run[6]])
    assert {-1.0, 0.0, 1.0} <= set(certs[:, 0])
    assert (certs[:, 6] > 0).sum() >= 3 and (certs[:, 5] > 0).any()
    assert ((certs[:, 0] == 1) & (certs[:, 6] > 0)).any()      # a row that is SAFE only through refinement


def leaves_are_sound(field, coeff, leaves, samples=65):
    """Every leaf's lb is at most the lookups at `samples` points of its interval."""
    for s, a, w, lb, _ in leaves:
        t = a + np.linspace(0.0, 1.0, samples) * w
        pts = np.stack([ct.poly_eval(np.asarray(coeff).reshape(-1, 3, 6)[s, k], t) for k in range(3)], axis=1)
        if not lb <= field.midpoint_distance(pts).min():
            return False
    return True


def test_leaves_are_sound_interval_by_interval(runs):
    rng = np.random.default_rng(3)
    for name, (field, coeff, T, margin, depth, refine, rows) in runs.items():
        cert, info = rows[0]
        pick = rng.choice(len(info["leaves"]), 24, replace=False)
        assert leaves_are_sound(field, coeff[0], [info["leaves"][j] for j in pick]), name


def random_boxes(field, rng, n, straddle):
    """Boxes inside the map: within one cell, or (straddle) across up to two cells per axis."""
    lo_cell = rng.integers(1, field.n - 3, (n, 3))
    c0 = (lo_cell + 0.5) * field.res + field.origin
    if straddle:
        a = rng.uniform(0.3, 1.0, (n, 3))
        b = a + rng.uniform(0.05, 0.9, (n, 3))
    else:
        a = rng.uniform(0.0, 0.6, (n, 3))
        b = a + rng.uniform(0.0, 0.39, (n, 3))
    return c0 + a * field.res, c0 + b * field.res


def boxes_are_sound(field, mutant, straddle, n=12, seed=4):
    rng = np.random.default_rng(seed)
    blo, bhi = random_boxes(field, rng, n, straddle)
    g = np.linspace(0.0, 1.0, 9)
    w = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    for i in range(n):
        brute = field.midpoint_distance(blo[i] + w * (bhi[i] - blo[i])).min()
        lb = ct.box_lower_bound(field, blo[i], bhi[i], mutant, 0.5 * (blo[i] + bhi[i]))
        if not (np.isfinite(lb) and lb <= brute):
            return False
    return True


def test_the_minimum_over_a_sub_box_is_at_a_vertex(fields):
    """Random sub-boxes of random cells of the random field: the least of the form over a 9^3 grid of the sub-box (which
    holds the 8 vertices) is the least over the vertices, to the rounding of the form."""
    field, _ = fields["random"]
    rng = np.random.default_rng(8)
    g = np.linspace(0.0, 1.0, 9)
    w = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    for _ in range(40):
        v = field.corners(rng.integers(0, field.n - 1))
        a = rng.uniform(0.0, 1.0, 3)
        b = a + rng.uniform(0.0, 1.0, 3) * (1.0 - a)
        u = a + w * (b - a)
        grid_min = min(ct.trilinear(p, v) for p in u)
        vertex_min = min(ct.trilinear([(a, b)[e >> 2][0], (a, b)[(e >> 1) & 1][1], (a, b)[e & 1][2]], v) for e in range(8))
        assert abs(grid_min - vertex_min) <= 16 * EPS * np.abs(v).max(), (grid_min, vertex_min)
    for kind in ct.FIELDS:        # and the lookup itself stays above a box's lb, inside one cell and across cells
        assert boxes_are_sound(fields[kind][0], None, False) and boxes_are_sound(fields[kind][0], None, True), kind


def apex_case(oracle_mod):
    """A row that turns round in front of the wall of ct.wall_case: x(t) = -0.5 + 40 (t - t*)^2, t* the midpoint of
    interval 32 of the first segment, y and z constant.  Over that interval the velocity at the midpoint is zero and the
    curve still moves 4 mm towards the wall: only the acceleration term of the radius covers it."""
    field = ct.wall_case(oracle_mod)[0]
    T = np.array([1.28, 1.28])
    ts = 32.5 * T[0] / 64
    coeff = np.zeros((2, 3, 6))
    coeff[0, 0, :3] = (-0.5 + 40.0 * ts * ts, -80.0 * ts, 40.0)
    x1 = ct.poly_eval(coeff[0, 0], T[0])
    coeff[1, 0, :2] = (x1, 0.0)
    coeff[:, 1, 0], coeff[:, 2, 0] = 0.13, 1.57
    return field, coeff.reshape(2, 18), T


def test_every_mutant_is_caught(oracle_mod, fields, runs):
    # the radius without the acceleration term: a leaf's bound misses the curve where it turns round
    field, coeff, T = apex_case(oracle_mod)
    for mutant, sound in ((None, True), ("no_A", False)):
        _, info = ct.certify(field, coeff, T, 0.1, 0, 0, mutant)
        apex = [leaf for leaf in info["leaves"] if leaf[0] == 0 and np.isfinite(leaf[3])]
        assert apex and leaves_are_sound(field, coeff, apex, 257) == sound, mutant
    # only the midpoint's cell; floor in place of the clamped local coordinates: boxes across cells
    rnd = fields["random"][0]
    for mutant in ("mid_cell", "floor"):
        assert not boxes_are_sound(rnd, mutant, True), mutant
    # < for <= at the margin: a margin that IS a midpoint's distance (level 0 alone, so that no child looks closer)
    field, coeff, T, margin, depth, refine, rows = runs["esdf_m3"]
    base, _ = ct.certify(field, coeff[1], T[1], -2.0, 0, 0)
    hi, hi_t = base[2], base[3]
    assert base[0] == 1 and hi > 0
    exact, _ = ct.certify(field, coeff[1], T[1], hi, 0, 0)
    assert exact[0] == -1 and exact[4] == hi_t and exact[2] == hi
    mutant, _ = ct.certify(field, coeff[1], T[1], hi, 0, 0, "lt")
    assert mutant[0] != -1 and mutant[4] == -1
    # the budget: more OPEN intervals than refinements allowed
    field, coeff, T, margin, depth, refine, rows = runs["random_m2"]
    kept, _ = ct.certify(field, coeff[1], T[1], margin, 1, 3)
    assert kept[6] == 3 and kept[5] > 0
    spent, _ = ct.certify(field, coeff[1], T[1], margin, 1, 3, "budget")
    assert spent[6] > 3
