"""The bound kinds the device optimizer is tested on (tests/test_bound_cases.py on the CPU, tests/test_gpu_optimizer_bounds.py
on the device): one builder, no GPU, no pytest.

Every row starts from GtopContext.default_bounds of its own trajectory (finite, symmetric about the waypoint, the start
strictly inside) and changes it into one of the kinds below.  Position entries of a row of n = 9 (m - 1) variables are
(j % (n / 3)) % 3 == 0 (tests/test_optimizer.py::test_default_bounds); the others are velocities and accelerations.

Row order is part of the case: with two trajectories per wavefront rows 2k and 2k + 1 share a wavefront — `all-fixed`
(which stops after two evaluations under a tolerance and never moves) sits beside a running row, every row with an
infinite bound beside a finite one — and the batch is odd, so the last wavefront holds one trajectory."""
import numpy as np

from grad_traj_optimization_amd import problem

SCENE = dict(grid=(60, 50, 30), density=0.03, seed=11)      # the scene of tests/test_optimizer.py

# (in pairs: rows 2k and 2k + 1 share a wavefront at two trajectories per wavefront)
KINDS = ("default", "free",
         "all-fixed", "lower-only",
         "upper-only", "tight",
         "derivatives-free", "positions-fixed",
         "every-fourth-fixed", "start-outside",
         "start-on-faces", "wide",
         "free")                                            # a second `free` row, alone in the last wavefront
LONG_KINDS = ("free", "all-fixed", "start-outside")         # the rows of the long problems (65 and 118 segments)

# the seed of every committed case: chosen so that tests/test_bound_cases.py holds (no decision of the serial road
# within 1e-6 of a tie, no vanishing step, and the set not vacuous)
SEEDS = {2: 4302, 6: 4206, 7: 4907, 9: 5709, 12: 6112, 13: 6613, 65: 4165, 118: 4218}


# (m, samples_per_lane pinned through set_launch_geometry(0, pin), the body the optimizer's launch rule then runs — as
# tests/golden/launch_rule.txt has it, asserted in tests/test_bound_cases.py — and its (spl, nt, long) there)
GEOMETRIES = ((2, 0, "ten-lanes", (3, 1, 0)),
              (6, 3, "ten-lanes", (3, 1, 0)),
              (6, 6, "two-per-wavefront", (6, 2, 0)),
              (7, 0, "five-lanes", (6, 1, 0)),
              (12, 0, "five-lanes", (6, 1, 0)),
              (13, 0, "chunked", (6, 1, 1)),
              (65, 0, "chunked", (6, 1, 1)),
              (118, 0, "chunked", (6, 1, 1)))
F32_GEOMETRIES = ((6, 0, "ten-lanes", (3, 1, 0)), (9, 0, "five-lanes", (6, 1, 0)))      # fp32 evaluations (elem=4)
SERIAL_M = (2, 6, 7, 12, 13, 65, 118)                      # the segment counts compared with the serial algorithm


def evals_for(m):
    """The evaluation cap of every run on m segments."""
    return 25 if m <= 13 else 12


def rules_for(m):
    """The stop rules run on m segments, by name: the cap alone; up to 13 segments also ftol_rel, xtol_rel and both,
    loose enough that at least a third of the rows stop before the cap (asserted on both sides)."""
    if m > 13:
        return {"cap": {}}
    return {"cap": {}, "ftol": dict(ftol_rel=FTOL_REL), "xtol": dict(xtol_rel=XTOL_REL),
            "both": dict(ftol_rel=FTOL_REL, xtol_rel=XTOL_REL)}


FTOL_REL, XTOL_REL = 0.3, 1.5


def scene_map():
    return problem.make_map(SCENE["grid"], density=SCENE["density"], seed=SCENE["seed"])


def position_mask(n):
    """True at the position entries of a row of n free variables."""
    j = np.arange(n)
    return (j % (n // 3)) % 3 == 0


def fixed_mask(kind, n):
    """The entries `kind` fixes (lb == ub == x0)."""
    if kind == "all-fixed":
        return np.ones(n, dtype=bool)
    if kind == "positions-fixed":
        return position_mask(n)
    if kind == "every-fourth-fixed":
        return np.arange(n) % 4 == 0
    return np.zeros(n, dtype=bool)


def apply_kind(kind, x0, lb, ub):
    """One row: (x0, lb, ub) of `kind` from the row's start point and default bounds (new arrays)."""
    x0, lb, ub = x0.copy(), lb.copy(), ub.copy()
    n = x0.size
    pos = position_mask(n)
    if kind == "default":
        pass
    elif kind == "free":
        lb[:], ub[:] = -np.inf, np.inf
    elif kind == "lower-only":
        ub[:] = np.inf
    elif kind == "upper-only":
        lb[:] = -np.inf
    elif kind == "derivatives-free":
        lb[~pos], ub[~pos] = -np.inf, np.inf
    elif kind in ("positions-fixed", "every-fourth-fixed", "all-fixed"):
        fix = fixed_mask(kind, n)
        lb[fix] = x0[fix]
        ub[fix] = x0[fix]
    elif kind == "start-outside":
        even = np.arange(n) % 2 == 0
        x0[even] = ub[even] + 5.0
        x0[~even] = lb[~even] - 5.0
    elif kind == "start-on-faces":
        lb[pos] = x0[pos]
        ub[~pos] = x0[~pos]
    elif kind == "tight":
        lb, ub = x0 - 1e-3, x0 + 1e-3
    elif kind == "wide":
        lb, ub = x0 - 1e3, x0 + 1e3
    else:
        raise ValueError(kind)
    return x0, lb, ub


def build(m, seed=None, kinds=None):
    """(T, Df, x0, lb, ub, kinds) for trajectories of m segments on the scene above: one row per entry of `kinds`
    (default: KINDS up to 13 segments, LONG_KINDS beyond), row i a trajectory of its own."""
    import grad_traj_optimization_amd as gtop
    if kinds is None:
        kinds = KINDS if m <= 13 else LONG_KINDS
    if seed is None:
        seed = SEEDS[m]
    kinds = list(kinds)
    b = problem.make_trajectories(len(kinds), m, scene_map(), seed=seed)
    lb0, ub0 = gtop.GtopContext.default_bounds(b.waypoints)
    assert np.all(lb0 < b.x) and np.all(b.x < ub0)           # the start strictly inside the default box
    rows = [apply_kind(k, b.x[i], lb0[i], ub0[i]) for i, k in enumerate(kinds)]
    x0, lb, ub = (np.ascontiguousarray(np.stack([r[j] for r in rows])) for j in range(3))
    assert np.all(lb <= ub)
    return b.T, b.Df, x0, lb, ub, kinds
