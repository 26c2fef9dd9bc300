"""The batched CCSA-MMA optimizer on the device on every KIND of bound and at the limits of its segment count.

Every other device test of the optimizer draws its bounds from default_bounds(): finite, symmetric about the waypoint,
the start strictly inside.  The rows of tests/bound_cases.py are open on one side or both, fixed (lb == ub), start on a
face or outside the box, a thousand times tighter or wider — each in every body of the loop (ten lanes per segment,
two trajectories per wavefront, five lanes per segment, the chunked body at its first, an unpadded and its last
length), in the three launch forms, with and without stop tolerances.

The reference of (a) is the SERIAL algorithm: csrc/mma.hpp around the oracle callback (oracle.optimize_batch /
oracle.mma_trace).  No row is excused: tests/test_bound_cases.py shows on the CPU that no decision on the serial road
of a committed case is within 1e-6 of a tie, a thousand times what the two callbacks differ by."""
import ctypes

import numpy as np
import pytest

from tests import bound_cases

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
TOL_ROAD = 1e-6        # best cost and best point against the serial road (test_device_lockstep_mma_follows_the_serial_algorithm)
TOL_CALLBACK = {"f64": 1e-5, "f32": 2e-4}   # the returned cost against the callback at the returned point
TOL_START = {"f64": 1e-9, "f32": 2e-4}      # "no worse than the start": the two callbacks' difference on the start's cost
GEOMS_13 = [pytest.param(m, pin, id=f"m{m}-pin{pin}-{body}") for m, pin, body, _ in bound_cases.GEOMETRIES if m <= 13]
GEOMS_F32 = [pytest.param(m, pin, id=f"m{m}-pin{pin}-{body}") for m, pin, body, _ in bound_cases.F32_GEOMETRIES]
GEOM_RULES = [pytest.param(m, pin, rule, id=f"m{m}-pin{pin}-{body}-{rule}") for m, pin, body, _ in bound_cases.GEOMETRIES
              for rule in bound_cases.rules_for(m)]
ALL_FIXED = {"cap": None, "ftol": (2, 3), "xtol": (2, 4), "both": (2, 4)}     # (nevals, code); None: (cap, 5)


class Lab:
    """One context on the scene of tests/test_optimizer.py; every device run and every serial road computed once."""

    def __init__(self, gtop, oracle):
        self.oracle = oracle
        mp = bound_cases.scene_map()
        self.ctx = gtop.GtopContext(device=0)
        self.ctx.init_sdf_map(mp.map_size, mp.origin, mp.resolution)
        self.ctx.update_sdf_map(mp.obstacle_points())
        self.sdf = oracle.Sdf.from_map_size(mp.origin, mp.resolution, mp.map_size)
        self.sdf.build_from_occupancy(mp.occupancy)
        self.prm = oracle.make_params()
        self._cases, self._runs, self._serial = {}, {}, {}

    def case(self, m):
        if m not in self._cases:
            self._cases[m] = bound_cases.build(m)
        return self._cases[m]

    def optimize(self, T, Df, x0, lb, ub, m, pin, rule, fusion=2, precision="f64"):
        """One call of optimize_batch_ex at the pinned geometry, in the given launch form; the context is put back."""
        ctx = self.ctx
        ctx.set_params()
        ctx.set_problem(T, Df)
        try:
            ctx.set_launch_geometry(0, pin)
            ctx.set_optimizer_precision(precision)
            ctx.set_optimizer_fusion(fusion)
            return ctx.optimize_batch_ex(x0, lb, ub, bound_cases.evals_for(m), **bound_cases.rules_for(m)[rule])
        finally:
            ctx.set_optimizer_fusion(2)
            ctx.set_launch_geometry(0, 0)
            ctx.set_optimizer_precision("f64")

    def run(self, m, pin, rule, fusion=2, precision="f64"):
        """The bound-kind batch of m segments; checked against the properties of (b) the first time it is run."""
        key = (m, pin, rule, fusion, precision)
        if key not in self._runs:
            T, Df, x0, lb, ub, kinds = self.case(m)
            res = self.optimize(T, Df, x0, lb, ub, m, pin, rule, fusion, precision)
            self.check_properties(res, m, pin, rule, fusion, precision)
            self._runs[key] = res
        return self._runs[key]

    def serial(self, m, rule):
        """csrc/mma.hpp around the oracle callback, row by row: (x, cost, nevals, code)."""
        key = (m, rule)
        if key not in self._serial:
            T, Df, x0, lb, ub, kinds = self.case(m)
            cap = bound_cases.evals_for(m)
            tr = [self.oracle.mma_trace(T[i], Df[i], x0[i], lb[i], ub[i], self.sdf, self.prm, cap, **bound_cases.rules_for(m)[rule])
                  for i in range(len(kinds))]
            out = (np.stack([t["x"] for t in tr]), np.array([t["minf"] for t in tr]),
                   np.array([t["nevals"] for t in tr]), np.array([t["code"] for t in tr]))
            if rule == "cap":      # the batched entry point of the same header: the same numbers
                xb, cb, nb, _ = self.oracle.optimize_batch(T, Df, x0, lb, ub, self.sdf, self.prm, cap, nthreads=4)
                assert np.array_equal(xb, out[0]) and np.array_equal(cb, out[1]) and np.array_equal(nb, out[2])
            self._serial[key] = out
        return self._serial[key]

    def check_properties(self, res, m, pin, rule, fusion, precision, rows=None):
        """(b): what holds whatever road the run took.  rows: the rows of the case the run was made of, in its order."""
        T, Df, x0, lb, ub, kinds = self.case(m)
        rows = np.arange(len(kinds)) if rows is None else np.asarray(rows)
        T, Df, x0, lb, ub, kinds = T[rows], Df[rows], x0[rows], lb[rows], ub[rows], [kinds[i] for i in rows]
        xs, costs, nev, code = res
        what = (m, pin, rule, fusion, precision)
        cap = bound_cases.evals_for(m)
        assert np.all(np.isfinite(xs)) and np.all(np.isfinite(costs)), what
        assert np.all(xs >= lb) and np.all(xs <= ub), what                       # both clamps are exact: no slack
        fixed = lb == ub
        assert np.array_equal(xs[fixed], lb[fixed]), what                        # a fixed coordinate never moves
        assert np.all((nev >= 1) & (nev <= cap)) and np.all((code >= 3) & (code <= 5)), what
        assert np.all((code == 5) == (nev == cap)), what
        # the row that cannot move
        for i in [i for i, k in enumerate(kinds) if k == "all-fixed"]:
            assert np.array_equal(xs[i], x0[i]), what
            want = ALL_FIXED[rule] or (cap, 5)
            assert (int(nev[i]), int(code[i])) == want, (what, int(nev[i]), int(code[i]))
            self.ctx.set_problem(T[i:i + 1], Df[i:i + 1])
            self.ctx.set_launch_geometry(0, 3 if (m <= 6 and pin in (0, 3)) else 6)   # the optimizer's body: same sums
            try:
                c_at, _ = self.ctx.eval_batch(x0[i:i + 1])
            finally:
                self.ctx.set_launch_geometry(0, 0)
            assert abs(costs[i] - c_at[0]) <= (1e-12 if precision == "f64" else TOL_CALLBACK["f32"]) * abs(c_at[0]), what
        # a start outside the box is the start clamped into it: the same bits, on every row
        xc = np.clip(x0, lb, ub)
        if not np.array_equal(xc, x0):
            again = self.optimize(T, Df, xc, lb, ub, m, pin, rule, fusion, precision)
            for a, r in zip(again, res):
                assert np.array_equal(a, r), (what, "started from the clamped point")
        # no worse than the (clamped) start; the returned cost is the callback's value at the returned point
        c0 = self.oracle.eval_batch(T, Df, xc, self.sdf, self.prm, nthreads=4)[0]
        assert np.all(costs <= c0 * (1 + TOL_START[precision])), what
        c_chk = self.oracle.eval_batch(T, Df, xs, self.sdf, self.prm, nthreads=4)[0]
        assert np.max(np.abs(c_chk - costs) / np.abs(c_chk)) <= TOL_CALLBACK[precision], what

    def check_road(self, res, m, rule):
        """(a): the serial algorithm's evaluation count, code, best cost and best point, on every row."""
        xs, costs, nev, code = res
        x_ref, c_ref, n_ref, k_ref = self.serial(m, rule)
        kinds = self.case(m)[5]
        for i, kind in enumerate(kinds):
            what = (m, rule, kind, int(nev[i]), int(code[i]), int(n_ref[i]), int(k_ref[i]))
            assert (nev[i], code[i]) == (n_ref[i], k_ref[i]), what
            assert abs(costs[i] - c_ref[i]) <= TOL_ROAD * abs(c_ref[i]), (what, costs[i], c_ref[i])
            assert np.max(np.abs(xs[i] - x_ref[i])) <= TOL_ROAD * max(1.0, np.max(np.abs(x_ref[i]))), what


@pytest.fixture(scope="module")
def lab(gtop, oracle_mod):
    lab = Lab(gtop, oracle_mod)
    yield lab
    lab.ctx.close()


@pytest.mark.parametrize("m,pin,rule", GEOM_RULES)
def test_the_loop_follows_the_serial_algorithm_on_every_kind_of_bound(lab, m, pin, rule):
    """(a) and (b), the one-launch loop: every geometry with the evaluation cap alone, up to 13 segments also under
    ftol_rel, under xtol_rel and under both (x after f: `all-fixed` reports XTOL then), where at least a third of the
    rows stop before the cap."""
    res = lab.run(m, pin, rule)
    lab.check_road(res, m, rule)
    if rule != "cap":
        early = (res[3] != 5) & (res[2] < bound_cases.evals_for(m))
        assert 3 * int(early.sum()) >= len(early), (m, pin, rule, res[2], res[3])


@pytest.mark.parametrize("m,pin", GEOMS_13)
@pytest.mark.parametrize("rule", ["cap", "ftol", "xtol", "both"])
def test_the_three_launch_forms_return_the_same_bits(lab, m, pin, rule):
    """(c): one launch for the loop, one per iteration, two per iteration — x, cost, evaluation count and code."""
    res = lab.run(m, pin, rule)
    for fusion in (1, 0):
        other = lab.run(m, pin, rule, fusion)
        for a, r in zip(other, res):
            assert np.array_equal(a, r), (m, pin, rule, fusion)


@pytest.mark.parametrize("m,pin", [pytest.param(6, 6, id="m6-pin6-two-per-wavefront"), pytest.param(12, 0, id="m12-pin0-five-lanes")])
@pytest.mark.parametrize("rule", ["cap", "ftol", "xtol"])
def test_a_row_does_not_depend_on_its_neighbours(lab, m, pin, rule):
    """(d): the batch in reversed row order (other rows share a wavefront) and `free`, `all-fixed`, `start-on-faces`
    each alone return, row for row, the bits of the forward batch."""
    T, Df, x0, lb, ub, kinds = lab.case(m)
    res = lab.run(m, pin, rule)
    rev = np.arange(len(kinds))[::-1]
    back = lab.optimize(T[rev], Df[rev], x0[rev], lb[rev], ub[rev], m, pin, rule)
    lab.check_properties(back, m, pin, rule, 2, "f64", rows=rev)
    for a, r in zip(back, res):
        assert np.array_equal(a[::-1], r), (m, pin, rule, "reversed")
    for kind in ("free", "all-fixed", "start-on-faces"):
        i = kinds.index(kind)
        alone = lab.optimize(T[i:i + 1], Df[i:i + 1], x0[i:i + 1], lb[i:i + 1], ub[i:i + 1], m, pin, rule)
        lab.check_properties(alone, m, pin, rule, 2, "f64", rows=[i])
        for a, r in zip(alone, res):
            assert np.array_equal(a[0], r[i]), (m, pin, rule, kind, "alone")


@pytest.mark.parametrize("m,pin", GEOMS_F32)
@pytest.mark.parametrize("fusion", [2, 1])
def test_fp32_evaluations_keep_the_exact_properties(lab, m, pin, fusion):
    """(e): the road may part from fp64's at a decision inside fp32's noise, so only what holds on any road: the
    properties of (b) (costs to fp32's 2e-4), what `all-fixed` reports under every rule, and determinism."""
    for rule in bound_cases.rules_for(m):
        res = lab.run(m, pin, rule, fusion, "f32")            # (check_properties: the first time a run is made)
        T, Df, x0, lb, ub, kinds = lab.case(m)
        again = lab.optimize(T, Df, x0, lb, ub, m, pin, rule, fusion, "f32")
        for a, r in zip(again, res):
            assert np.array_equal(a, r), (m, pin, rule, fusion, "second call")


@pytest.mark.parametrize("fusion", [1, 0])
def test_the_longest_problem_in_the_other_launch_forms(lab, fusion):
    """(f): 118 segments — the most one wavefront's LDS holds with the optimizer's state — in the launch forms that
    keep the state in global memory: (a), (b), and the one-launch loop's bits."""
    res = lab.run(118, 0, "cap", fusion)
    lab.check_road(res, 118, "cap")
    for a, r in zip(res, lab.run(118, 0, "cap")):
        assert np.array_equal(a, r), fusion


@pytest.mark.parametrize("fusion", [2, 1, 0])
def test_one_segment_more_is_refused_and_nothing_is_written(lab, gtop, fusion):
    """(f): 119 segments: GTOP_ERR_INVALID in every launch form, through the host entry point and the resident one,
    and the x passed in is left as it was."""
    import torch
    from grad_traj_optimization_amd._lib import GtopStop
    T, Df, x0, lb, ub, kinds = bound_cases.build(119, seed=4219, kinds=bound_cases.LONG_KINDS)
    ctx = lab.ctx
    ctx.set_params()
    ctx.set_problem(T, Df)
    B = len(kinds)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    x = x0.copy()
    cost, nev, code = np.full(B, -7.0), np.full(B, -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
    stop = GtopStop(12, 0.0, 0.0, 0.0)
    dev = torch.device("cuda:0")
    xd, Dfd, Td, lbd, ubd = (torch.tensor(a, device=dev) for a in (x0, Df.reshape(-1, 18), T, lb, ub))
    try:
        ctx.set_optimizer_fusion(fusion)
        rc = ctx._L.gtop_optimize_batch_ex(ctx._h, B, x.ctypes.data_as(dp), lb.ctypes.data_as(dp), ub.ctypes.data_as(dp),
                                           ctypes.byref(stop), cost.ctypes.data_as(dp), nev.ctypes.data_as(ip),
                                           code.ctypes.data_as(ip))
        assert rc == ERR_INVALID
        with pytest.raises(gtop.GtopError) as err:
            ctx.optimize_device_ex(xd, Dfd, Td, lbd, ubd, 12)
        assert err.value.code == ERR_INVALID
        torch.cuda.synchronize()
    finally:
        ctx.set_optimizer_fusion(2)
    assert np.array_equal(x, x0) and np.all(cost == -7.0) and np.all(nev == -7) and np.all(code == -7)
    assert np.array_equal(xd.cpu().numpy(), x0)
    # the context is none the worse for it
    res = lab.run(2, 0, "cap")
    lab.check_road(res, 2, "cap")
