"""Pairwise separation and distinct-candidate selection without a GPU: the numpy twin (tests/separation_twin.py) held
to known answers in dyadic numbers and to the figures' own laws, five mutants of it killed by those checks, and the
companion header's symbols and binding table.

The checks have names (CHECKS): `failed_checks(mutant)` runs all of them on the twin or on one mutant of it."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import separation_twin as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_separation_workspace_bytes", "gtop_separation_device", "gtop_separation_batch",
         "gtop_select_distinct_device")
INF = np.inf
GRID = dict(t_lo=0.0, dt=0.25, n=17)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- known answers: every number is dyadic or a correctly rounded sqrt of one, so every figure is exact ----
def known_answers():
    """[(name, kwargs of sw.separation on sw.known_rows(), rows taken, pair_min, pair_max, row summaries)]."""
    r2 = np.sqrt(16.25)
    cases = []
    # rows 0 and 1 meet head-on, 0.5 apart in y: closest at tau = 2, farthest (4, 0.5) apart at tau = 0 and 4
    cases.append(("head_on", dict(t0=None, hold_ends=False, radius=1.0), [0, 1],
                  [[INF, 0.5], [0.5, INF]], [[-INF, r2], [r2, -INF]],
                  [[0.5, 1, 2.0, 1, 1, 17], [0.5, 0, 2.0, 1, 1, 17]]))
    # row 1 starts 1 s later: flown at tau = 1 .. 4 of the grid (13 samples), x_1 = 5 - tau: closest at tau = 2.5,
    # farthest over the common samples at tau = 1 and 4: (3, 0.5)
    r1 = np.sqrt(9.25)
    cases.append(("late_start", dict(t0=[0.0, 1.0, 1.0], hold_ends=False, radius=0.5), [0, 1],
                  [[INF, 0.5], [0.5, INF]], [[-INF, r1], [r1, -INF]],
                  [[0.5, 1, 2.5, 0, 1, 17], [0.5, 0, 2.5, 0, 1, 13]]))
    # the same, held: row 1 stands at x = 4 before its start, so tau = 0 gives (4, 0.5) again
    cases.append(("late_start_held", dict(t0=[0.0, 1.0, 1.0], hold_ends=True, radius=0.0), [0, 1],
                  [[INF, 0.5], [0.5, INF]], [[-INF, r2], [r2, -INF]],
                  [[0.5, 1, 2.5, 0, 1, 17], [0.5, 0, 2.5, 0, 1, 17]]))
    # row 2 starts at tau = 10: flown nowhere on the grid
    cases.append(("no_overlap", dict(t0=[0.0, 0.0, 10.0], hold_ends=False, radius=1.0), [0, 1, 2],
                  [[INF, 0.5, INF], [0.5, INF, INF], [INF, INF, INF]],
                  [[-INF, r2, -INF], [r2, -INF, -INF], [-INF, -INF, -INF]],
                  [[0.5, 1, 2.0, 1, 1, 17], [0.5, 0, 2.0, 1, 1, 17], [INF, -1, -1, 0, 0, 0]]))
    return cases


def tie_rows():
    """Row 0 and two copies of row 1: row 0 is equally near both."""
    c, T = sw.known_rows()
    return c[[0, 1, 1]], T


def run_known(name, mutant=None, separation=sw.separation):
    for case, kw, take, want_min, want_max, want_rows in known_answers():
        if case == name:
            c, T = sw.known_rows()
            t0 = kw["t0"]
            if t0 is not None:
                t0 = [t0[i] for i in take]
            got = separation(c[take], T, t0, hold_ends=kw["hold_ends"], radius=kw["radius"], mutant=mutant, **GRID)
            return got, (np.array(want_min), np.array(want_max), np.array(want_rows, dtype=np.float64))
    raise KeyError(name)


def selection_case(seed, B=40):
    """(passed, cost, pair_max, min_gap, K): costs with ties, NaN and inf among them, clusters of near-identical rows."""
    rng = np.random.default_rng(seed)
    cluster = rng.integers(0, 6, B)
    centre = rng.uniform(0.0, 10.0, 6)
    x = centre[cluster] + rng.uniform(-0.05, 0.05, B)
    pair_max = np.abs(x[:, None] - x[None, :])
    np.fill_diagonal(pair_max, -np.inf)
    cost = rng.integers(0, 12, B).astype(np.float64)
    cost[rng.integers(0, B, 2)] = np.inf
    cost[rng.integers(0, B, 2)] = np.nan
    passed = (rng.integers(0, 4, B) != 0).astype(np.uint8)
    return passed, cost, pair_max, 0.5, 8


def laws_fail(pair_min, pair_max):
    B = pair_min.shape[0]
    d = np.arange(B)
    has = np.isfinite(pair_min)
    return not (same_bits(pair_min, pair_min.T) and same_bits(pair_max, pair_max.T)
                and np.all(pair_min[d, d] == np.inf) and np.all(pair_max[d, d] == -np.inf)
                and np.all(pair_min[has] <= pair_max[has]) and np.all(pair_max[~has] == -np.inf))


def failed_checks(mutant=None):
    """The names of the checks the twin (or one mutant of it) fails."""
    bad = set()
    for name in ("head_on", "late_start", "late_start_held", "no_overlap"):
        got, want = run_known(name, mutant)
        if not all(same_bits(g, w) for g, w in zip(got, want)):
            bad.add(name)
    # tie: row 0 is 0.5 from rows 1 and 2 alike and names the lower
    c, T = tie_rows()
    _, _, rows = sw.separation(c, T, None, mutant=mutant, **GRID)
    if not (rows[0, 0] == 0.5 and rows[0, 1] == 1 and rows[1, 0] == 0.0 and rows[1, 1] == 2 and rows[2, 1] == 1):
        bad.add("tie")
    # laws on random rows, per-row start times, both kinds of ends
    coeff, T = sw.random_rows(7, 3, 11)
    t0 = np.random.default_rng(12).uniform(0.0, 1.5, 7)
    for hold in (False, True):
        kw = dict(t_lo=0.25, dt=0.125, n=21, hold_ends=hold, radius=2.0, mutant=mutant)
        pmin, pmax, rows = sw.separation(coeff, T, t0, **kw)
        if laws_fail(pmin, pmax):
            bad.add("laws")
        perm = np.random.default_rng(13).permutation(7)
        qmin, qmax, qrows = sw.separation(coeff[perm], T[perm], t0[perm], **kw)
        if not (same_bits(qmin, pmin[np.ix_(perm, perm)]) and same_bits(qmax, pmax[np.ix_(perm, perm)])
                and same_bits(qrows[:, [0, 2, 3, 4, 5]], rows[perm][:, [0, 2, 3, 4, 5]])):
            bad.add("permutation")
        for i, j in ((0, 1), (2, 6), (5, 3)):
            two = [i, j]
            smin, smax, _ = sw.separation(coeff[two], T[two], t0[two], **kw)
            if not (same_bits(smin[0, 1], pmin[i, j]) and same_bits(smax[0, 1], pmax[i, j])):
                bad.add("batch_independence")
    # the selection: each choice correct, the run complete, chosen[0] the cheapest eligible row
    for seed in (21, 22, 23):
        passed, cost, pair_max, gap, K = selection_case(seed)
        for p in (passed, None):
            chosen, count = sw.select_distinct(p, cost, pair_max, gap, K, mutant=mutant)
            if sw.selection_faults(p, cost, pair_max, gap, K, chosen, count):
                bad.add("selection")
    return bad


def test_the_twin_passes_every_check():
    assert failed_checks() == set()


@pytest.mark.parametrize("name", ["head_on", "late_start", "late_start_held", "no_overlap"])
def test_known_answers_in_dyadic_numbers(name):
    got, want = run_known(name)
    for g, w, what in zip(got, want, ("pair_min", "pair_max", "rows")):
        assert same_bits(g, w), (name, what, g, w)


def test_laws_on_random_rows():
    coeff, T = sw.random_rows(9, 4, 31, shared_T=True)
    t0 = np.random.default_rng(32).uniform(0.0, 2.0, 9)
    pmin, pmax, rows = sw.separation(coeff, T, t0, 0.0, 0.0625, 40, hold_ends=False, radius=1.5)
    assert not laws_fail(pmin, pmax)
    # the summary restates the matrix row
    for i in range(9):
        others = np.delete(pmin[i], i)
        assert rows[i, 0] == others.min() and rows[i, 3] == np.count_nonzero(others < 1.5)
        assert rows[i, 4] == np.count_nonzero(np.isfinite(others))
        assert rows[i, 1] == (-1 if np.isinf(rows[i, 0]) else np.flatnonzero(pmin[i] == rows[i, 0])[0])
    assert np.any(rows[:, 5] < 40) and np.all(rows[:, 5] > 0)
    # held ends: every row is flown at every sample, so every pair has a common one
    hmin, hmax, hrows = sw.separation(coeff, T, t0, 0.0, 0.0625, 40, hold_ends=True)
    assert np.all(hrows[:, 5] == 40) and np.all(hrows[:, 4] == 8) and np.all(hrows[:, 3] == 0)
    assert np.all(hmin <= pmin) and np.all(hmax >= pmax)                 # more common samples: wider on both sides


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_selection_rule(seed):
    passed, cost, pair_max, gap, K = selection_case(seed)
    chosen, count = sw.select_distinct(passed, cost, pair_max, gap, K)
    assert sw.selection_faults(passed, cost, pair_max, gap, K, chosen, count) == []
    assert 2 <= count <= 6                                               # six clusters: at most one row of each
    # min_gap = 0 with every pair overlapping: the K cheapest eligible rows in (cost, index) order
    open_max = np.where(np.isfinite(pair_max), pair_max, 1.0)
    chosen0, count0 = sw.select_distinct(passed, cost, open_max, 0.0, K)
    eligible = np.flatnonzero((passed != 0) & np.isfinite(cost))
    order = eligible[np.lexsort((eligible, cost[eligible]))]
    assert count0 == K and chosen0.tolist() == order[:K].tolist()
    # more asked for than there are: the fill
    few = np.zeros_like(passed)
    few[order[:3]] = 1
    chosen3, count3 = sw.select_distinct(few, cost, open_max, 0.0, K)
    assert count3 == 3 and chosen3.tolist() == order[:3].tolist() + [-1] * (K - 3)
    # no rows
    chosen_e, count_e = sw.select_distinct(None, np.zeros(0), np.zeros((0, 0)), 0.0, 4)
    assert count_e == 0 and chosen_e.tolist() == [-1] * 4


CAUGHT_BY = {"first_dropped": "head_on", "strict_end": "head_on", "always_clamp": "late_start",
             "max_for_min": "head_on", "highest_tie": "tie"}


@pytest.mark.parametrize("mutant", sw.MUTANTS)
def test_every_mutant_is_killed(mutant):
    bad = failed_checks(mutant)
    assert CAUGHT_BY[mutant] in bad, (mutant, bad)
    if mutant == "always_clamp":
        assert "no_overlap" in bad
    if mutant == "highest_tie":
        assert "selection" in bad


# ---- the surface ----
def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import separation as gs
    L = gs.sep_library()
    assert L.gtop_sep_abi_version() == 1 == gs.SEP_ABI_VERSION == gtop.SEP_ABI_VERSION
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_sep_abi_version"} <= exported
    for name in ("GtopSepOpts", "SEP_ROW", "SEP_ABI_VERSION", "SEP_ENTRY_POINTS", "separation_workspace_bytes",
                 "separation_device", "separation_batch", "select_distinct_device"):
        assert hasattr(gtop, name) and name in gtop.__all__, name
    assert len(gs.SEP_ROW) == 6
    o = gs.GtopSepOpts()
    assert (o.hold_ends, o.reserved[0], o.reserved[1]) == (0, 0, 0)


def test_binding_table_covers_the_header(gtop):
    import ctypes as C
    from grad_traj_optimization_amd import separation as gs
    text = open(os.path.join(ROOT, "include", "gtop_separation.h")).read()
    body = text[text.index("#ifndef GTOP_SEPARATION_H_"):]
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gs.SEP_ENTRY_POINTS) == set(NAMES) | {"gtop_sep_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gs.SEP_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # the struct as the header lays it out: three doubles and four 32-bit words
    assert C.sizeof(gs.GtopSepOpts) == 40
    assert [f[0] for f in gs.GtopSepOpts._fields_] == ["t_lo", "dt", "radius", "n_samples", "hold_ends", "reserved"]
    for macro, value in (("GTOP_SEP_ABI_VERSION", 1), ("GTOP_SEP_ROW", 6), ("GTOP_SEP_MAX_SAMPLES", 65536),
                         ("GTOP_SEP_MAX_B", 4096), ("GTOP_SEP_MAX_DISTINCT", 64)):
        assert re.search(rf"^#define {macro} {value}\b", body, flags=re.M), macro
    assert (gs.SEP_MAX_SAMPLES, gs.SEP_MAX_B, gs.SEP_MAX_DISTINCT) == (65536, 4096, 64)


def test_workspace_bytes_is_pure_and_bounded(gtop):
    """No context and no GPU: the size for B rows, monotone in both arguments, and the refusals."""
    from grad_traj_optimization_amd import separation as gs
    assert gs.separation_workspace_bytes(0, 1) == 0
    small = gs.separation_workspace_bytes(1, 1)
    assert small >= 3 * 8                                                # at least the one sample's position
    assert gs.separation_workspace_bytes(130, 25) >= 130 * 25 * 3 * 8
    assert gs.separation_workspace_bytes(2, 1) >= small and gs.separation_workspace_bytes(1, 300) > small
    assert gs.separation_workspace_bytes(4096, 65536) >= 4096 * 65536 * 3 * 8     # past 2^32: size_t
    for B, n in ((-1, 1), (4097, 1), (1, 0), (1, 65537)):
        with pytest.raises(ValueError):
            gs.separation_workspace_bytes(B, n)
    assert gs.sep_library().gtop_separation_workspace_bytes(1, 1, None) == 1


def test_the_surface_of_gtop_h_is_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert not [n for n in _abi.ENTRY_POINTS if "sep_" in n or "separation" in n or "distinct" in n]
    text = open(os.path.join(ROOT, "include", "gtop.h")).read()
    assert "gtop_sep" not in text and "GTOP_SEP" not in text and "gtop_separation" not in text
