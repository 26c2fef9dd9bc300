"""The continuous-time certificate of pairwise separation without a GPU: the numpy twin (tests/sepcert_twin.py) held to
exact arithmetic (its lower bound never passes the true distance, evaluated with fractions.Fraction on dyadic numbers),
to known answers and to its own laws, seven mutants of it killed by those checks, and the companion header's symbols
and binding table.

The checks have names: `failed_checks(mutant)` runs all of them on the twin or on one mutant of it."""
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import separation_twin as sw
from tests import sepcert_twin as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_sepcert_workspace_bytes", "gtop_certify_separation_device", "gtop_certify_separation_batch")
INF = np.inf
N_DENSE = 2048                     # times per piece beside its first: a power of two keeps them dyadic


bits, same_bits = ct.bits, ct.same_bits


# ---- the curves in exact arithmetic ------------------------------------------------------------------------------
def _exp2(x):
    """e with x = n / 2^e for a finite float x."""
    return float(x).as_integer_ratio()[1].bit_length() - 1


def _int(x, e):
    """x 2^e as an integer (exact: e is at least _exp2(x))."""
    n, d = float(x).as_integer_ratio()
    return n * ((1 << e) // d)


def breakpoints(T, start):
    """start + off_k, k = 0 .. m, and the off_k: every sum rounded, as the header accumulates them."""
    off = [np.float64(0.0)]
    for t in T:
        off.append(off[-1] + np.float64(t))
    return [np.float64(start) + o for o in off], off


def exact_pieces(Ti, start_i, Tj, start_j, t_lo, t_hi, hold):
    """[(a, b, state_i, state_j)] by the header's statement and not by the twin's walk: the sorted distinct breakpoints
    of either row inside the window cut it; a row's state in a piece is read at the piece's midpoint."""
    (bi, _), (bj, _) = breakpoints(Ti, start_i), breakpoints(Tj, start_j)
    wlo, whi = np.float64(t_lo), np.float64(t_hi)
    if not hold:
        wlo, whi = max(wlo, bi[0], bj[0]), min(whi, bi[-1], bj[-1])
    if not wlo <= whi:
        return []
    cuts = sorted({wlo, whi} | {b for b in bi + bj if wlo < b < whi})
    spans = [(wlo, whi)] if wlo == whi else list(zip(cuts[:-1], cuts[1:]))

    def state(bp, mid):
        if hold and mid < Fraction(bp[0]):
            return ct.BEFORE
        if hold and mid >= Fraction(bp[-1]):
            return ct.AFTER
        return min(sum(1 for b in bp[1:-1] if Fraction(b) <= mid), len(bp) - 2)

    return [(a, b, state(bi, (Fraction(a) + Fraction(b)) / 2), state(bj, (Fraction(a) + Fraction(b)) / 2))
            for a, b in spans]


def dense_min_d2(c_i, T_i, start_i, c_j, T_j, start_j, t_lo, t_hi, hold):
    """The least squared distance of the two curves, as a Fraction, over N_DENSE + 1 evenly spaced times of every piece,
    its ends included; None without common time.  Dyadic numbers carried as integers over one power of two: exact."""
    c_i, c_j = c_i.reshape(-1, 3, 6), c_j.reshape(-1, 3, 6)
    rows = []
    for c, T, start in ((c_i, T_i, start_i), (c_j, T_j, start_j)):
        bp, off = breakpoints(T, start)
        held = np.array([ct.sample_value(c[-1, k], np.float64(T[-1])) for k in range(3)])
        rows.append((c, np.float64(start), off, held))
    pieces = exact_pieces(T_i, start_i, T_j, start_j, t_lo, t_hi, hold)
    if not pieces:
        return None
    F = max(_exp2(v) for c, _, _, held in rows for v in list(c.reshape(-1)) + list(held))
    E = 11 + max(_exp2(v) for a, b, _, _ in pieces for v in (a, b)) if pieces else 0
    E = max([E] + [_exp2(v) for _, start, off, _ in rows for v in [start] + off])
    shift = [1 << ((5 - n) * E) for n in range(6)]
    best = None
    for a, b, s_i, s_j in pieces:
        A, step = _int(a, E), (_int(b, E) - _int(a, E)) // N_DENSE
        assert step * N_DENSE == _int(b, E) - _int(a, E)
        polys = []
        for (c, start, off, held), s in zip(rows, (s_i, s_j)):
            if s >= 0:
                C = [[_int(c[s, k, n], F) * shift[n] for n in range(6)] for k in range(3)]
                origin = _int(start, E) + _int(off[s], E)
            else:
                S = c[0, :, 0] if s == ct.BEFORE else held
                C = [[_int(S[k], F) * shift[0], 0, 0, 0, 0, 0] for k in range(3)]
                origin = 0
            polys.append((C, origin))
        for k in range(N_DENSE + 1 if step else 1):
            t = A + step * k
            d2 = 0
            for axis in range(3):
                p = []
                for C, origin in polys:
                    u, c6 = t - origin, C[axis]
                    p.append(((((c6[5] * u + c6[4]) * u + c6[3]) * u + c6[2]) * u + c6[1]) * u + c6[0])
                d2 += (p[0] - p[1]) ** 2
            best = d2 if best is None or d2 < best else best
    return Fraction(best, 1 << (2 * (F + 5 * E)))


@functools.lru_cache(maxsize=None)
def sound_case(m, seed, with_t0, hold):
    """A batch of five random rows and the exact dense least squared distance of each of its pairs over the window."""
    coeff, T = sw.random_rows(5, m, seed)
    t0 = np.random.default_rng(seed + 100).uniform(0.0, 0.75, 5) if with_t0 else None
    start = sw.start_times(t0, 5)
    t_lo, t_hi = (0.125, 0.5 * m + 0.25) if hold else (-INF, INF)
    dense = {(i, j): dense_min_d2(coeff[i], T[i], start[i], coeff[j], T[j], start[j], t_lo, t_hi, hold)
             for j in range(5) for i in range(j)}
    return coeff, T, t0, t_lo, t_hi, dense


SOUND_CASES = [(2, 41, False, False), (2, 42, True, False), (2, 43, True, True), (2, 44, False, True),
               (3, 45, True, False), (3, 46, False, True), (3, 47, True, True), (3, 48, False, False)]
MIN_SEP = 1.0
SHRINK2 = Fraction(ct.SHRINK) ** 2


def pair_faults(row, d2, min_sep):
    """What is wrong with a pair's row against the exact dense least squared distance d2 (None: no common time)."""
    verdict, lo, hi = row[0], row[1], row[2]
    if d2 is None:
        return [] if (verdict, lo, hi) == (1.0, INF, INF) else ["a row without common time"]
    faults = []
    if lo == INF or (lo > 0.0 and Fraction(lo) ** 2 > d2):
        faults.append(f"lo {lo!r} passes the true distance {float(d2) ** 0.5!r}")
    if hi != INF and Fraction(hi) ** 2 < d2 * SHRINK2:
        faults.append(f"hi {hi!r} is below the least distance {float(d2) ** 0.5!r}")
    if verdict == 1.0 and not lo >= min_sep:
        faults.append("SAFE with lo < min_sep")
    if verdict == -1.0 and not hi < min_sep:
        faults.append("UNSAFE with hi >= min_sep")
    return faults


def parabola_rows():
    """Row 0 stands at the origin; row 1 flies y = 1 - t^2 over two segments of 0.25 (the second in its local time):
    the distance falls to 0.75 at the window's end, where the first-order model alone overshoots it by h^2."""
    c = np.zeros((2, 2, 18))
    c[1, 0, 6], c[1, 0, 8] = 1.0, -1.0
    c[1, 1, 6], c[1, 1, 7], c[1, 1, 8] = 0.9375, -0.5, -1.0
    return c, np.array([0.25, 0.25])


def soundness_faults(mutant=None, cases=SOUND_CASES):
    faults = []
    for case in cases:
        coeff, T, t0, t_lo, t_hi, dense = sound_case(*case)
        for cull in (False, True):
            pairs, rows, infos = ct.certify(coeff, T, t0, MIN_SEP, t_lo, t_hi, hold_ends=case[3], cull=cull,
                                            mutant=mutant)
            start = sw.start_times(t0, 5)
            for (i, j), d2 in dense.items():
                faults += [(case, cull, i, j, f) for f in pair_faults(pairs[i, j], d2, MIN_SEP)]
                if (i, j) in infos:     # the pair walked the tree: its pieces are the header's, found independently
                    want = exact_pieces(T[i], start[i], T[j], start[j], t_lo, t_hi, case[3])
                    if infos[(i, j)]["pieces"] != want or pairs[i, j, 7] != len(want):
                        faults.append((case, cull, i, j, "the pieces walked are not the header's"))
    c, T = parabola_rows()
    d2 = dense_min_d2(c[0], T, 0.0, c[1], T, 0.0, -INF, INF, False)
    assert d2 == Fraction(9, 16)
    pairs, _, _ = ct.certify(c, T, None, 0.7, mutant=mutant)
    faults += [("parabola", f) for f in pair_faults(pairs[0, 1], d2, 0.7)]
    c, T, t0 = ct.closing_rows()
    d2 = dense_min_d2(c[0], T, t0[0], c[1], T, t0[1], 0.0, 2.0, True)
    assert d2 == Fraction(9, 64)
    for min_sep in (0.3, 0.376):
        pairs, _, infos = ct.certify(c, T, t0, min_sep, 0.0, 2.0, hold_ends=True, mutant=mutant)
        faults += [("closing", min_sep, f) for f in pair_faults(pairs[0, 1], d2, min_sep)]
        if infos[(0, 1)]["pieces"] != exact_pieces(T, t0[0], T, t0[1], 0.0, 2.0, True):
            faults.append(("closing", min_sep, "the pieces walked are not the header's"))
    return faults


# ---- known answers ---------------------------------------------------------------------------------------------------
def slack_of(pos, vel, tmag):
    return ct.SLACK * (pos + vel * tmag)


def near(lo, d, E):
    """The law of a known lower bound: d (1 - 2^-39) - E <= lo <= d."""
    return d * (1.0 - 2.0 ** -39) - E <= lo <= d


def known_faults(mutant=None):
    """The names of the known-answer checks the twin (or one mutant of it) fails."""
    bad = set()
    c, T = ct.straight_rows()
    run = lambda min_sep, t0=None, **kw: ct.certify(c, T, t0, min_sep, mutant=mutant, **kw)[0][0, 1]
    E = slack_of(1.3125 + 0.5, 1.0, 2.0)                  # the piece [1, 2]: |c0| + |c1| T, the speed, the largest time
    # head_on: closest, 0.5 apart, at 1.3125: the end of a level-0 interval, so no midpoint sees it
    r = run(0.49)
    if not (r[0] == 1.0 and near(r[1], 0.5, E) and 0.5 < r[2] <= np.hypot(0.5, 1.0 / 128) and r[3] == 1.3125 - 1.0 / 128
            and r[4] == -1.0 and r[5] == 0.0 and r[7] == 2.0):
        bad.add("head_on")
    r = run(0.51)
    if not (r[0] == -1.0 and r[2] < 0.51 and 1.0 < r[4] < 1.3125):
        bad.add("head_on")
    # window: the window ends at 1, before the rows meet: the least distance is at its end, where s* is clamped
    d1 = np.sqrt(0.3125 * 0.3125 + 0.25)
    r = run(0.55, t_hi=1.0)
    if not (r[0] == 1.0 and near(r[1], d1, E) and r[7] == 1.0):
        bad.add("window")
    # late_start: the mover is row j and starts 0.25 late: three pieces, and the rows meet 0.25 later
    cs = c[::-1].copy()
    r = ct.certify(cs, T, [0.0, 0.25], 0.49, mutant=mutant)[0][0, 1]
    if not (r[0] == 1.0 and near(r[1], 0.5, slack_of(1.8125, 1.0, 2.0)) and r[7] == 3.0
            and abs(r[3] - 1.5625) <= 0.75 / 128):
        bad.add("late_start")
    # no common time: disjoint flown ranges
    r = run(0.49, t0=[0.0, 5.0])
    if not same_bits(r, ct.DIAGONAL):
        bad.add("disjoint")
    # instant: a window of one instant is evaluated; at min_sep = the distance itself it is neither a violation (`<`) nor
    # certified (the bound is shrunk)
    r = run(0.49, t_lo=1.3125, t_hi=1.3125)
    if not (r[0] == 1.0 and r[2] == 0.5 and r[3] == 1.3125 and near(r[1], 0.5, E) and r[7] == 1.0):
        bad.add("instant")
    r = run(0.5, t_lo=1.3125, t_hi=1.3125, max_refine=0)
    if not (r[0] == 0.0 and r[4] == -1.0 and r[5] == 64.0):
        bad.add("instant")
    # equal rows
    r = ct.certify(c[[0, 0]], T, None, 0.49, mutant=mutant)[0][0, 1]
    if not (r[0] == -1.0 and r[2] == 0.0 and r[4] == 1.0 / 128 and r[1] <= 0.0):
        bad.add("equal_rows")
    # standing: past both rows' ends each stands where it ended (the static row starts at 1): held, two pieces; not held,
    # no common time
    dh = np.sqrt(0.6875 * 0.6875 + 0.25)
    r = run(0.49, t0=[0.0, 1.0], t_lo=2.5, t_hi=4.0, hold_ends=True)
    if not (r[0] == 1.0 and r[2] == dh and r[3] == 2.5 + 1.0 / 256 and near(r[1], dh, slack_of(1.1875, 0.0, 4.0))
            and r[7] == 2.0):
        bad.add("standing")
    if not same_bits(run(0.49, t0=[0.0, 1.0], t_lo=2.5, t_hi=4.0), ct.DIAGONAL):
        bad.add("standing")
    r = run(0.49, t0=[0.0, 1.0], t_lo=0.0, t_hi=4.0, hold_ends=True)          # before its start the static row stands too
    if not (r[0] == 1.0 and r[7] == 4.0 and near(r[1], 0.5, slack_of(1.8125, 1.0, 4.0))):
        bad.add("standing")
    # all_inside: held, every breakpoint of both rows strictly inside the window: 2 m + 3 = 7 pieces, and the least
    # distance, 0.375 exactly, is met only in the last one, where both rows stand after their ends
    cc, Tc, t0c = ct.closing_rows()
    r = ct.certify(cc, Tc, t0c, 0.3, 0.0, 2.0, hold_ends=True, mutant=mutant)[0][0, 1]
    if not (r[0] == 1.0 and r[7] == 7.0 and r[2] == 0.375 and r[3] == 0.75 + 1.25 / 128
            and near(r[1], 0.375, slack_of(1.375, 2.0, 0.75))):     # (the least leaf: the end of [0.625, 0.75], where
                                                                      # row 1 still flies; that piece's slack)
        bad.add("all_inside")
    r = ct.certify(cc, Tc, t0c, 0.376, 0.0, 2.0, hold_ends=True, mutant=mutant)[0][0, 1]
    if not (r[0] == -1.0 and r[7] == 7.0 and r[2] == 0.375 and 0.625 < r[4] < 0.75):
        bad.add("all_inside")
    # cull: the mover's box spans x, so the boxes are 0.5 apart where their centres are 0.59 apart
    r = run(0.55, cull=True)
    if not (r[0] == -1.0 and r[7] == 2.0):
        bad.add("cull")
    r = run(0.45, cull=True)
    if not (r[0] == 1.0 and 0.5 * (1.0 - 2.0 ** -37) <= r[1] <= 0.5 and r[2] == INF and r[7] == -1.0):
        bad.add("cull")
    return bad


def symmetry_faults(mutant=None):
    faults = []
    for m, seed, with_t0, hold in SOUND_CASES[:4]:
        coeff, T, t0, t_lo, t_hi, _ = sound_case(m, seed, with_t0, hold)
        start = sw.start_times(t0, 5)
        for i, j in ((0, 1), (2, 4), (3, 1)):
            kw = dict(min_sep=MIN_SEP, t_lo=t_lo, t_hi=t_hi, hold_ends=hold, mutant=mutant)
            a, _ = ct.certify_pair(coeff[i], T[i], start[i], coeff[j], T[j], start[j], **kw)
            b, _ = ct.certify_pair(coeff[j], T[j], start[j], coeff[i], T[i], start[i], **kw)
            if not same_bits(a, b):
                faults.append((seed, i, j))
    return faults


def failed_checks(mutant=None):
    bad = known_faults(mutant)
    if soundness_faults(mutant, SOUND_CASES[:4] if mutant else SOUND_CASES):
        bad.add("soundness")
    if mutant not in ("start_ignored", "j_junctions") and symmetry_faults(mutant):   # (these two treat j apart by design)
        bad.add("symmetry")
    return bad


def test_the_twin_passes_every_check():
    assert known_faults() == set()
    assert failed_checks() == set()


def test_soundness_in_exact_arithmetic():
    """lo never passes the true distance, hi is never below the least one, whatever the verdict; with and without start
    times, both kinds of ends, cull 0 and 1."""
    assert soundness_faults() == []
    # not vacuous: every verdict is met, pairs are culled, and some pair has no common time
    seen, culled = set(), 0
    for case in SOUND_CASES:
        coeff, T, t0, t_lo, t_hi, dense = sound_case(*case)
        pairs, rows, _ = ct.certify(coeff, T, t0, MIN_SEP, t_lo, t_hi, hold_ends=case[3], cull=True)
        seen |= set(pairs[..., 0].reshape(-1).tolist())
        culled += int(rows[:, 9].sum())
    assert {1.0, -1.0} <= seen and culled > 0


def test_the_pair_is_symmetric_bit_for_bit():
    assert symmetry_faults() == []


@pytest.mark.parametrize("case", range(len(ct.CASES)))
def test_the_committed_cases_decide(case):
    """No pair of a case the device test runs is left UNDECIDED at max_depth = 2: the device test cannot pass by leaving
    pairs out of its comparison."""
    coeff, T, t0, kw = ct.case_inputs(ct.CASES[case])
    kw = dict(kw, max_depth=2, max_refine=64)
    pairs, rows, _ = ct.certify(coeff, T, t0, **kw)
    assert not np.any(pairs[..., 0] == 0.0), np.argwhere(pairs[..., 0] == 0.0)[:5]
    B = coeff.shape[0]
    if B >= 4:
        assert np.any(pairs[..., 0] == -1.0) and np.any(pairs[..., 7] > 0)     # both verdicts, pairs that walk the tree
    if ct.CASES[case][4] == "rows_inside":                                      # every pair has its 2 m + 3 pieces
        off = ~np.eye(B, dtype=bool)
        assert np.all(pairs[..., 7][off] == 2 * coeff.shape[1] + 3)


CAUGHT_BY = {"no_remainder": "soundness", "no_clamp": "window", "start_ignored": "late_start",
             "j_junctions": "late_start", "le_violation": "instant", "cull_centres": "cull", "piece_cap": "all_inside"}


@pytest.mark.parametrize("mutant", ct.MUTANTS)
def test_every_mutant_is_killed(mutant):
    bad = known_faults(mutant)
    if CAUGHT_BY[mutant] == "soundness":
        c, T = parabola_rows()
        pairs, _, _ = ct.certify(c, T, None, 0.7, mutant=mutant)
        if pair_faults(pairs[0, 1], Fraction(9, 16), 0.7):
            bad.add("soundness")
    assert CAUGHT_BY[mutant] in bad, (mutant, bad)
    if mutant in ("j_junctions", "start_ignored", "cull_centres"):     # the exact check sees these on random rows too
        assert soundness_faults(mutant, SOUND_CASES[1:2])
    if mutant == "piece_cap":                                          # and the piece cross-check sees this one
        assert any("pieces" in str(f) for f in soundness_faults(mutant, []))


def test_the_row_summary_restates_the_matrix():
    coeff, T, t0, t_lo, t_hi, _ = sound_case(*SOUND_CASES[1])
    pairs, rows, _ = ct.certify(coeff, T, t0, MIN_SEP, cull=True)
    for i in range(5):
        e = np.delete(pairs[i], i, axis=0)
        assert same_bits(pairs[i, i], ct.DIAGONAL)
        assert rows[i, 1] == e[:, 1].min() and rows[i, 3] == e[:, 2].min()
        assert rows[i, 7] == np.count_nonzero(e[:, 0] == -1) and rows[i, 8] == np.count_nonzero(e[:, 0] == 0)
        assert rows[i, 0] == (-1 if rows[i, 7] else (0 if rows[i, 8] else 1))
        assert pairs[i, int(rows[i, 2]), 1] == rows[i, 1] and rows[i, 9] == np.count_nonzero(e[:, 7] == -1)
    assert same_bits(pairs, pairs.transpose(1, 0, 2))
    one, rows1, _ = ct.certify(coeff[:1], T[:1], None, MIN_SEP)
    assert same_bits(one[0, 0], ct.DIAGONAL) and rows1[0].tolist() == [1, INF, -1, INF, -1, -1, -1, 0, 0, 0]


# ---- the surface -----------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_versioned(gtop):
    from grad_traj_optimization_amd import separation_certificate as gc
    L = gc.sepcert_library()
    assert L.gtop_sepcert_abi_version() == 1 == gc.SEPCERT_ABI_VERSION == gtop.SEPCERT_ABI_VERSION
    nm = subprocess.run(["nm", "-D", "--defined-only", gtop.library_path()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert set(NAMES) | {"gtop_sepcert_abi_version"} <= exported
    for name in ("GtopSepCertOpts", "SEPCERT_PAIR", "SEPCERT_ROW", "SEPCERT_ABI_VERSION", "SEPCERT_ENTRY_POINTS",
                 "sepcert_library", "sepcert_workspace_bytes", "certify_separation_device", "certify_separation_batch"):
        assert hasattr(gtop, name) and name in gtop.__all__, name
    assert len(gc.SEPCERT_PAIR) == 8 == ct.N_PAIR and len(gc.SEPCERT_ROW) == 10 == ct.N_ROW
    o = gc.GtopSepCertOpts()
    assert (o.hold_ends, o.cull, o.reserved[0], o.reserved[1]) == (0, 0, 0, 0)


def test_binding_table_covers_the_header(gtop):
    import ctypes as C
    from grad_traj_optimization_amd import separation_certificate as gc
    text = open(os.path.join(ROOT, "include", "gtop_separation_certificate.h")).read()
    body = text[text.index("#ifndef GTOP_SEPARATION_CERTIFICATE_H_"):]
    decl = dict(re.findall(r"^int (gtop_\w+)\(([^;]*)\);", body, flags=re.M | re.S))
    assert set(decl) == set(gc.SEPCERT_ENTRY_POINTS) == set(NAMES) | {"gtop_sepcert_abi_version"}
    for name, args in decl.items():
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip()
        n = 0 if args == "void" else args.count(",") + 1
        since, restype, argtypes = gc.SEPCERT_ENTRY_POINTS[name]
        assert since == 1 and restype is C.c_int and len(argtypes) == n, name
    # the struct as the header lays it out: three doubles and six 32-bit words
    assert C.sizeof(gc.GtopSepCertOpts) == 48
    assert [f[0] for f in gc.GtopSepCertOpts._fields_] == ["min_sep", "t_lo", "t_hi", "max_depth", "max_refine",
                                                           "hold_ends", "cull", "reserved"]
    for macro, value in (("GTOP_SEPCERT_ABI_VERSION", 1), ("GTOP_SEPCERT_PAIR", 8), ("GTOP_SEPCERT_ROW", 10),
                         ("GTOP_SEPCERT_MAX_B", 2048)):
        assert re.search(rf"^#define {macro} {value}\b", body, flags=re.M), macro
    assert "256 MiB" in body and gc.SEPCERT_MAX_B == 2048


def test_workspace_bytes_is_pure_and_bounded(gtop):
    """No context and no GPU: the size for B rows, monotone, and the refusals."""
    from grad_traj_optimization_amd import separation_certificate as gc
    assert gc.sepcert_workspace_bytes(0) == 0
    assert gc.sepcert_workspace_bytes(1) >= 6 * 8 and gc.sepcert_workspace_bytes(2048) >= 2048 * 6 * 8
    assert gc.sepcert_workspace_bytes(67) >= gc.sepcert_workspace_bytes(66)
    assert gc.sepcert_workspace_bytes(5) == gc.sepcert_workspace_bytes(5)
    for B in (-1, 2049):
        with pytest.raises(ValueError):
            gc.sepcert_workspace_bytes(B)
    assert gc.sepcert_library().gtop_sepcert_workspace_bytes(1, None) == 1


def test_the_older_surfaces_are_untouched(gtop):
    from grad_traj_optimization_amd import _abi
    from grad_traj_optimization_amd import separation as gs
    assert _abi.ABI_VERSION == 12 and gtop.load_library().gtop_abi_version() == 12
    assert gs.SEP_ABI_VERSION == 1 and gs.sep_library().gtop_sep_abi_version() == 1 and len(gs.SEP_ENTRY_POINTS) == 5
    assert not [n for n in list(_abi.ENTRY_POINTS) + list(gs.SEP_ENTRY_POINTS) if "sepcert" in n or "certify_sep" in n]
    for header in ("gtop.h", "gtop_separation.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "sepcert" not in text.lower() and "certify_separation" not in text, header
