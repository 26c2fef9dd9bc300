"""The continuous-time certificate of pairwise separation (include/gtop_separation_certificate.h:
gtop_certify_separation_device) restated in numpy on the tree of tests/interval_tree_twin.py, statement by statement:
every step is one rounded fp64 operation in the header's order, nothing fused (numpy fuses nothing), so the kernels'
rows are reproduced bit for bit.

A `mutant` names one deliberate mistake (tests/test_sepcert_twin.py kills each of them):
  "no_remainder"   the second-order remainder dropped from the bound
  "no_clamp"       s* not clamped into the interval
  "start_ignored"  row j's start time read as 0 in its local time
  "j_junctions"    the junctions of row j left out of the pieces
  "le_violation"   `<=` for `<` in the violation test
  "cull_centres"   the cull on the distance of the box centres instead of the box distance
  "piece_cap"      the piece walk stopped after 2 m + 2 turns, one short of what a held window can hold"""
import numpy as np

from tests.interval_tree_twin import CERTIFIED, INFLATE, OPEN, SLACK, VIOLATION, Tree, verdict, walk
from tests.separation_twin import start_times

MUTANTS = ("no_remainder", "no_clamp", "start_ignored", "j_junctions", "le_violation", "cull_centres", "piece_cap")
N_PAIR, N_ROW = 8, 10
SHRINK = 1.0 - 2.0 ** -40
BEFORE, AFTER = -1, -2
DIAGONAL = (1.0, np.inf, np.inf, -1.0, -1.0, 0.0, 0.0, 0.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def horner_pos(c, u):
    return ((((c[5] * u + c[4]) * u + c[3]) * u + c[2]) * u + c[1]) * u + c[0]


def horner_vel(c, u):
    return ((((5.0 * c[5]) * u + 4.0 * c[4]) * u + 3.0 * c[3]) * u + 2.0 * c[2]) * u + c[1]


def sample_value(c, u):
    """The library's sample expression: the powers by multiplication, the terms from the highest power down onto 0."""
    t2 = u * u
    t3 = t2 * u
    t4 = t2 * t2
    t5 = t4 * u
    return ((((((0.0 + t5 * c[5]) + t4 * c[4]) + t3 * c[3]) + t2 * c[2]) + u * c[1]) + c[0])


def norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def segment_bounds(c, T):
    """(Acc (3,), Pos, Vel) of coefficients c (3, 6) over a duration T: the header's three Horner bounds."""
    q0, q1, q2, q3, q4, q5 = (np.abs(c)[:, n] for n in range(6))
    acc = ((20.0 * q5 * T + 12.0 * q4) * T + 6.0 * q3) * T + 2.0 * q2
    vel = (((5.0 * q5 * T + 4.0 * q4) * T + 3.0 * q3) * T + 2.0 * q2) * T + q1
    pos = ((((q5 * T + q4) * T + q3) * T + q2) * T + q1) * T + q0
    return acc, (pos[0] + pos[1]) + pos[2], (vel[0] + vel[1]) + vel[2], pos


class RowClock:
    """A row on the common clock: its state at a time a (a segment, or standing) and the breakpoint that ends it."""

    def __init__(self, c, T, start, hold):
        self.c, self.T, self.start, self.hold, self.m = c.reshape(-1, 3, 6), T, np.float64(start), bool(hold), len(T)
        off = np.float64(0.0)
        for k in range(self.m):
            off = off + T[k]
        self.end = self.start + off
        self.s, self.off, self.off_next = 0, np.float64(0.0), np.float64(0.0) + T[0]

    def state(self, a):
        if self.hold and a < self.start:
            return BEFORE, self.start
        if self.hold and a >= self.end:
            return AFTER, np.inf
        while self.s < self.m - 1 and self.start + self.off_next <= a:
            self.s += 1
            self.off = self.off_next
            self.off_next = self.off_next + self.T[self.s]
        return self.s, self.start + self.off_next

    def inside(self, state):
        """(coefficients (3, 6), duration, off) of the row inside a piece."""
        if state >= 0:
            return self.c[state], self.T[state], self.off
        c = np.zeros((3, 6))
        for k in range(3):
            c[k, 0] = self.c[0, k, 0] if state == BEFORE else sample_value(self.c[-1, k], self.T[-1])
        return c, np.float64(0.0), np.float64(0.0)


class Node:
    """What the separation certificate adds to the tree: an interval's midpoint figures and its lower bound, a leaf's
    into lo."""

    def __init__(self, min_sep, mutant):
        self.min_sep, self.mutant = np.float64(min_sep), mutant
        self.lo, self.hi, self.hi_t, self.viol_t = np.inf, np.inf, np.inf, np.inf
        self.leaves = []           # (a, w, lb, status)

    def piece(self, ci, start_i, off_i, cj, start_j, off_j, remc, E):
        self.ci, self.start_i, self.off_i, self.cj, self.start_j, self.off_j = ci, start_i, off_i, cj, start_j, off_j
        self.remc, self.E = remc, E

    def evaluate(self, L, s, base, w, a):
        h = 0.5 * w
        tc = a + h
        with np.errstate(all="ignore"):
            ui = (tc - self.start_i) - self.off_i
            uj = (tc - (0.0 if self.mutant == "start_ignored" else self.start_j)) - self.off_j
            D = [horner_pos(self.ci[k], ui) - horner_pos(self.cj[k], uj) for k in range(3)]
            W = [horner_vel(self.ci[k], ui) - horner_vel(self.cj[k], uj) for k in range(3)]
            dmid = norm3(*D)
            DW = (D[0] * W[0] + D[1] * W[1]) + D[2] * W[2]
            WW = (W[0] * W[0] + W[1] * W[1]) + W[2] * W[2]
            q = (-DW) / WW
            clamped = q if self.mutant == "no_clamp" else np.fmin(np.fmax(q, -h), h)
            st = np.where((WW == 0.0) | np.isnan(q), 0.0, clamped)
            dlin = norm3(D[0] + W[0] * st, D[1] + W[1] * st, D[2] + W[2] * st)
            rem = (self.remc * h) * h
            if self.mutant == "no_remainder":
                rem = 0.0 * rem
            lb = ((dlin * SHRINK) - rem * INFLATE) - self.E
            lb = np.where(np.isnan(lb), -np.inf, lb)
            dmid, lb, tc = np.broadcast_to(dmid, (64,)), np.broadcast_to(lb, (64,)), np.broadcast_to(tc, (64,))
            viol = dmid <= self.min_sep if self.mutant == "le_violation" else dmid < self.min_sep
            cert = lb >= self.min_sep
        d = np.where(np.isnan(dmid), np.inf, dmid)
        j = int(np.argmin(d))                                  # the first of equal values: the earliest time
        if d[j] < self.hi or (d[j] == self.hi and tc[j] < self.hi_t):
            self.hi, self.hi_t = d[j], tc[j]
        if viol.any():
            self.viol_t = min(self.viol_t, tc[viol].min())
        status = np.where(viol, VIOLATION, np.where(cert, CERTIFIED, OPEN))
        return status.tolist(), lb

    def leaf(self, s, a, w, lb, status):
        self.lo = min(self.lo, lb)
        self.leaves.append((a, w, lb, status))


def certify_pair(ci, Ti, start_i, cj, Tj, start_j, min_sep, t_lo=-np.inf, t_hi=np.inf, max_depth=2, max_refine=64,
                 hold_ends=False, mutant=None):
    """One pair's row (8,) and info (pieces: [(a, nxt, state_i, state_j)], leaves) with cull == 0."""
    Ri, Rj = RowClock(ci, Ti, start_i, hold_ends), RowClock(cj, Tj, start_j, hold_ends)
    wlo, whi = np.float64(t_lo), np.float64(t_hi)
    if not hold_ends:
        wlo = np.fmax(np.fmax(wlo, Ri.start), Rj.start)
        whi = np.fmin(np.fmin(whi, Ri.end), Rj.end)
    out = np.array(DIAGONAL)
    info = dict(window=(wlo, whi), pieces=[], leaves=[])
    if not wlo <= whi:
        return out, info
    node, tree = Node(min_sep, mutant), Tree(max_depth, max_refine)
    a, pieces = wlo, 0
    with np.errstate(all="ignore"):
        for it in range(2 * Ri.m + (2 if mutant == "piece_cap" else 3)):
            si, ni = Ri.state(a)
            sj, nj = Rj.state(a)
            nxt = np.fmin(np.fmin(whi, ni), np.inf if mutant == "j_junctions" else nj)
            if nxt > a or (it == 0 and whi == wlo):
                c_i, T_i, off_i = Ri.inside(si)
                c_j, T_j, off_j = Rj.inside(sj)
                acc_i, pos_i, vel_i, _ = segment_bounds(c_i, T_i)
                acc_j, pos_j, vel_j, _ = segment_bounds(c_j, T_j)
                A = acc_i + acc_j
                tmag = np.fmax(np.fmax(np.abs(a), np.abs(nxt)), np.fmax(np.abs(Ri.start), np.abs(Rj.start)))
                remc = 0.5 * norm3(A[0], A[1], A[2])
                E = SLACK * ((pos_i + pos_j) + (vel_i + vel_j) * tmag)
                node.piece(c_i, Ri.start, off_i, c_j, Rj.start, off_j, remc, E)
                walk(node, 0, pieces, a, 0.015625 * (nxt - a), tree)
                info["pieces"].append((a, nxt, si, sj))
                pieces += 1
            if nxt >= whi or not nxt > a:
                break
            a = nxt
    v, first = verdict(node.viol_t, tree.nund)
    out[:] = (v, node.lo, node.hi, node.hi_t if node.hi != np.inf else -1.0, first, tree.nund, tree.nref, pieces)
    info["leaves"] = node.leaves
    return out, info


def row_boxes(coeff, T):
    """(B, 6): (xlo, ylo, zlo, xhi, yhi, zhi) of every row's whole curve, the cull's prepass."""
    coeff = np.asarray(coeff, dtype=np.float64)
    B, m = coeff.shape[:2]
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (B, m))
    box = np.empty((B, 6))
    lane = np.arange(64, dtype=np.float64)
    with np.errstate(all="ignore"):
        for b in range(B):
            lo, hi, nan = np.full(3, np.inf), np.full(3, -np.inf), False
            for s in range(m):
                Ts = T[b, s]
                w = 0.015625 * Ts
                a = lane * w
                h = 0.5 * w
                tc = a + h
                c = coeff[b, s].reshape(3, 6)
                acc, _, _, pos = segment_bounds(c, Ts)
                for k in range(3):
                    p, v = horner_pos(c[k], tc), horner_vel(c[k], tc)
                    r = ((np.abs(v) * h + ((0.5 * acc[k]) * h) * h) * INFLATE) + SLACK * pos[k]
                    lower, upper = p - r, p + r
                    nan |= bool(np.any(np.isnan(lower) | np.isnan(upper)))
                    lo[k], hi[k] = min(lo[k], np.fmin.reduce(lower)), max(hi[k], np.fmax.reduce(upper))
            box[b, :3], box[b, 3:] = (-np.inf, np.inf) if nan else (lo, hi)    # a NaN face: the whole space
    return box


def box_distance(bi, bj, mutant=None):
    with np.errstate(all="ignore"):
        if mutant == "cull_centres":
            g = [0.5 * (bi[k] + bi[3 + k]) - 0.5 * (bj[k] + bj[3 + k]) for k in range(3)]
        else:
            g = [np.fmax(np.fmax(bi[k] - bj[3 + k], bj[k] - bi[3 + k]), 0.0) for k in range(3)]
        return norm3(g[0], g[1], g[2])


def summarise(pairs):
    """rows (B, 10) from pairs (B, B, 8)."""
    B = pairs.shape[0]
    rows = np.empty((B, N_ROW))
    for i in range(B):
        e = np.delete(pairs[i], i, axis=0)
        js = np.delete(np.arange(B), i)
        unsafe, undecided = e[:, 0] == -1.0, e[:, 0] == 0.0
        r = rows[i]
        r[0] = -1.0 if unsafe.any() else (0.0 if undecided.any() else 1.0)
        r[1], r[3] = (e[:, 1].min(), e[:, 2].min()) if len(e) else (np.inf, np.inf)
        r[2] = js[np.flatnonzero(e[:, 1] == r[1])[0]] if r[1] != np.inf else -1.0
        if r[3] != np.inf:
            k = np.flatnonzero(e[:, 2] == r[3])[0]
            r[4], r[5] = js[k], e[k, 3]
        else:
            r[4], r[5] = -1.0, -1.0
        r[6] = e[unsafe, 4].min() if unsafe.any() else -1.0
        r[7], r[8], r[9] = unsafe.sum(), undecided.sum(), (e[:, 7] == -1.0).sum()
    return rows


def certify(coeff, T, t0, min_sep, t_lo=-np.inf, t_hi=np.inf, max_depth=2, max_refine=64, hold_ends=False, cull=False,
            mutant=None, only=None):
    """(pairs (B, B, 8), rows (B, 10), info {(i, j): info of the pair}) as the header defines them.  coeff (B, m, 18),
    T (B, m) or (m,), t0 as gtop_set_start_times takes it.  only: the pairs (i, j), i < j, to compute (the others stay
    the diagonal's row): for tests that look at a few pairs."""
    coeff = np.asarray(coeff, dtype=np.float64)
    B, m = coeff.shape[:2]
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (B, m))
    start = start_times(t0, B)
    pairs = np.empty((B, B, N_PAIR))
    pairs[:] = DIAGONAL
    box = row_boxes(coeff, T) if cull else None
    infos = {}
    for j in range(B):
        for i in range(j):
            if only is not None and (i, j) not in only:
                continue
            if cull:
                bd = box_distance(box[i], box[j], mutant)
                if bd >= min_sep:
                    pairs[i, j] = pairs[j, i] = (1.0, bd * SHRINK, np.inf, -1.0, -1.0, 0.0, 0.0, -1.0)
                    continue
            row, infos[(i, j)] = certify_pair(coeff[i], T[i], start[i], coeff[j], T[j], start[j], min_sep, t_lo, t_hi,
                                              max_depth, max_refine, hold_ends, mutant)
            pairs[i, j] = pairs[j, i] = row
    return pairs, summarise(pairs), infos


def closing_rows():
    """Two rows of two segments of 0.25 (T shared) that fly towards each other along x, 0.375 apart in y, and END facing
    each other: row 0 from x = 1 to 0, row 1 from x = -1 to 0.  Their distance falls until both have ended and is 0.375
    from then on: under hold_ends, with start times 0.125 and 0.25 and the window [0, 2], all six breakpoints are inside
    the window, the pieces are 2 m + 3 = 7, and the least distance is met in the last one, where both stand."""
    c = np.zeros((2, 2, 18))
    c[0, 0, 0], c[0, 0, 1], c[0, 1, 0], c[0, 1, 1] = 1.0, -2.0, 0.5, -2.0
    c[1, 0, 0], c[1, 0, 1], c[1, 1, 0], c[1, 1, 1] = -1.0, 2.0, -0.5, 2.0
    c[1, :, 6] = 0.375
    return c, np.array([0.25, 0.25]), np.array([0.125, 0.25])


def straight_rows(y=0.5, t_meet=1.3125):
    """Two straight constant-velocity rows of two segments (T shared, 1 and 1): row 0 flies x = t - t_meet, row 1 stands
    on the y axis at (0, y, 0) as a polynomial row — every higher coefficient 0, so the remainder is 0; they are closest,
    y apart, at t_meet: 1.3125 is no midpoint (2 k + 1) / 128 of a level-0 interval of either piece."""
    c = np.zeros((2, 2, 18))
    c[0, 0, 0], c[0, 0, 1] = -t_meet, 1.0                 # x = t - t_meet
    c[0, 1, 0], c[0, 1, 1] = 1.0 - t_meet, 1.0            # the second segment, in its local time
    c[1, :, 6] = y
    return c, np.array([1.0, 1.0])


# ---- the cases the device test runs (tests/test_gpu_sepcert.py); tests/test_sepcert_twin.py holds each to deciding ----
# (B, m, seed, shared T, start times, hold_ends, cull, max_depth, max_refine): B = 2 .. 5 and 67 (past one wavefront of
# rows, odd); m = 7 has more pieces than 64 / 8; every kind of T, of start times, of ends, of cull; depth 0 and 3; budgets
# 0 and 1 (it ends inside a pair); "rows_inside": held, with every breakpoint of every row strictly inside the window, so
# that every pair has its 2 m + 3 pieces, the last with both rows standing after their ends
CASES = [
    (2, 2, 501, False, "none", False, False, 3, 1),
    (3, 2, 502, True, "one", True, True, 0, 0),
    (4, 2, 503, False, "rows", False, True, 3, 1),
    (5, 2, 504, True, "rows", True, False, 3, 0),
    (5, 3, 505, False, "rows", False, False, 0, 1),
    (5, 7, 506, False, "rows", True, True, 3, 1),
    (5, 7, 507, True, "none", False, False, 3, 1),
    (5, 3, 510, False, "rows_inside", True, False, 3, 1),
    (67, 2, 508, False, "rows", False, True, 3, 1),
]
CASE_MIN_SEP = 1.5


def case_inputs(case):
    """(coeff, T, t0, keyword arguments of certify) of one case: the random rows of tests/separation_twin.py, each row
    moved as a whole by up to 1.5 m per axis so that some pairs' boxes are apart."""
    from tests.separation_twin import random_rows
    B, m, seed, shared, t0kind, hold, cull, depth, refine = case
    coeff, T = random_rows(B, m, seed, shared_T=shared)
    rng = np.random.default_rng(seed + 1)
    coeff = coeff.copy()
    coeff[:, :, 0::6] += rng.uniform(-1.5, 1.5, (B, 1, 3))
    t0 = None if t0kind == "none" else (0.375 if t0kind == "one" else rng.uniform(0.2, 0.75, B) if t0kind == "rows_inside"
                                        else rng.uniform(0.0, 0.75, B))
    if t0kind == "rows" and B >= 4:
        t0[1] = 50.0               # row 1 starts after every window has ended: no common time, or (held) it stands
    if t0kind == "rows_inside":
        t_lo, t_hi = 0.125, 1.2 * m + 1.0          # past every end: 0.75 + 1.1 m at the most
    elif hold:
        t_lo, t_hi = 0.125, 0.6 * m
    else:
        t_lo, t_hi = (-np.inf, np.inf) if seed % 2 else (0.3, 0.5 * m)
    return coeff, T, t0, dict(min_sep=CASE_MIN_SEP, t_lo=t_lo, t_hi=t_hi, max_depth=depth, max_refine=refine,
                              hold_ends=hold, cull=cull)
