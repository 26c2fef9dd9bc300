"""The continuous-time clearance certificate (include/gtop.h: gtop_certify_trajectories_device) restated in numpy for
ONE trajectory, statement by statement where the header fixes the arithmetic (interval ends, radii, cell ranges,
sub-boxes, vertex values: plain fp64 operations, nothing fused — numpy fuses nothing), from pieces that are already
tested: midpoint distances come through the C oracle's evaluateEDTWithGrad (oracle.Sdf.edt_query), corner values from
the field array.  The velocity is numpy's unfused sum where the kernel's poly_vel has fmas: the one place the two may
differ in the last bits, which tests/test_gpu_certify.py bounds.  The tree is the shared walk of
tests/interval_tree_twin.py; Node is what this certificate adds to it.

Also here: the fields and trajectories the tests share (CASES, wall_case), and the mutants the tests must catch."""
import numpy as np

from tests.interval_tree_twin import CERTIFIED, INFLATE, OPEN, SLACK, VIOLATION, Tree, verdict, walk

N_CERT = 8
KAPPA = 2.0 ** -46
MUTANTS = ("no_A", "mid_cell", "floor", "lt", "budget")


class Field:
    """A distance field as the lookup sees it: the z-fastest array and the grid of an oracle.Sdf."""

    def __init__(self, osdf):
        self.osdf = osdf
        self.n = np.array(osdf.grid, dtype=np.int64)
        self.val = np.asarray(osdf.dist, dtype=np.float64).reshape(osdf.grid)
        self.origin = np.array(osdf.c.origin[:])
        self.min_range = np.array(osdf.c.min_range[:])
        self.max_range = np.array(osdf.c.max_range[:])
        self.res = float(osdf.c.resolution)
        self.res_inv = float(osdf.c.resolution_inv)
        # the launcher's grid-dependent parts of the two allowances (csrc/gtop_certify.hip), same operations
        coord = 0.0
        for k in range(3):
            coord = max(coord, abs(self.origin[k]), abs(self.min_range[k]), abs(self.max_range[k]))
        coord = coord + (int(self.n.max()) + 2) * self.res
        self.kappa = KAPPA * (8.0 + coord * self.res_inv)
        self.e_map = SLACK * coord

    def out_of_map(self, pts):
        return np.any((pts < self.min_range + 1e-4) | (pts > self.max_range - 1e-4), axis=-1)

    def cell(self, x):
        """The lookup's cell of coordinates x (..., 3): floor((x - res/2 - origin) / res), and the quotient."""
        q = ((x - 0.5 * self.res) - self.origin) * self.res_inv
        return np.floor(q).astype(np.int64), q

    def corners(self, cell):
        """values[x][y][z] of one cell, each index clamped per axis."""
        i = [np.clip([cell[k], cell[k] + 1], 0, self.n[k] - 1) for k in range(3)]
        return self.val[np.ix_(i[0], i[1], i[2])]

    def midpoint_distance(self, pts):
        none = np.zeros((0, 3))
        return self.osdf.edt_query(pts, -1.0, none, none, none)[0]


def trilinear(diff, v):
    """gtop_edt_trilinear's value (edt_environment.cpp:104-112), unfused."""
    v00 = (1 - diff[0]) * v[0][0][0] + diff[0] * v[1][0][0]
    v01 = (1 - diff[0]) * v[0][0][1] + diff[0] * v[1][0][1]
    v10 = (1 - diff[0]) * v[0][1][0] + diff[0] * v[1][1][0]
    v11 = (1 - diff[0]) * v[0][1][1] + diff[0] * v[1][1][1]
    v0 = (1 - diff[1]) * v00 + diff[1] * v10
    v1 = (1 - diff[1]) * v01 + diff[1] * v11
    return (1 - diff[2]) * v0 + diff[2] * v1


def poly_eval(c, t):
    """poly_eval of csrc/gtop_device_common.h: the dot over descending powers, powers by multiplication."""
    t2 = t * t
    t3 = t2 * t
    t4 = t2 * t2
    t5 = t4 * t
    s = 0.0 * t
    s = s + t5 * c[5]
    s = s + t4 * c[4]
    s = s + t3 * c[3]
    s = s + t2 * c[2]
    s = s + t * c[1]
    s = s + c[0]
    return s


def poly_vel(c, t):
    """poly_vel of csrc/gtop_report_common.h, without its fmas."""
    t2 = t * t
    t3 = t2 * t
    t4 = t2 * t2
    s = (5.0 * c[5]) * t4
    s = (4.0 * c[4]) * t3 + s
    s = (3.0 * c[3]) * t2 + s
    s = (2.0 * c[2]) * t + s
    s = c[1] + s
    return s


def box_lower_bound(field, blo, bhi, mutant=None, mid=None, gaps=None, lower=None):
    """lb of one box [blo, bhi] (3,) each, as the header states it.  mid: the midpoint (for the mid_cell mutant).
    lower(cell, v) -> (the cell's corner values for the forms, those the allowance scales with): the moving boxes'."""
    f = field
    if f.out_of_map(blo) or f.out_of_map(bhi):
        return -np.inf
    i0, q0 = f.cell(blo)
    i1, q1 = f.cell(bhi)
    if gaps is not None:
        for q in (*q0, *q1):
            gaps.append(abs(q - np.rint(q)) / max(abs(q), 1.0))
        for x, lim in ((blo, f.min_range + 1e-4), (bhi, f.max_range - 1e-4)):
            gaps.extend(np.abs(x - lim) / np.maximum(np.abs(lim), 1.0))
    span = i1 - i0
    if np.any(span < 0) or np.any(span > 1):
        return -np.inf
    if mutant == "mid_cell":
        i0 = f.cell(mid)[0]
        span = np.zeros(3, dtype=np.int64)
    vmin, vabs = np.inf, 0.0
    for dx in range(span[0] + 1):
        for dy in range(span[1] + 1):
            for dz in range(span[2] + 1):
                cell = i0 + (dx, dy, dz)
                v = V = f.corners(cell)
                if lower is not None:
                    v, V = lower(cell, v)
                c0 = (cell + 0.5) * f.res + f.origin
                u = [(blo - c0) * f.res_inv, (bhi - c0) * f.res_inv]
                if mutant == "floor":
                    u = [w - np.floor(w) for w in u]
                else:
                    u = [np.minimum(np.maximum(w, 0.0), 1.0) for w in u]
                for e in range(8):
                    o = (e >> 2, (e >> 1) & 1, e & 1)
                    vmin = min(vmin, trilinear([u[o[0]][0], u[o[1]][1], u[o[2]][2]], v))
                vabs = max(vabs, float(np.abs(V).max()))
    lb = vmin - f.kappa * vabs
    return lb if lb == lb else -np.inf


class Node:
    """What the clearance certificate adds to the tree: an interval's midpoint distance and lower bound, a leaf's into lo."""

    def __init__(self, field, margin, mutant):
        self.f, self.margin, self.mutant = field, margin, mutant
        self.lo, self.hi, self.hi_t, self.viol_t = np.inf, np.inf, 0.0, np.inf
        self.hi_at = None          # (segment, local time) of the midpoint behind hi
        self.gaps = []             # relative distances of every decision from a tie
        self.leaves = []           # (segment, a, w, lb, status)

    def segment(self, c, Ts, t_off):
        """Segment coefficients c (3, 6) of duration Ts from trajectory time t_off: its acceleration bound and slack."""
        self.c, self.t_off = c, t_off
        T2 = Ts * Ts
        T3 = T2 * Ts
        q = np.abs(c)
        self.A = 2.0 * q[:, 2] + 6.0 * q[:, 3] * Ts + 12.0 * q[:, 4] * T2 + 20.0 * q[:, 5] * T3
        Pk = ((((q[:, 5] * Ts + q[:, 4]) * Ts + q[:, 3]) * Ts + q[:, 2]) * Ts + q[:, 1]) * Ts + q[:, 0]
        self.E = SLACK * Pk + self.f.e_map

    def midpoints(self, p, t):
        """The distances of the 64 midpoints p at the trajectory times t."""
        return self.f.midpoint_distance(p)

    def lower_bound(self, s, a, w, blo, bhi, mid):
        """lb of the interval [a, a + w] of segment s, whose curve box is [blo, bhi]."""
        return box_lower_bound(self.f, blo, bhi, self.mutant, mid, self.gaps)

    def evaluate(self, L, s, base, w, a):
        h = 0.5 * w
        tc = a + h
        p = np.stack([poly_eval(self.c[k], tc) for k in range(3)], axis=1)
        v = np.stack([poly_vel(self.c[k], tc) for k in range(3)], axis=1)
        if self.mutant == "no_A":
            r = np.abs(v) * h
        else:
            r = np.abs(v) * h + 0.5 * self.A * h * h
        r = r * INFLATE + self.E
        blo, bhi = p - r, p + r
        t = self.t_off + tc
        d = self.midpoints(p, t)
        status, lbs = [], []
        for j in range(64):
            if d[j] < self.hi or (d[j] == self.hi and t[j] < self.hi_t):
                self.hi, self.hi_t, self.hi_at = d[j], t[j], (s, tc[j])
            viol = d[j] < self.margin if self.mutant == "lt" else d[j] <= self.margin
            self.gaps.append(abs(d[j] - self.margin) / max(abs(self.margin), abs(d[j]), 1e-300))
            if viol:
                self.viol_t = min(self.viol_t, t[j])
            lb = self.lower_bound(s, a[j], w, blo[j], bhi[j], p[j])
            if np.isfinite(lb):
                self.gaps.append(abs(lb - self.margin) / max(abs(self.margin), abs(lb), 1e-300))
            lbs.append(lb)
            status.append(VIOLATION if viol else (CERTIFIED if lb > self.margin else OPEN))
        return status, lbs

    def leaf(self, s, a, w, lb, status):
        self.lo = min(self.lo, lb)
        self.leaves.append((s, a, w, lb, status))


def run(node, coeff, T, tree):
    """The tree of every segment of one trajectory, coeff (m, 18), T (m,), with `node`: (cert (8,), info)."""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6)
    T = np.asarray(T, dtype=np.float64)
    t_off = np.float64(0.0)
    for s in range(len(T)):
        node.segment(coeff[s], T[s], t_off)
        walk(node, 0, s, np.float64(0.0), 0.015625 * T[s], tree)
        t_off = t_off + T[s]
    safe, first = verdict(node.viol_t, tree.nund)
    cert = np.array([safe, node.lo, node.hi, node.hi_t, first, tree.nund, tree.nref, t_off])
    return cert, dict(hi_at=node.hi_at, tie=min(node.gaps), leaves=node.leaves)


def certify(field, coeff, T, margin, max_depth=2, max_refine=256, mutant=None):
    """One trajectory's certificate: (cert (8,), info).  coeff (m, 18), T (m,).  info: hi_at = (segment, local time) of
    the midpoint behind hi, tie = the least relative distance of any decision from a tie, leaves."""
    return run(Node(field, np.float64(margin), mutant), coeff, T, Tree(max_depth, max_refine, budget=mutant == "budget"))


def position(coeff, s, t):
    """The point of segment s at local time t, the kernel's bits."""
    c = np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6)[s]
    return np.array([poly_eval(c[k], np.float64(t)) for k in range(3)])


def dense_clearance(field, coeff, T, n=20001):
    """The least of n evenly spaced lookups along the curve (the interpolated distance, -1 out of the map)."""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6)
    T = np.asarray(T, dtype=np.float64)
    ends = np.concatenate([[0.0], np.cumsum(T)])
    t = np.linspace(0.0, ends[-1], n)
    seg = np.minimum(np.searchsorted(ends, t, side="right") - 1, len(T) - 1)
    loc = t - ends[seg]
    pts = np.empty((n, 3))
    for s in range(len(T)):
        rows = seg == s
        for k in range(3):
            pts[rows, k] = poly_eval(coeff[s, k], loc[rows])
    return float(field.midpoint_distance(pts).min()), pts


# ---- the fields and trajectories the tests share ------------------------------------------------------------------
GRID, RES = (24, 20, 16), 0.2
FIELDS = ("esdf", "window", "signed", "random")


def make_field(oracle_mod, kind, seed=5):
    """(Field, MapSpec) on the 24 x 20 x 16 map at 0.2 m: an exact ESDF, a windowed one (10000 outside the window), a
    signed one (negative inside obstacles, to -0.6), uniform random values in [-0.5, 2]."""
    from grad_traj_optimization_amd import problem
    mp = problem.make_map(GRID, RES, density=0.04, seed=seed, box_vox=(2, 5))
    osdf = oracle_mod.Sdf.from_map_size(mp.origin, RES, mp.map_size)
    pts = mp.obstacle_points()
    if kind == "esdf":
        osdf.build_from_points(pts)
    elif kind == "window":
        occ = np.zeros(osdf.dist.size)
        lo, hi = mp.origin + (0.9, 0.7, 0.3), mp.origin + (3.9, 3.3, 2.9)
        inside = np.all((pts > lo) & (pts < hi), axis=1)
        osdf.update_window(occ, lo, hi, pts[inside])
        assert (osdf.dist == 10000.0).any() and (osdf.dist < 10000.0).any()
    elif kind == "signed":
        occ = osdf.build_from_points(pts).copy()
        free = osdf.dist.copy()
        osdf.build_from_occupancy(1.0 - occ)
        depth = np.maximum(-0.6, RES - osdf.dist)
        osdf.dist[:] = np.where(occ > 0, depth, free)
        assert (osdf.dist < 0).any()
    elif kind == "random":
        osdf.dist[:] = np.random.default_rng(seed).uniform(-0.5, 2.0, osdf.dist.size)
    else:
        raise ValueError(kind)
    return Field(osdf), mp


def make_rows(oracle_mod, mp, B, m, seed):
    """(coeff (B, m, 18), T (B, m), Batch): the generator's random-walk rows through the oracle's coefficients."""
    from grad_traj_optimization_amd import problem
    b = problem.make_trajectories(B, m, mp, seed=seed, step_len=(0.6, 1.2), margin=0.5)
    coeff = np.stack([oracle_mod.coefficients(b.T[i], b.Df[i], b.x[i]) for i in range(B)])
    return coeff, b.T.copy(), b


# name: (field kind, m, rows, seed, margin, max_depth, max_refine)
CASES = {
    "esdf_m3": ("esdf", 3, 3, 11, 0.2795, 2, 256),
    "esdf_m7": ("esdf", 7, 2, 12, 0.2, 2, 64),
    "window_m2": ("window", 2, 3, 13, 0.15, 2, 128),
    "signed_m3": ("signed", 3, 2, 14, 0.8, 1, 1),
    "random_m2": ("random", 2, 2, 15, 0.3, 1, 24),
}


def wall_case(oracle_mod):
    """The tunnelling case: a one-voxel wall across x = 0 in an otherwise empty 24 x 20 x 16 map, crossed by a
    two-segment row at about 3.3 m/s.  The wall's field is below 0.1 m over a slab about 0.2 m thick: 0.06 s of
    flight, between the samples at 0.3 and 0.6 s of a report at dt_sample = 0.3.
    -> (Field, MapSpec, coeff (1, 2, 18), T (1, 2), Batch, margin, dt_sample)"""
    from grad_traj_optimization_amd import problem
    occ = np.zeros(GRID, dtype=np.uint8)
    occ[12, :, :] = 1
    mp = problem.MapSpec(GRID, RES, np.array([-2.4, -2.0, 0.0]), occ)
    osdf = oracle_mod.Sdf.from_map_size(mp.origin, RES, mp.map_size)
    osdf.build_from_points(mp.obstacle_points())
    wp = np.array([[[-1.63, 0.13, 1.57], [0.21, 0.11, 1.61], [1.71, 0.17, 1.53]]])
    T = np.array([[0.56, 0.46]])
    Df, Dp = problem.initial_derivatives(wp, start_vel=[[3.3, 0.0, 0.0]], end_vel=[[3.3, 0.0, 0.0]])
    x = Dp.reshape(1, -1).copy()
    x[0, 1] = 3.3                       # the interior waypoint's x velocity: a steady crossing
    b = problem.Batch(wp, T, Df, x, 2)
    coeff = np.stack([oracle_mod.coefficients(T[0], Df[0], x[0])])
    return Field(osdf), mp, coeff, T, b, 0.1, 0.3


def crossing(field, coeff, T, margin, n=20001):
    """(first, last) trajectory time at which a dense scan of the curve finds distance <= margin."""
    _, pts = dense_clearance(field, coeff, T, n)
    d = field.midpoint_distance(pts)
    t = np.linspace(0.0, float(np.sum(T)), n)
    hit = np.flatnonzero(d <= margin)
    return (t[hit[0]], t[hit[-1]]) if len(hit) else None
