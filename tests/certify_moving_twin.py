"""The certificate against the moving boxes (include/gtop.h: gtop_certify_moving_device) restated in numpy for ONE
trajectory, on tests/certify_twin.py: its Field, trilinear, poly_eval, its cell and vertex loop and — as a subclass of
its node on the tree of tests/interval_tree_twin.py — its interval evaluation, status rule and output row.  Only what
the header adds is stated here, in plain fp64 operations as the header has them: the range of box time of an interval,
the swept faces of either kind of box, and the lower bound with corner values lowered to the distance to the swept
boxes, V taken from the static values.

Midpoint distances come through the C oracle's evaluateEDTWithGrad (oracle.Sdf.edt_query); a polynomial box is shown to
it as a standing box at the centre gtop_box_polynomial_centres gives for that time.  numpy fuses nothing where the
kernel's shared lookup has fmas (a constant-velocity box's centre, the corner voxel's centre, the squared sum of
gtop_edt_box_min): the places tests/test_gpu_certify_moving.py bounds.

Also here: the box lists and rows the tests share, the moving tunnelling case, and the mutants the tests must catch."""
import numpy as np

from tests import certify_twin as ct

MUTANTS = ("mid_faces", "no_Aq", "tau_a", "no_clamp", "V_after")


class Boxes:
    """A box list of either kind.  Constant velocity: p0, vel, scale (n, 3).  Polynomial: coef (n, 3, 6) in ascending
    powers, scale (n, 3), t_range (n, 2) (None: unbounded)."""

    def __init__(self, poly, scale, p0=None, vel=None, coef=None, t_range=None):
        self.poly = poly
        self.scale = np.asarray(scale, dtype=np.float64).reshape(-1, 3)
        self.n = len(self.scale)
        if poly:
            self.coef = np.asarray(coef, dtype=np.float64).reshape(-1, 3, 6)
            self.t_range = None if t_range is None else np.asarray(t_range, dtype=np.float64).reshape(-1, 2)
            self.t1 = np.full(self.n, -np.inf) if t_range is None else self.t_range[:, 0]
            self.t2 = np.full(self.n, np.inf) if t_range is None else self.t_range[:, 1]
        else:
            self.p0 = np.asarray(p0, dtype=np.float64).reshape(-1, 3)
            self.vel = np.asarray(vel, dtype=np.float64).reshape(-1, 3)

    @classmethod
    def const_vel(cls, p0, vel, scale):
        return cls(False, scale, p0=p0, vel=vel)

    @classmethod
    def polynomial(cls, coef, scale, t_range=None):
        return cls(True, scale, coef=coef, t_range=t_range)

    def set_on(self, ctx):
        """The list into a GtopContext."""
        if self.poly:
            ctx.set_moving_box_polynomials(self.coef, self.scale, self.t_range)
        else:
            ctx.set_moving_boxes(self.p0, self.vel, self.scale)

    def take(self, rows):
        rows = np.atleast_1d(rows)
        if self.poly:
            return Boxes.polynomial(self.coef[rows], self.scale[rows], None if self.t_range is None else self.t_range[rows])
        return Boxes.const_vel(self.p0[rows], self.vel[rows], self.scale[rows])

    def centres_fma(self, tau):
        """(len(tau), n, 3): a polynomial list's centres, the interface's fma Horner after the clamp."""
        from grad_traj_optimization_amd import box_polynomial_centres
        return box_polynomial_centres(self.coef, np.asarray(tau, dtype=np.float64), self.t_range)

    def swept(self, tau_a, tau_b, mutant=None):
        """(smin, smax) (n, 3): faces that contain every box at every box time of [tau_a, tau_b]."""
        if mutant == "mid_faces":
            tau_a = tau_b = 0.5 * (tau_a + tau_b)
        if not self.poly:
            lo, hi = [], []
            for t in (tau_a, tau_b):                      # gtop_edt_box_faces at either end
                c = self.p0 + self.vel * t
                hi.append(c + 0.5 * self.scale)
                lo.append(c - 0.5 * self.scale)
            return np.minimum(lo[0], lo[1]), np.maximum(hi[0], hi[1])
        if mutant == "no_clamp":
            tca, tcb = np.full(self.n, tau_a), np.full(self.n, tau_b)
        else:
            tca = np.minimum(np.maximum(tau_a, self.t1), self.t2)
            tcb = np.minimum(np.maximum(tau_b, self.t1), self.t2)
        with np.errstate(invalid="ignore", over="ignore"):
            hh = 0.5 * (tcb - tca)
            tm = tca + hh
            M = np.maximum(np.abs(tca), np.abs(tcb))[:, None]
            M2 = M * M
            M3 = M2 * M
            c, a = self.coef, np.abs(self.coef)
            if mutant == "no_clamp":                      # (the centre's own clamp would undo the mutation)
                cm = np.stack([Boxes.polynomial(self.coef[q:q + 1], self.scale[q:q + 1]).centres_fma([tm[q]])[0, 0]
                               for q in range(self.n)])
            else:
                cm = np.stack([self.take(q).centres_fma([tm[q]])[0, 0] for q in range(self.n)])
            tm, hh = tm[:, None], hh[:, None]
            vq = ((((5.0 * c[..., 5]) * tm + 4.0 * c[..., 4]) * tm + 3.0 * c[..., 3]) * tm + 2.0 * c[..., 2]) * tm + c[..., 1]
            Aq = 2.0 * a[..., 2] + 6.0 * a[..., 3] * M + 12.0 * a[..., 4] * M2 + 20.0 * a[..., 5] * M3
            Qk = ((((a[..., 5] * M + a[..., 4]) * M + a[..., 3]) * M + a[..., 2]) * M + a[..., 1]) * M + a[..., 0]
            rq = np.abs(vq) * hh if mutant == "no_Aq" else np.abs(vq) * hh + 0.5 * Aq * hh * hh
            rq = rq * ct.INFLATE + ct.SLACK * Qk
            ok = np.isfinite(cm) & np.isfinite(rq)
            half = 0.5 * self.scale
            return np.where(ok, (cm - rq) - half, -np.inf), np.where(ok, (cm + rq) + half, np.inf)


def lookup(field, boxes, pts, tau):
    """The query's `dist` for each (pts[i], tau[i]) against the static field and the boxes (tau < 0: static only),
    through the oracle."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (len(pts),))
    osdf = field.osdf
    if boxes is None or boxes.n == 0:
        return field.midpoint_distance(pts)
    if not boxes.poly:
        return osdf.edt_query(pts, tau, boxes.p0, boxes.vel, boxes.scale)[0]
    centres = boxes.centres_fma(tau)
    still = np.zeros((boxes.n, 3))
    return np.array([osdf.edt_query(pts[i], tau[i], centres[i], still, boxes.scale)[0][0] for i in range(len(pts))])


def box_min(field, cell, values, smin, smax):
    """gtop_edt_box_min without its (exact) skip: values[x][y][z] lowered to the distance from the corner voxel's centre
    to each box [smin[q], smax[q]]; the squares summed x, y, z in that order."""
    f = field
    pt = (np.asarray(cell)[:, None] + np.arange(2)[None, :] + 0.5) * f.res + f.origin[:, None]     # [axis][offset]
    lo, hi = np.asarray(smin)[:, :, None], np.asarray(smax)[:, :, None]
    d1 = np.where((pt >= lo) & (pt <= hi), 0.0, np.minimum(np.abs(pt - lo), np.abs(pt - hi)))     # [box][axis][offset]
    sq = d1 * d1
    d2 = np.sqrt(sq[:, 0, :, None, None] + sq[:, 1, None, :, None] + sq[:, 2, None, None, :])
    return np.minimum(np.asarray(values, dtype=np.float64), d2.min(axis=0))


def moving_lower_bound(field, boxes, blo, bhi, tau_a, tau_b, mutant=None, gaps=None):
    """lb of the curve box [blo, bhi] over the box times [tau_a, tau_b], as the header states it."""
    apply = (tau_a if mutant == "tau_a" else tau_b) >= 0.0
    if apply:
        smin, smax = boxes.swept(tau_a, tau_b, mutant)

    def lower(cell, v):
        low = box_min(field, cell, v, smin, smax) if apply else v
        return low, (low if mutant == "V_after" else v)      # V: of the static values
    return ct.box_lower_bound(field, blo, bhi, gaps=gaps, lower=lower)


class Node(ct.Node):
    """What the boxes add to the clearance node: the row's start time on the boxes' clock, midpoint distances at the
    intervals' box times, and the lower bound over an interval's range of box time."""

    def __init__(self, field, boxes, start, margin, mutant):
        super().__init__(field, margin, None)
        self.boxes, self.start, self.box_mutant = boxes, np.float64(start), mutant
        self.ranges = {}          # (segment, a, w) -> (blo, bhi, tau_a, tau_b)

    def segment(self, c, Ts, t_off):
        super().segment(c, Ts, t_off)
        self.delta = ct.SLACK * (abs(self.start) + (t_off + Ts))

    def midpoints(self, p, t):
        return lookup(self.f, self.boxes, p, self.start + t)

    def lower_bound(self, s, a, w, blo, bhi, mid):
        ta = self.start + (self.t_off + a)
        tb = self.start + (self.t_off + (a + w))
        tau_a, tau_b = ta - self.delta, tb + self.delta
        self.ranges[(s, a, w)] = (blo, bhi, tau_a, tau_b)
        return moving_lower_bound(self.f, self.boxes, blo, bhi, tau_a, tau_b, self.box_mutant, self.gaps)


def certify(field, boxes, coeff, T, t0, margin, max_depth=2, max_refine=256, mutant=None):
    """One trajectory's certificate against the field and the boxes at start time t0: (cert (8,), info) as
    certify_twin.certify gives them; info["ranges"]: (segment, a, w) -> (blo, bhi, tau_a, tau_b) of every interval
    evaluated."""
    if boxes is None or boxes.n == 0:
        return ct.certify(field, coeff, T, margin, max_depth, max_refine)
    node = Node(field, boxes, t0, np.float64(margin), mutant)
    cert, info = ct.run(node, coeff, T, ct.Tree(max_depth, max_refine))
    info["ranges"] = node.ranges
    return cert, info


def dense_lookups(field, boxes, coeff, T, t0, n=20001):
    """(t (n,), d (n,)): the query's distance at n evenly spaced times of the curve, box time t0 + t."""
    coeff =np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6)
    T = np.asarray(T, dtype=np.float64)
    ends = np.concatenate([[0.0], np.cumsum(T)])
    t = np.linspace(0.0, ends[-1], n)
    seg = np.minimum(np.searchsorted(ends, t, side="right") - 1, len(T) - 1)
    loc = t - ends[seg]
    pts = np.stack([np.choose(seg, [ct.poly_eval(coeff[s, k], loc) for s in range(len(T))]) for k in range(3)], axis=1)
    return t, lookup(field, boxes, pts, t0 + t)


def leaf_is_sound(field, boxes, lb, blo, bhi, tau_a, tau_b, n=5):
    """lb is at most the lookups on an n^3 x n grid of (the curve box) x (its range of box time)."""
    g = np.linspace(0.0, 1.0, n)
    w = np.stack(np.meshgrid(g, g, g, g, indexing="ij"), axis=-1).reshape(-1, 4)
    pts = blo + w[:, :3] * (bhi - blo)
    tau = tau_a + w[:, 3] * (tau_b - tau_a)
    return bool(lb <= lookup(field, boxes, pts, tau).min())


# ---- the box lists and rows the tests share --------------------------------------------------------------------
def shared_boxes(mp, poly, t_total=3.0):
    """Three boxes that fly through the 24 x 20 x 16 map of certify_twin.make_field.  Polynomial: one braking (it
    turns round inside the map), one whose t_range ends at 1.1 s — mid-trajectory, after which it stands — and one
    unbounded."""
    o = np.asarray(mp.origin, dtype=np.float64)
    p0 = o + np.array([[0.9, 1.7, 1.4], [3.6, 0.8, 1.8], [2.2, 3.1, 1.1]])
    vel = np.array([[0.9, 0.3, 0.05], [-0.7, 0.6, -0.1], [0.2, -0.8, 0.15]])
    scale = np.array([[0.5, 0.4, 0.6], [0.3, 0.7, 0.5], [0.6, 0.3, 0.4]])
    if not poly:
        return Boxes.const_vel(p0, vel, scale)
    coef = np.zeros((3, 3, 6))
    coef[:, :, 0], coef[:, :, 1] = p0, vel
    coef[0, :, 2] = -0.25 * vel[0]                        # braking: the velocity changes sign at t = 2 s
    coef[1, :, 3] = (0.02, -0.03, 0.01)
    coef[2, :, 2], coef[2, :, 4] = (0.05, 0.02, -0.01), (-0.002, 0.001, 0.0)
    t_range = np.array([[-np.inf, np.inf], [0.0, 1.1], [-np.inf, np.inf]])
    return Boxes.polynomial(coef, scale, t_range)


def tunnel_case(oracle_mod, poly=False, t0=2.0, at_rest=False):
    """The moving tunnelling case: the row of certify_twin.wall_case in the 24 x 20 x 16 map with the single occupied
    column occ[0, 0, :], and a plate of extent (0.4, 0.1, 0.4) that flies along +y at 4 m/s and sits over the curve's
    point of local time 0.45 s at box time t0 + 0.45.  at_rest: the row starts and ends at rest, as the C++ class flies
    every path (the interior waypoint's velocity stays 3.3 m/s); the plate sits over THAT curve's point.
    -> (Field, MapSpec, coeff (1, 2, 18), T (1, 2), Batch, margin, dt_sample, Boxes, t0)"""
    from grad_traj_optimization_amd import problem
    _, _, coeff, T, b, margin, dt = ct.wall_case(oracle_mod)
    if at_rest:
        Df, _ = problem.initial_derivatives(b.waypoints)
        b = problem.Batch(b.waypoints, T, Df, b.x, 2)
        coeff = np.stack([oracle_mod.coefficients(T[0], Df[0], b.x[0])])
    occ = np.zeros(ct.GRID, dtype=np.uint8)
    occ[0, 0, :] = 1
    mp = problem.MapSpec(ct.GRID, ct.RES, np.array([-2.4, -2.0, 0.0]), occ)
    osdf = oracle_mod.Sdf.from_map_size(mp.origin, ct.RES, mp.map_size)
    osdf.build_from_points(mp.obstacle_points())
    vel = np.array([0.0, 4.0, 0.0])
    p0 = ct.position(coeff[0], 0, 0.45) - vel * (t0 + 0.45)
    scale = np.array([0.4, 0.1, 0.4])
    if poly:
        coef = np.zeros((1, 3, 6))
        coef[0, :, 0], coef[0, :, 1] = p0, vel
        boxes = Boxes.polynomial(coef, scale[None])
    else:
        boxes = Boxes.const_vel(p0[None], vel[None], scale[None])
    return ct.Field(osdf), mp, coeff, T, b, margin, dt, boxes, t0


def crossing(field, boxes, coeff, T, t0, margin, n=20001):
    """(first, last, least distance) of a dense scan's times with distance <= margin; None if there are none."""
    t, d = dense_lookups(field, boxes, coeff, T, t0, n)
    hit = np.flatnonzero(d <= margin)
    return (t[hit[0]], t[hit[-1]], float(d.min())) if len(hit) else None
