"""The moving-obstacle cost restated independently of the library: oracle/np_twin.py's cost_grad loop — the reference's
callback, src/grad_traj_optimizer.cpp:281-432 — with the lookup of each collision sample (:363) replaced by the C
oracle's already-tested EDTEnvironment::evaluateEDTWithGrad (oracle.Sdf.edt_query) at the sample's absolute time

    tau = ((t0 + T[0]) + ... + T[s-1]) + t,     t the sample's local time (:353), fp64, summed left to right.

np_twin.cost_grad asks a duck-typed `sdf.query(pos)` once per sample in (segment, sample) order, so the lookup is a thin
object that walks the precomputed tau list.  Besides cost and gradient it reports, per sample, the base voxel index of
the interpolation and whether a box lowered any of the 8 corner values (what the tests condition on)."""
import numpy as np

from oracle import np_twin


def sample_times(T, t0=0.0):
    """tau of every collision sample, in the callback's (segment, sample) order; the local times replay :351-:353
    (dt = T/30, t = 1e-3, t += dt while t < T)."""
    T = np.asarray(T, dtype=np.float64)
    taus = []
    start = np.float64(t0)
    for s in range(len(T)):
        dt = T[s] / 30.0
        t = 1e-3
        while t < T[s]:
            taus.append(start + t)
            t += dt
        start = start + T[s]
    return np.array(taus)


def box_distance(points, tau, p0, vel, scale):
    """minDistToAllBox (src/edt_environment.cpp:26-73) at `points` (..., 3): per axis 0 inside the slab, else the distance
    to the nearer face; 1e7 without boxes."""
    points = np.asarray(points, dtype=np.float64)
    best = np.full(points.shape[:-1], 10000000.0)
    for b in range(len(p0)):
        c = p0[b] + vel[b] * tau
        bmax, bmin = c + 0.5 * scale[b], c - 0.5 * scale[b]
        inside = (points >= bmin) & (points <= bmax)
        d1 = np.where(inside, 0.0, np.minimum(np.abs(points - bmin), np.abs(points - bmax)))
        d = np.sqrt(d1[..., 0] * d1[..., 0] + d1[..., 1] * d1[..., 1] + d1[..., 2] * d1[..., 2])
        best = np.minimum(best, d)
    return best


class TimedLookup:
    """sdf.query(pos) for np_twin.cost_grad: evaluateEDTWithGrad(pos, tau_k) for the k-th call."""

    def __init__(self, osdf, taus, p0, vel, scale, map_min=None, map_max=None):
        self.osdf, self.taus = osdf, taus
        self.p0, self.vel, self.scale = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in (p0, vel, scale))
        self.k = 0
        self.base_idx, self.lowered, self.dist = [], [], []
        self.field = osdf.dist.reshape(osdf.grid)
        self.n = np.array(osdf.grid)
        self.map_min = np.array(osdf.c.min_range[:]) if map_min is None else map_min
        self.map_max = np.array(osdf.c.max_range[:]) if map_max is None else map_max

    def query(self, pos):
        tau = self.taus[self.k]
        self.k += 1
        pos = np.asarray(pos, dtype=np.float64)
        d, g = self.osdf.edt_query(pos, tau, self.p0, self.vel, self.scale)
        res, org = self.osdf.resolution, self.osdf.origin
        idx = np.floor((pos - 0.5 * res - org) * (1.0 / res)).astype(np.int64)   # sdf_map.cpp:201-204
        in_map = not (np.any(pos < self.map_min + 1e-4) or np.any(pos > self.map_max - 1e-4))
        low = False
        if in_map and tau >= 0.0 and len(self.p0):
            off = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)])
            corners = idx + off
            centres = (corners + 0.5) * res + org
            cl = np.clip(corners, 0, self.n - 1)
            static = self.field[cl[:, 0], cl[:, 1], cl[:, 2]]
            low = bool(np.any(box_distance(centres, tau, self.p0, self.vel, self.scale) < static))
        self.base_idx.append(idx)
        self.lowered.append(low)
        self.dist.append(float(d[0]))
        return float(d[0]), g[0]


def cost_grad(T, Df, x, osdf, p, p0, vel, scale, t0=0.0, gen=None):
    """One callback evaluation with the time-aware lookup.  osdf: oracle.Sdf; p: np_twin's parameter dict; boxes
    {p0, vel, scale} (nbox, 3) each (nbox may be 0); t0: the trajectory's start time on the boxes' clock (negative:
    every sample static only).  Returns cost, grad (9(m-1),) and dict(base_idx (N, 3), lowered (N,), tau (N,),
    dist (N,)) over the N collision samples."""
    taus = sample_times(T, t0)
    look = TimedLookup(osdf, taus, p0, vel, scale)
    cost, grad, _ = np_twin.cost_grad(T, Df, x, look, p, gen=gen)
    assert look.k == len(taus)
    info = dict(base_idx=np.array(look.base_idx).reshape(-1, 3), lowered=np.array(look.lowered, dtype=bool), tau=taus,
                dist=np.array(look.dist))
    return cost, grad, info


def eval_batch(T, Df, x, osdf, p, p0, vel, scale, t0=None):
    """Rows of a batch: T (B, m), Df (B, 3, 6), x (B, n), t0 None / scalar / (B,)."""
    B = x.shape[0]
    t0 = np.broadcast_to(0.0 if t0 is None else np.asarray(t0, dtype=np.float64), (B,))
    cost, grad, infos = np.empty(B), np.empty_like(x), []
    for b in range(B):
        cost[b], grad[b], info = cost_grad(T[b], Df[b], x[b], osdf, p, p0, vel, scale, t0[b])
        infos.append(info)
    return cost, grad, infos


def parked_field(osdf, p0, scale):
    """F' = min(F, distance from each voxel centre to the nearest of the boxes standing still at p0)."""
    n = osdf.grid
    ii = np.stack(np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(n[2]), indexing="ij"), axis=-1)
    centres = (ii + 0.5) * osdf.resolution + osdf.origin
    p0, scale = (np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (p0, scale))
    bd = box_distance(centres, 0.0, p0, np.zeros_like(p0), scale)
    return np.minimum(osdf.dist.reshape(n), bd)
