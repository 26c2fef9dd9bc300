"""The per-segment report and the segment-time reallocation (include/gtop.h: gtop_validate_segments*,
gtop_reallocate_times*) restated in numpy, independently of the library.

reduce_segments reduces per-sample data — the sample's time, segment, distance, out-of-map flag, velocity and
acceleration, as tests/validate_twin.py produces them — to the B x m x 10 rows.  retime_length and retime_limits are the
two modes of the reallocation in plain numpy float64 operations, one rounded IEEE operation per step and nothing fused,
so that the device kernel (csrc/gtop_retime.hip, compiled unfused) reproduces their bits.

`mutant` switches on ONE deliberate mistake; tests/test_segments_twin.py shows that the checks catch each of them."""
import numpy as np

N_SEG = 10
EMPTY_ROW = np.array([0.0, -1.0, np.inf, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
MUTANTS = ("strict_margin", "init_time_first_only", "rho_min", "no_sqrt_acc", "boundary_to_earlier")


def segment_of_samples(T, dt=0.01, mutant=None):
    """(eval_t (N,), segment (N,)) of every getTraj sample: validate_twin.sample_times' walk restated (mutant
    boundary_to_earlier: a sample exactly on a segment boundary stays in the earlier segment)."""
    T = np.asarray(T, dtype=np.float64)
    time_sum = np.float64(0.0)
    for s in range(len(T)):
        time_sum = time_sum + T[s]
    dt = np.float64(dt)
    ts, segs = [], []
    t = np.float64(0.0)
    while t <= time_sum:
        u, idx = t, 0
        while idx < len(T) - 1 and (T[idx] < u if mutant == "boundary_to_earlier" else T[idx] <= u):
            u = u - T[idx]
            idx += 1
        ts.append(t)
        segs.append(idx)
        t = t + dt
    return np.array(ts), np.array(segs, dtype=np.int64)


def reduce_segments(m, t, seg, dist, oom, v, a, margin, mutant=None):
    """(m, 10): the rows of one trajectory from its per-sample quantities (dist already -1 where out of the map)."""
    t, seg, dist = np.asarray(t, dtype=np.float64), np.asarray(seg), np.asarray(dist, dtype=np.float64)
    oom, v, a = np.asarray(oom, dtype=bool), np.asarray(v, dtype=np.float64), np.asarray(a, dtype=np.float64)
    out = np.tile(EMPTY_ROW, (m, 1))
    for s in range(m):
        k = np.flatnonzero(seg == s)
        if k.size == 0:
            continue
        r = out[s]
        r[0], r[1] = k.size, k[0]
        d = dist[k]
        comparable = d < np.inf                     # (a NaN or +inf distance never becomes a clearance)
        if comparable.any():
            i = int(np.argmin(np.where(comparable, d, np.inf)))      # the first of equal minima
            r[2], r[3] = d[i], t[k[i]]
        r[4] = np.count_nonzero(d < margin if mutant == "strict_margin" else d <= margin)
        r[5] = np.count_nonzero(oom[k])
        r[6] = np.sqrt((v[k] ** 2).sum(axis=1).max())
        r[7] = np.sqrt((a[k] ** 2).sum(axis=1).max())
        r[8] = np.abs(v[k]).max()
        r[9] = np.abs(a[k]).max()
    return out


def check_laws(S, R):
    """The identities include/gtop.h states between one trajectory's segment rows S (m, 10) and its whole report
    R (12,): a list of the names of those that FAIL (empty = all hold)."""
    S, R = np.asarray(S, dtype=np.float64), np.asarray(R, dtype=np.float64)
    bad = []
    if S[:, 0].sum() != R[0]:
        bad.append("sum of counts")
    full = np.flatnonzero(S[:, 0] > 0)
    if full.size == 0 or S[full[0], 1] != 0 or np.any(S[full[1:], 1] != S[full[:-1], 1] + S[full[:-1], 0]):
        bad.append("first samples advance by the counts")
    empty = S[:, 0] == 0
    if np.any(S[empty] != EMPTY_ROW):
        bad.append("rows of segments without samples")
    if S[:, 2].min() != R[1]:
        bad.append("clearance")
    else:
        s = int(np.argmin(S[:, 2]))                 # the earliest segment attaining it
        if np.isfinite(R[1]) and not (S[s, 3] == R[2] and S[s, 1] <= R[3] < S[s, 1] + S[s, 0]):
            bad.append("clearance time and sample")
    if S[:, 4].sum() != R[4]:
        bad.append("samples below the margin")
    if S[:, 5].sum() != R[6]:
        bad.append("samples out of the map")
    if np.any(S[:, 6:10].max(axis=0) != R[7:11]):
        bad.append("velocity and acceleration maxima")
    return bad


# ---- segment-time reallocation ----
def positions(m, x, Df):
    """(m + 1, 3): the waypoint positions as they stand in one row's x (9 (m - 1),) and Df (18,)."""
    x, Df = np.asarray(x, dtype=np.float64).reshape(3, 3 * m - 3), np.asarray(Df, dtype=np.float64).reshape(3, 6)
    p = np.empty((m + 1, 3))
    p[0], p[m] = Df[:, 0], Df[:, 3]
    for k in range(1, m):
        p[k] = x[:, 3 * (k - 1)]
    return p


def retime_length(m, x, Df, mean_v, init_time, mutant=None):
    """LENGTH for one row: (m,) times.  sqrt(dx*dx + dy*dy + dz*dz) / mean_v, init_time on the first and the last
    segment (the reference's commented block, src/grad_traj_optimizer.cpp:209-227)."""
    p = positions(m, x, Df)
    mean_v, init_time = np.float64(mean_v), np.float64(init_time)
    T = np.empty(m)
    for i in range(m):
        dx, dy, dz = (np.float64(p[i, k] - p[i + 1, k]) for k in range(3))
        length = np.sqrt((dx * dx + dy * dy) + dz * dz)
        ends = i == 0 or (i == m - 1 and mutant != "init_time_first_only")
        T[i] = length / mean_v + init_time if ends else length / mean_v
    return T


def retime_limits(m, x, T, seg, max_vel=0.0, max_acc=0.0, per_axis=False, uniform=False, scale_x=False,
                  max_ratio=4.0, mutant=None):
    """LIMITS for one row: (T_out (m,), x_out).  seg: the row's (m, 10) segment report."""
    T, seg = np.asarray(T, dtype=np.float64), np.asarray(seg, dtype=np.float64)
    V, A = (seg[:, 8], seg[:, 9]) if per_axis else (seg[:, 6], seg[:, 7])
    ratio = np.empty(m)
    for s in range(m):
        rv = V[s] / np.float64(max_vel) if max_vel > 0 else np.float64(0.0)
        if max_acc > 0:
            q = A[s] / np.float64(max_acc)
            ra = q if mutant == "no_sqrt_acc" else np.sqrt(q)
        else:
            ra = np.float64(0.0)
        ratio[s] = np.fmin(np.fmax(np.fmax(rv, ra), np.float64(1.0)), np.float64(max_ratio))
    if uniform:
        ratio[:] = ratio.max()
    T_out = ratio * T
    x_out = np.array(x, dtype=np.float64).reshape(3, 3 * m - 3).copy()
    if scale_x:
        for k in range(1, m):
            rho = (np.fmin if mutant == "rho_min" else np.fmax)(ratio[k - 1], ratio[k])
            x_out[:, 3 * (k - 1) + 1] = x_out[:, 3 * (k - 1) + 1] / rho
            x_out[:, 3 * (k - 1) + 2] = x_out[:, 3 * (k - 1) + 2] / (rho * rho)
    return T_out, x_out.reshape(-1)


def acc_bound(coeff, T):
    """A-bar of one trajectory: an upper bound of |a_k(t)| over the whole curve from its coefficients (m, 18),
    sum_j |j (j-1) c_j| T_s^(j-2), the largest over segments and axes."""
    c = np.abs(np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6))
    T = np.asarray(T, dtype=np.float64)
    j = np.arange(2, 6)
    return float(((j * (j - 1))[None, None, :] * c[:, :, 2:] * T[:, None, None] ** (j - 2)[None, None, :]).sum(axis=2).max())


def vel_bound(coeff, T):
    """V-bar: the same for |v_k(t)|, sum_j |j c_j| T_s^(j-1)."""
    c = np.abs(np.asarray(coeff, dtype=np.float64).reshape(-1, 3, 6))
    T = np.asarray(T, dtype=np.float64)
    j = np.arange(1, 6)
    return float((j[None, None, :] * c[:, :, 1:] * T[:, None, None] ** (j - 1)[None, None, :]).sum(axis=2).max())
