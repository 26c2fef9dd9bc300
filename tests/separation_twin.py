"""The numpy twin of include/gtop_separation.h: the pairwise separation figures and the selection of distinct
candidates, operation by operation.  Every product and every sum is a numpy operation of its own (one rounding each),
min and max are exact, and np.sqrt closes each figure — so the device's outputs are these bits.

A `mutant` names one deliberate mistake (tests/test_separation_twin.py kills each of them):
  "first_dropped"  the first grid sample is left out
  "strict_end"     `<` in place of `<=` in the flown test
  "always_clamp"   the clamp of hold_ends = 1 applied when hold_ends = 0 too
  "max_for_min"    the greatest distance written as pair_min
  "highest_tie"    the highest index in place of the lowest on a tie (row summary and selection)"""
import numpy as np

MUTANTS = ("first_dropped", "strict_end", "always_clamp", "max_for_min", "highest_tie")
SEP_ROW = 6


def start_times(t0, B):
    """The rules of gtop_set_start_times: None -> 0, one value -> shared, else one per row."""
    if t0 is None:
        return np.zeros(B)
    t0 = np.atleast_1d(np.asarray(t0, dtype=np.float64)).reshape(-1)
    if t0.shape[0] == 1:
        return np.full(B, t0[0])
    assert t0.shape[0] == B, "a start-time count that is not 0, 1 or B"
    return t0.copy()


def grid_times(t_lo, dt, n):
    return np.float64(t_lo) + np.arange(n).astype(np.float64) * np.float64(dt)    # the product rounded, then the sum


def poly_eval(c, t):
    """sum_j c[..., j] t^j as the library's every sample forms it: the powers by multiplication, the terms from the
    highest power down onto 0."""
    t2 = t * t
    t3 = t2 * t
    t4 = t2 * t2
    t5 = t4 * t
    s = 0.0 + t5 * c[..., 5]
    s = s + t4 * c[..., 4]
    s = s + t3 * c[..., 3]
    s = s + t2 * c[..., 2]
    s = s + t * c[..., 1]
    return s + c[..., 0]


def sample_rows(coeff, T, t0, t_lo, dt, n, hold_ends, mutant=None):
    """(positions (B, n, 3), flown (B, n) bool, tau (n,)) of rows coeff (B, m, 18), T (B, m) or (m,)."""
    coeff = np.asarray(coeff, dtype=np.float64)
    B, m = coeff.shape[:2]
    T = np.asarray(T, dtype=np.float64)
    T = np.broadcast_to(T, (B, m))
    start = start_times(t0, B)
    tau = grid_times(t_lo, dt, n)
    pos = np.full((B, n, 3), np.nan)
    flown = np.zeros((B, n), dtype=bool)
    for b in range(B):
        time_sum = 0.0
        for s in range(m):
            time_sum = time_sum + float(T[b, s])
        u = tau - start[b]
        if mutant == "strict_end":
            fl = (u >= 0.0) & (u < time_sum)
        else:
            fl = (u >= 0.0) & (u <= time_sum)
        if hold_ends or mutant == "always_clamp":
            u = np.where(u < 0.0, 0.0, np.where(u > time_sum, time_sum, u))
            fl = np.ones(n, dtype=bool)
        if mutant == "first_dropped":
            fl[0] = False
        # the segment walk: while s < m - 1 and T_s <= t: t -= T_s, ++s
        idx = np.zeros(n, dtype=np.int64)
        t = u.copy()
        for s in range(m - 1):
            go = (idx == s) & (T[b, s] <= t)
            t = np.where(go, t - T[b, s], t)
            idx = idx + go
        seg = coeff[b, idx].reshape(n, 3, 6)
        p = poly_eval(seg, t[:, None])
        pos[b] = np.where(fl[:, None], p, np.nan)
        flown[b] = fl
    return pos, flown, tau


def separation(coeff, T, t0, t_lo, dt, n, hold_ends=False, radius=0.0, mutant=None):
    """(pair_min (B, B), pair_max (B, B), rows (B, 6)) as include/gtop_separation.h defines them."""
    pos, flown, tau = sample_rows(coeff, T, t0, t_lo, dt, n, hold_ends, mutant)
    B = pos.shape[0]
    pair_min = np.full((B, B), np.inf)
    pair_max = np.full((B, B), -np.inf)
    rows = np.zeros((B, SEP_ROW))
    with np.errstate(invalid="ignore"):
        for i in range(B):
            d = pos[i][None] - pos                                     # (B, n, 3)
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            common = flown[i][None] & flown
            common[i] = False                                          # the diagonal
            lo2 = np.where(common, d2, np.inf).min(axis=1)
            hi2 = np.where(common, d2, -np.inf).max(axis=1)
            has = common.any(axis=1)
            pair_min[i] = np.where(has, np.sqrt(hi2 if mutant == "max_for_min" else lo2), np.inf)
            pair_max[i] = np.where(has, np.sqrt(np.where(has, hi2, 0.0)), -np.inf)
            least = pair_min[i].min() if B else np.inf
            r = rows[i]
            r[0] = least
            if np.isinf(least):
                r[1], r[2] = -1.0, -1.0
            else:
                ties = np.flatnonzero(pair_min[i] == least)
                j = int(ties[-1] if mutant == "highest_tie" else ties[0])
                r[1] = j
                k = np.flatnonzero(common[j] & (d2[j] == lo2[j]))
                r[2] = tau[k[0]] if len(k) else -1.0
            r[3] = np.count_nonzero(pair_min[i] < radius) if radius > 0.0 else 0
            r[4] = np.count_nonzero(has)
            r[5] = np.count_nonzero(flown[i])
    return pair_min, pair_max, rows


def select_distinct(passed, cost, pair_max, min_gap, K, mutant=None):
    """(chosen (K,) int32, count) by the greedy rule of gtop_select_distinct_device."""
    cost = np.asarray(cost, dtype=np.float64)
    B = cost.shape[0]
    alive = np.isfinite(cost) if passed is None else (np.asarray(passed) != 0) & np.isfinite(cost)
    alive = alive.copy()
    chosen = np.full(K, -1, dtype=np.int32)
    count = 0
    while count < K and alive.any():
        idx = np.flatnonzero(alive)
        ties = idx[cost[idx] == cost[idx].min()]
        p = int(ties[-1] if mutant == "highest_tie" else ties[0])
        chosen[count] = p
        count += 1
        alive[p] = False
        with np.errstate(invalid="ignore"):
            alive &= np.asarray(pair_max)[:, p] >= min_gap             # a NaN or -inf entry fails
    assert B or count == 0
    return chosen, count


def selection_faults(passed, cost, pair_max, min_gap, K, chosen, count):
    """What is wrong with a selection (from the twin or the device), by the rule's own statement and without the
    greedy loop: [] when each choice is correct, the run is complete and the fill is -1."""
    cost, pair_max = np.asarray(cost, dtype=np.float64), np.asarray(pair_max)
    chosen = [int(c) for c in chosen]
    B = cost.shape[0]
    eligible = np.isfinite(cost) if passed is None else (np.asarray(passed) != 0) & np.isfinite(cost)
    faults = []
    if not (0 <= count <= K and len(chosen) == K and all(c == -1 for c in chosen[count:])):
        return ["count or fill"]

    def qualifies(r, before):
        with np.errstate(invalid="ignore"):
            return bool(eligible[r]) and r not in before and all(pair_max[r, c] >= min_gap for c in before)

    for t in range(count):
        p, before = chosen[t], chosen[:t]
        if not (0 <= p < B and qualifies(p, before)):
            faults.append(f"choice {t} = {p} does not qualify")
            continue
        better = [r for r in range(B) if qualifies(r, before) and (cost[r] < cost[p] or (cost[r] == cost[p] and r < p))]
        if better:
            faults.append(f"choice {t} = {p}: row {better[0]} is cheaper or earlier")
    if count < K and any(qualifies(r, chosen[:count]) for r in range(B)):
        faults.append("stopped while a row still qualifies")
    if eligible.any():
        idx = np.flatnonzero(eligible)
        if count == 0 or chosen[0] != int(idx[np.argmin(cost[idx])]):      # (argmin keeps the first of equal costs)
            faults.append("chosen[0] is not the cheapest eligible row")
    return faults


# ---- inputs ----
def random_rows(B, m, seed, shared_T=False):
    """(coeff (B, m, 18), T (B, m) or (m,)): random quintics of a few metres, segment times in [0.4, 1.1].  The rows
    are not continuous curves: the figures are defined for any coefficient rows."""
    rng = np.random.default_rng(seed)
    coeff = rng.uniform(-1.0, 1.0, (B, m, 18)) * np.tile([3.0, 2.0, 1.0, 0.5, 0.25, 0.125], 3)
    T = rng.uniform(0.4, 1.1, (m,) if shared_T else (B, m))
    return coeff, T


def known_rows():
    """Three rows of two 2-second segments in dyadic numbers: row 0 is x = t; row 1 is x = 4 - t, y = 0.5 (each
    segment in its local time); row 2 stands at (8, 8, 8).  T is shared."""
    c = np.zeros((3, 2, 18))
    c[0, 0, 1] = 1.0                      # x = t
    c[0, 1, 0], c[0, 1, 1] = 2.0, 1.0     # x = 2 + t'
    c[1, 0, 0], c[1, 0, 1] = 4.0, -1.0    # x = 4 - t
    c[1, 1, 0], c[1, 1, 1] = 2.0, -1.0    # x = 2 - t'
    c[1, :, 6] = 0.5                      # y = 0.5
    c[2, :, 0] = c[2, :, 6] = c[2, :, 12] = 8.0
    return c, np.array([2.0, 2.0])
