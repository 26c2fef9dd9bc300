"""The inputs of tests/test_gpu_post.py, built once here so that tests/test_post_twin.py runs the twin, the oracle and
the mutants on exactly the same numbers (numpy only, fixed seeds)."""
import numpy as np

DT_BIN = 2.0 ** -6
DT = 0.01


# ---- segment probe: discontinuous pieces, x = the segment's index, y = the local time, z = a quintic of its own ----
def probe_coeff(m, seed=0):
    rng = np.random.default_rng(9000 + seed)
    c = np.zeros((m, 18))
    c[:, 0] = np.arange(m)                       # x(t) = s: poly_eval returns it exactly
    c[:, 7] = 1.0                                # y(t) = t: exactly the local time
    c[:, 12:18] = rng.normal(0.0, 1.0, (m, 6)) * np.array([3.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    return c


PROBE_BIN_STEPS = (4, 1, 9, 16, 1, 2, 30, 7)     # segment times in units of DT_BIN: 70 steps, 71 samples


def probe(family):
    """(T (m,), dt, coeff (m, 18)) of a probe family: 'binary' (samples exactly on boundaries), 'decimal' (the
    accumulated rounding decides), 'short' (segments shorter than dt)."""
    if family == "binary":
        T, dt = np.array(PROBE_BIN_STEPS, dtype=np.float64) * DT_BIN, DT_BIN
    elif family == "decimal":
        T, dt = np.array([0.1, 0.3, 0.7, 0.2, 0.6, 0.05, 0.15, 0.03]), DT
    elif family == "short":
        T, dt = np.array([0.03, 0.004, 0.003, 0.02, 0.001, 0.001, 0.001, 0.05, 0.0005, 0.012, 0.03, 0.002]), DT
    else:
        raise KeyError(family)
    return T, dt, probe_coeff(len(T), seed=len(T))


PROBES = ("binary", "decimal", "short")


# ---- chunk edges of the 64-lane sample walk ----
CHUNK_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 257)


def chunk_caps(n):
    return sorted({c for c in (1, 63, 64, 65, n - 1, n, n + 1) if c >= 1})


def chunk_case(n):
    """(T (3,), dt, coeff (3, 18)) with exactly n samples: time_sum lies half a step past sample n - 1.  Arbitrary
    (discontinuous) coefficients: the point carried from one chunk to the next is far from its neighbours."""
    rng = np.random.default_rng(100 + n)
    ts = (n - 1) * DT + 0.5 * DT
    T = np.array([0.5, 0.3, 0.2]) * ts
    coeff = rng.normal(0.0, 1.0, (3, 18)) * np.tile([5.0, 2.0, 2.0, 2.0, 2.0, 2.0], 3)
    return T, DT, coeff


# ---- segment counts: the passes of the per-segment loop ----
SEGMENT_COUNTS = (1, 2, 63, 64, 65, 128, 130, 227)
BIG_V, BIG_A = 4000.0, 4000.0


def arrangements(m):
    """[(segment of the largest velocity, segment of the largest acceleration)]: the velocity in segment 0, in the last
    segment, and between them in segment 64 (the first lane of the second pass; m > 65), in segment 63 (the last lane
    of the first pass; m = 64, where it is the last segment, and m = 65) or in the middle of a shorter trajectory; the
    acceleration elsewhere (m >= 2).  Duplicates are dropped: one arrangement for m = 1, two for m = 2 and m = 64."""
    mid = 64 if m > 65 else 63 if m > 63 else m // 2
    out = []
    for a in (0, mid, m - 1):
        pair = (a, (a + max(1, m // 3)) % m)
        if pair not in out:
            out.append(pair)
    return out


def segment_case(m, seg_v, seg_a):
    """(T (m,), dt, coeff (m, 18)): every segment at its own scale, T between 0.6 and 2.4 steps long (1 to 3 counted
    steps each, at most ~350 samples), the largest end-time velocity in seg_v, the largest acceleration in seg_a."""
    rng = np.random.default_rng(500 + m)
    T = DT * (0.6 + 1.8 * rng.random(m))
    scale = 0.5 + rng.permutation(m) / m
    coeff = rng.normal(0.0, 1.0, (m, 18)) * scale[:, None]
    coeff[seg_v, 1] = BIG_V                      # c1 of x: velocity only
    coeff[seg_a, 8] = BIG_A                      # c2 of y: acceleration 2 c2, velocity 2 c2 T << BIG_V
    return T, DT, coeff


# ---- batch structure ----
BATCHES = (1, 3, 1025)
BATCH_M = 3


def batch_case(B, shared_times=False):
    """(T (B, m) or (m,), dt, coeff (B, m, 18)), every row different; every seventh row is eight times as long (more
    than one 64-sample chunk) when the times are per row."""
    rng = np.random.default_rng(700 + B)
    coeff = rng.normal(0.0, 1.0, (B, BATCH_M, 18)) * (1.0 + np.arange(B)[:, None, None] / B)
    if shared_times:
        return np.array([0.31, 0.07, 0.42]), DT, coeff
    T = rng.uniform(0.01, 0.06, (B, BATCH_M))
    T[::7] *= 8.0
    return T, DT, coeff


# ---- coefficients ----
COEF_T = (0.05, 0.3, 1.0, 7.0, 20.0)
COEF_M = (2, 6, 13)
COEF_B = 5


def coef_case(m, shared_times):
    """(T (B, m) or (m,), Df (B, 18), x (B, 9(m-1))): way-points 10^3 from the origin (pT - p0 - v0 T - a0 T^2 / 2
    cancels), non-zero boundary velocity / acceleration, every T of COEF_T in every case."""
    rng = np.random.default_rng(300 + 10 * m + int(shared_times))
    tset = np.array(COEF_T)
    T = np.stack([tset[(np.arange(m) + b) % len(tset)] for b in range(COEF_B)])
    if m < len(tset):                            # two segments hold two times per row: the rows cover the set
        assert set(T.reshape(-1)) == set(tset)
    if shared_times:
        T = T[0].copy() if m >= len(tset) else np.array([0.05, 20.0])
    Df = np.empty((COEF_B, 3, 6))
    Df[:, :, (0, 3)] = 1000.0 + rng.normal(0.0, 3.0, (COEF_B, 3, 2))
    Df[:, :, (1, 4)] = rng.normal(0.0, 1.0, (COEF_B, 3, 2))
    Df[:, :, (2, 5)] = rng.normal(0.0, 2.0, (COEF_B, 3, 2))
    x = np.empty((COEF_B, 3, m - 1, 3))
    x[..., 0] = 1000.0 + rng.normal(0.0, 3.0, (COEF_B, 3, m - 1))
    x[..., 1] = rng.normal(0.0, 1.0, (COEF_B, 3, m - 1))
    x[..., 2] = rng.normal(0.0, 2.0, (COEF_B, 3, m - 1))
    return T, Df.reshape(COEF_B, 18), x.reshape(COEF_B, 9 * (m - 1))


# ---- grid-stride loops: more elements than the 1024 x 256 lanes of one pass ----
LANES = 1024 * 256
GRID_B = 700
GRID_SETUP_M, GRID_COEF_M = 40, 130


def grid_setup_case():
    """Waypoints (700, 41, 3): 700 * (40 + 18 + 9 * 39) = 286 300 outputs."""
    assert GRID_B * (GRID_SETUP_M + 18 + 9 * (GRID_SETUP_M - 1)) > LANES
    rng = np.random.default_rng(41)
    return np.cumsum(rng.uniform(-1.0, 1.0, (GRID_B, GRID_SETUP_M + 1, 3)), axis=1)


def grid_coef_case():
    """(T (130,), Df (700, 18), x (700, 9 * 129)): 700 * 130 * 3 = 273 000 elements.  Times and derivatives are short
    binary fractions, which keeps the exact solves cheap; the test is about the indexing of the second pass."""
    assert GRID_B * GRID_COEF_M * 3 > LANES
    rng = np.random.default_rng(130)
    T = (4.0 + np.arange(GRID_COEF_M) % 29) / 16.0
    Df = np.round(rng.normal(0.0, 2.0, (GRID_B, 18)) * 256.0) / 256.0
    x = np.round(rng.normal(0.0, 2.0, (GRID_B, 9 * (GRID_COEF_M - 1))) * 256.0) / 256.0
    return T, Df, x
