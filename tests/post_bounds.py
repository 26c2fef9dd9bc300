"""The bounds and comparisons shared by tests/test_gpu_post.py (the kernels) and tests/test_post_twin.py (the oracle,
a plain-float model and its mutants): what is compared with ==, and |got - exact| <= K * u * magnitude for the rest.
Every K is derived, rounding by rounding, in the docstring of tests/test_gpu_post.py; no GPU in here."""
import json
import math
import os

import numpy as np

from tests import post_twin as twin

K_POINT = 16
K_MAX = 12
K_COEF = 256


def K_LENGTH(n, serial=False):
    return 20 + (max(n - 2, 0) if serial else 6 + (n + 63) // 64)


def K_JERK(m, serial=False):
    return 12 + 3 * m if serial else 24


def K_ACC(m, serial=False):
    return 4 + m if serial else 16


def K_MEAN(cmax, num, serial=False):
    return 13 + num if serial else 22 + cmax


def stat_k(name, n, m, cmax, num, serial=False):
    """K of one statistic.  serial = an implementation that adds every sum term by term in sequence (the oracle): the
    summation term of the derivation is then the number of terms instead of the tree's levels plus the passes."""
    return {"length": K_LENGTH(n, serial), "jerk": K_JERK(m, serial), "acc_cost": K_ACC(m, serial), "max_v": K_MAX,
            "max_a": K_MAX, "mean_v": K_MEAN(cmax, num, serial), "mean_a": K_MEAN(cmax, num, serial)}[name]


def log(rec):
    """GTOP_POST_LOG=<file> appends one JSON line per check."""
    path = os.environ.get("GTOP_POST_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# comparisons against the twin
# ---------------------------------------------------------------------------------------------------------------------
def compare_samples(got, smp, cap):
    """got (cap, 3) against the twin's samples(): (largest ratio over the stored points, list of exact violations)."""
    got = np.asarray(got, dtype=np.float64).reshape(cap, 3)
    k = min(smp["n"], cap)
    bad = []
    if not np.all(got[k:] == 0.0):
        bad.append("a value behind min(count, cap)")
    worst = 0.0
    for i in range(k):
        for a in range(3):
            worst = max(worst, twin.ratio(got[i, a], smp["pts"][i][a], smp["mag"][i][a]))
    return worst, bad


def compare_probe(got, smp, cap):
    """The probe's x and y columns: the segment index and the local time of every stored sample, bit for bit."""
    got = np.asarray(got, dtype=np.float64).reshape(cap, 3)
    k = min(smp["n"], cap)
    bad = []
    for i in range(k):
        if got[i, 0] != float(smp["idx"][i]):
            bad.append(f"sample {i}: segment {got[i, 0]:g}, the reference walks to {smp['idx'][i]}")
        if got[i, 1].tobytes() != np.float64(smp["tloc"][i]).tobytes():
            bad.append(f"sample {i}: local time {got[i, 1]!r}, the reference's {smp['tloc'][i]!r}")
    return bad


def compare_stats(got, ref, serial=False):
    """got[9] against the twin's stats(): ({name: (ratio, K)}, list of exact violations)."""
    val, mag, info = ref
    got = np.asarray(got, dtype=np.float64).reshape(9)
    n, m, cmax, num = int(val[8]), len(info["counts"]), max(info["counts"]), info["num"]
    bad = []
    if got[0].tobytes() != np.float64(val[0]).tobytes():
        bad.append(f"time_sum {got[0]!r} != {val[0]!r}")
    if got[8] != val[8]:
        bad.append(f"sample count {got[8]:g} != {val[8]:g}")
    out = {}
    for i, name in enumerate(twin.STATS):
        if name not in ("time_sum", "n_samples"):
            if not math.isfinite(got[i]):
                bad.append(f"{name} is {got[i]}")
                continue
            out[name] = (twin.ratio(got[i], val[i], mag[i]), stat_k(name, n, m, cmax, num, serial))
    return out, bad


def compare_coefficients(got, ref):
    """got (m, 18) against {(s, axis): (c, mag)}: the largest ratio over the listed entries."""
    got = np.asarray(got, dtype=np.float64)
    worst = 0.0
    for (s, a), (c, mg) in ref.items():
        for j in range(6):
            worst = max(worst, twin.ratio(got[s, 6 * a + j], c[j], mg[j]))
    return worst


def hold_samples(what, got, smp, cap, probe=False):
    worst, bad = compare_samples(got, smp, cap)
    if probe:
        bad += compare_probe(got, smp, cap)
    log(dict(what=str(what), quantity="point", ratio=worst, K=K_POINT))
    assert not bad, (what, bad[:5])
    assert worst <= K_POINT, f"{what}: points: largest |err| / (u * mag) {worst:.3g} > K = {K_POINT}"
    return worst


def hold_stats(what, got, ref, serial=False):
    out, bad = compare_stats(got, ref, serial)
    for name, (r, k) in out.items():
        log(dict(what=str(what), quantity=name, ratio=r, K=k))
    assert not bad, (what, bad)
    over = {name: rk for name, rk in out.items() if not rk[0] <= rk[1]}
    assert not over, f"{what}: |err| / (u * mag) above K: {over}"
    return out


def hold_coefficients(what, got, ref):
    worst = compare_coefficients(got, ref)
    log(dict(what=str(what), quantity="coefficient", ratio=worst, K=K_COEF))
    assert worst <= K_COEF, f"{what}: coefficients: largest |err| / (u * mag) {worst:.3g} > K = {K_COEF}"
    return worst


_TWIN_CACHE = {}


def twin_of(key, coeff, T, dt):
    """(samples, stats) of the twin, computed once per input and shared (read-only) among the tests."""
    if key not in _TWIN_CACHE:
        smp = twin.samples(coeff, T, dt)
        _TWIN_CACHE[key] = (smp, twin.stats(coeff, T, dt, smp=smp))
    return _TWIN_CACHE[key]
