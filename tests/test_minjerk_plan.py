"""The launch plan of the minimum-jerk start point (csrc/gtop_minjerk_plan.{h,cpp}) on the CPU: plain C++ that a host
compiler builds without any HIP header (tests/minjerk_plan.py, tests/cpp/minjerk_plan_dump.cpp).

The expectations below were written by hand from the rule, not generated from the plan: one lane per trajectory, 24
bytes of LDS per lane and interior waypoint, at most 65 536 bytes per workgroup, lanes a power of two from 64 down to 8:
  64 lanes   24 * 64 * (m - 1) <= 65 536  <=>  m - 1 <= 42   (64 512 bytes at m = 43; 66 048 at 44)
  32 lanes   24 * 32 * (m - 1) <= 65 536  <=>  m - 1 <= 85   (65 280 at m = 86; 66 048 at 87)
  16 lanes   24 * 16 * (m - 1) <= 65 536  <=>  m - 1 <= 170  (65 280 at m = 171; 65 664 at 172)
   8 lanes   up to the limit of 227 segments                 (43 392 at m = 227)
  workgroups ceil(B / lanes); m outside 2 .. 227 or B < 0 refused.
The GPU side of the same switches is tests/test_gpu_minjerk.py."""
import shutil

import pytest

from tests import minjerk_plan

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")

# (B, m) -> (supported, lanes, workgroups, LDS bytes)
EXPECTED = {
    (1, 2): (1, 64, 1, 1536), (1, 3): (1, 64, 1, 3072), (130, 6): (1, 64, 3, 7680),
    # 64 -> 32 lanes
    (130, 42): (1, 64, 3, 62976), (130, 43): (1, 64, 3, 64512), (130, 44): (1, 32, 5, 33024), (130, 45): (1, 32, 5, 33792),
    # 32 -> 16
    (130, 85): (1, 32, 5, 64512), (130, 86): (1, 32, 5, 65280), (130, 87): (1, 16, 9, 33024), (130, 88): (1, 16, 9, 33408),
    # 16 -> 8
    (130, 170): (1, 16, 9, 64896), (130, 171): (1, 16, 9, 65280), (130, 172): (1, 8, 17, 32832), (130, 173): (1, 8, 17, 33024),
    # the limits of m
    (1, 226): (1, 8, 1, 43200), (1, 227): (1, 8, 1, 43392), (130, 227): (1, 8, 17, 43392),
    (1, 228): (0, 0, 0, 0), (1, 1): (0, 0, 0, 0), (1, 0): (0, 0, 0, 0), (1, -3): (0, 0, 0, 0),
    # B: nothing to launch, exact multiples and one past them, a refusal
    (0, 6): (1, 64, 0, 7680), (64, 6): (1, 64, 1, 7680), (65, 6): (1, 64, 2, 7680), (128, 6): (1, 64, 2, 7680),
    (129, 6): (1, 64, 3, 7680), (8, 227): (1, 8, 1, 43392), (9, 227): (1, 8, 2, 43392), (-1, 6): (0, 0, 0, 0),
    (2147483647, 6): (1, 64, 33554432, 7680), (2147483647, 227): (1, 8, 268435456, 43392),
}


def test_plan_matches_the_hand_written_expectations():
    pairs = list(EXPECTED)
    for pair, p in zip(pairs, minjerk_plan.plans(pairs)):
        assert (p["supported"], p["lanes"], p["blocks"], p["lds_bytes"]) == EXPECTED[pair], (pair, p)


def test_constants():
    c = minjerk_plan.constants()
    assert c == dict(min_segments=2, max_segments=227, block_doubles=3, max_lanes=64, min_lanes=8, lds_budget=65536)


def test_every_supported_length_fits_and_the_next_size_up_would_not():
    ms = list(range(2, 228))
    for m, p in zip(ms, minjerk_plan.plans([(1, m) for m in ms])):
        assert p["supported"] == 1 and p["lanes"] in (8, 16, 32, 64)
        assert p["lds_bytes"] == 24 * p["lanes"] * (m - 1) <= 65536
        assert p["lanes"] == 64 or 24 * 2 * p["lanes"] * (m - 1) > 65536, m


def test_lds_slots_are_distinct_in_bounds_and_lane_interleaved():
    assert minjerk_plan.slot_violations() == []
