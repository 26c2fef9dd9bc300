"""The shapes at which the swarm term's kernels (csrc/gtop_swarm.hip, csrc/gtop_sep_sample.h) take the branches that
only long rows and long grids reach, and the arithmetic that says which branch a shape takes — stated from the
kernels' constants, so that the GPU tests (tests/test_gpu_swarm_limits.py) and the CPU test of the twin at the same
lengths (tests/test_swarm_twin.py) name one table.  Nothing here needs a GPU.

A case is (B, m, n_samples, shared T, start-time kind, hold_ends, frozen, edges), the columns of CASES of
tests/test_gpu_swarm.py and the names of the edges the case is there for; edge_faults() says which of them a run of
the twin does NOT show."""
import numpy as np

LANES = 64            # a wavefront: the rows kernel's lanes, the pass over items / variables / kstart entries
STAGE = 256           # kSwarmStage: samples staged in LDS per turn of the rows kernel
TILE, CHUNK = 64, 8   # kSepTile, kSepChunk: the rows of a tile, the padding of the samples
SAMPLE_BLOCKS = 4096  # sep_launch_sample: at most this many blocks of 4 samples over all tiles
MAX_M, MAX_SAMPLES, OPT_MAX_M = 227, 65536, 118

LIMIT_CASES = [
    (3, 9, 8, False, "B", 0, False, ("second_variable_pass", "empty_segments")),
    (3, 8, 64, True, 0, 1, True, ("one_below_the_lanes",)),
    (2, 64, 130, True, 0, 1, True, ("second_kstart_pass",)),
    (3, 65, 520, False, "B", 0, False, ("two_stages", "boundary_in_every_stage", "straddled_stage_edge")),
    (3, 65, 600, False, "B", 0, False, ("three_stages", "boundary_in_every_stage")),
    (3, 227, 64, False, 0, 1, False, ("moments_full", "empty_segments_160")),
    (3, 227, 700, True, "B", 0, True, ("moments_full", "three_stages", "boundary_in_every_stage", "skipped_passes")),
    (66, 118, 300, False, "B", 1, False, ("optimizer_largest_m", "a_tile_and_two_rows", "two_stages")),
    (3, 13, 16400, False, "B", 0, False, ("stride_loop", "one_tile")),
    (65, 7, 8200, True, "B", 0, False, ("stride_loop", "two_tiles")),
    (130, 9, 5480, False, "B", 0, False, ("stride_loop", "three_tiles", "padded_last_tile")),
    (2, 2, 65536, False, 0, 1, False, ("most_samples", "stages_256")),
]

# the float twin against the exact one where the sums are long (dyadic rows): (B, m, n_samples, hold_ends, frozen, seed)
TWIN_CASES = [(2, 9, 300, 0, False, 31), (2, 65, 130, 1, True, 32)]


def case_id(case):
    return f"B{case[0]}-m{case[1]}-n{case[2]}"


def sample_blocks(B, n):
    """(tiles, npad, gridDim.y) of sep_launch_sample for B rows on n samples."""
    tiles = -(-B // TILE)
    npad = -(-n // CHUNK) * CHUNK
    return tiles, npad, min((npad + 3) // 4, max(1, SAMPLE_BLOCKS // tiles))


def row_starts(seg_b, flown_b, m):
    """(kstart (m + 1,), kf, kend) of one row: the first flown sample whose segment is >= s, s = 0 .. m; a segment s
    owns the samples kstart[s] .. kstart[s + 1] - 1.  The flown samples of a row are contiguous."""
    ks = np.flatnonzero(flown_b)
    if ks.size == 0:
        return np.zeros(m + 1, dtype=np.int64), 0, 0
    kf, kend = int(ks[0]), int(ks[-1]) + 1
    assert ks.size == kend - kf and np.all(np.diff(seg_b[kf:kend]) >= 0)
    return kf + np.searchsorted(seg_b[kf:kend], np.arange(m + 1), side="left"), kf, kend


def row_figures(seg_b, flown_b, m):
    """What the rows kernel meets on one row, counted from the twin's walk: the stages, the segments without a sample,
    per stage the segment boundaries strictly inside it, the stage edges a segment straddles, and the 64-item passes
    the skip test leaves out / takes."""
    kstart, kf, kend = row_starts(seg_b, flown_b, m)
    stages = [(c0, min(c0 + STAGE, kend)) for c0 in range(kf, kend, STAGE)]
    inside, straddled, skipped, taken = [], 0, 0, 0
    for c0, c1 in stages:
        k = np.arange(c0 + 1, c1)
        inside.append(int(np.count_nonzero(seg_b[k] != seg_b[k - 1])))
        straddled += int(c0 > kf and seg_b[c0] == seg_b[c0 - 1])
        for base in range(0, 18 * m, LANES):
            s_lo, s_hi = base // 18, min((base + LANES - 1) // 18, m - 1)
            if kstart[s_lo] >= c1 or kstart[s_hi + 1] <= c0:
                skipped += 1
            else:
                taken += 1
    return dict(stages=len(stages), empty=int(np.count_nonzero(kstart[1:] == kstart[:-1])), inside=inside,
                straddled=straddled, skipped=skipped, taken=taken)


def edge_faults(case, seg, flown):
    """The edges named by the case that the twin's seg / flown (B, n) do not show (an empty list: all there), and the
    figures they were read from."""
    B, m, n = case[:3]
    nvar, items = 9 * (m - 1), 18 * m
    tiles, npad, gy = sample_blocks(B, n)
    rows = [row_figures(seg[b], flown[b], m) for b in range(B)]
    most = max(rows, key=lambda r: r["stages"])
    shows = {
        "second_variable_pass": LANES < nvar <= 2 * LANES,
        "one_below_the_lanes": nvar == LANES - 1,
        "second_kstart_pass": m == LANES,                       # s = 0 .. m: entry 64 alone is a second trip
        "empty_segments": all(r["empty"] > 0 for r in rows),
        "empty_segments_160": all(r["empty"] >= 160 for r in rows),
        "moments_full": m == MAX_M,
        "two_stages": any(r["stages"] >= 2 for r in rows),
        "three_stages": all(r["stages"] >= 3 for r in rows),
        "boundary_in_every_stage": all(r["stages"] >= 2 and min(r["inside"]) > 0 for r in rows),
        "straddled_stage_edge": any(r["straddled"] > 0 for r in rows),
        "skipped_passes": all(r["skipped"] > 0 and r["taken"] > 0 for r in rows) and items > 3 * LANES,
        "optimizer_largest_m": m == OPT_MAX_M,
        "a_tile_and_two_rows": B == TILE + 2,
        "stride_loop": npad // 4 > max(1, SAMPLE_BLOCKS // tiles) and gy * 4 < npad,
        "one_tile": tiles == 1,
        "two_tiles": tiles == 2,
        "three_tiles": tiles == 3,
        "padded_last_tile": B % TILE != 0 and tiles > 1,
        "most_samples": n == MAX_SAMPLES,
        "stages_256": most["stages"] == MAX_SAMPLES // STAGE,
    }
    figures = dict(nvar=nvar, items=items, tiles=tiles, npad=npad, gy=gy, stages=[r["stages"] for r in rows[:4]],
                   empty=[r["empty"] for r in rows[:4]], inside=[r["inside"][:4] for r in rows[:4]],
                   straddled=sum(r["straddled"] for r in rows), skipped=[r["skipped"] for r in rows[:4]])
    return [e for e in case[7] if not shows[e]], figures
