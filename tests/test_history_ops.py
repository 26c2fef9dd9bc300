"""CPU tests that keep the catalogue of tests/history_ops.py honest: every entry point of the headers is claimed by an
operation or excluded with a reason, the buffer-sharing table is what csrc/ says, and the schedules of the random
histories visit what tests/test_gpu_history.py promises."""
import collections
import glob
import os
import re

from tests import history_ops as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_entry_points():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        names |= set(re.findall(r"\bint\s+(gtop_\w+)\s*\(", open(path).read()))
    return names


# entries the catalogue must hold in more than one variant: eval_device in f64, in f32 and under the moving cost; the
# optimizer's host form with fusion 2 and with fusion 0; its device form static and under the moving cost; get_sdf
# behind both window updates
VARIANTS = {"gtop_eval_device": 3, "gtop_optimize_batch_ex": 2, "gtop_optimize_device_ex": 2, "gtop_get_sdf": 2}


def check_entry_points(ops, excluded):
    """The rules, as a function of the tables so that the test can also show that it bites."""
    declared = header_entry_points()
    claimed = {e for o in ops.values() for e in o.entries}
    assert len(declared) > 100
    assert not declared - claimed - set(excluded), f"neither claimed nor excluded: {sorted(declared - claimed - set(excluded))}"
    assert not claimed & set(excluded), f"claimed and excluded: {sorted(claimed & set(excluded))}"
    assert not (claimed | set(excluded)) - declared, f"in no header: {sorted((claimed | set(excluded)) - declared)}"
    for entry in claimed:
        n = sum(entry in o.entries for o in ops.values())
        assert n == VARIANTS.get(entry, 1), f"{entry}: claimed by {n} operations, {VARIANTS.get(entry, 1)} expected"


def check_buffer_users(table):
    found = H.buffer_users_in_source()
    assert len(found) > 25 and set(found) == set(table), sorted(set(found) ^ set(table))
    for name, users in found.items():
        assert users == table[name], f"c->{name}: csrc says {sorted(users)}, BUFFER_USERS says {sorted(table[name])}"


def test_every_entry_point_is_claimed_or_excluded():
    check_entry_points(H.OPS, H.EXCLUDED)
    assert all(reason for reason in H.EXCLUDED.values())
    for o in H.OPS.values():
        assert o.entries and o.reads <= set(H.STATE), o.name
        assert H.op_file(o), f"{o.name}: {o.entries[0]} is defined in no gtop_capi_*.cpp"


def test_removing_an_operation_is_noticed():
    import pytest
    for name in H.OPS:
        with pytest.raises(AssertionError, match="neither claimed nor excluded|expected"):
            check_entry_points({k: v for k, v in H.OPS.items() if k != name}, H.EXCLUDED)


def test_buffer_sharing_table():
    check_buffer_users(H.BUFFER_USERS)


def test_removing_a_buffer_user_is_noticed():
    import pytest
    for name, users in H.BUFFER_USERS.items():
        for gone in users:
            with pytest.raises(AssertionError):
                check_buffer_users({**H.BUFFER_USERS, name: users - {gone}})


def test_reach_of_the_operations():
    """What the pairs of the directed test are drawn from: the buffers an operation's entries mention, themselves or
    through the C-API functions they call (so a file may reach a buffer that only another file names: the reports read
    c->boxes through gtop_box_list).  The reach is parsed from csrc/, and a parser that misses a call only shrinks the
    list of tests; so the reach is held from the other side too: every file that names a shared buffer supplies an
    operation to that buffer's pairs."""
    assert H.entry_reach("gtop_separation_batch") == ("gtop_capi_separation.cpp",
                                                      frozenset({"sep_stage", "mma_g", "d_T", "d_x", "d_Df"}))
    assert H.entry_reach("gtop_eval_device")[1] == {"box_rows"}       # (through gtop_moving_args, behind a template)
    assert H.entry_reach("gtop_time_gradient_device")[1] == frozenset()
    assert "seg_rep" in H.entry_reach("gtop_insert_waypoints")[1] and "d_pts" in H.entry_reach("gtop_set_paths")[1]
    # optimize_on_stream and gradient_on_stream are file-local names that four files define: each caller means its own
    assert {"mma_f", "mma_g", "mma_vec", "box_rows"} <= H.entry_reach("gtop_optimize_swarm_device")[1]
    assert {"mma_f", "mma_g", "swarm_stage", "d_x"} <= H.entry_reach("gtop_optimize_swarm")[1]
    assert H.entry_reach("gtop_optimize_times_moving_device")[1] == {"boxes", "box_rows"}
    assert H.entry_reach("gtop_optimize_joint_device")[1] == frozenset()
    names = [name for _, name in H._functions()]
    assert names.count("optimize_on_stream") == 4 and names.count("gradient_on_stream") == 4
    shared = H.shared_buffers()
    assert len(shared) >= 14
    for b in shared:
        pairs = H.pairs_for(b)
        assert pairs, b
        assert all(H.op_file(H.OPS[p]) != H.op_file(H.OPS[q]) for p, q in pairs)
        files = {H.op_file(H.OPS[n]) for pair in pairs for n in pair}
        missing = H.BUFFER_USERS[b] - files - H.NO_OPERATION_OF_ITS_OWN.get(b, set())
        assert not missing, f"{b}: no operation of {sorted(missing)} is among its pairs"
    for b, files in H.NO_OPERATION_OF_ITS_OWN.items():
        reach = {H.op_file(o) for o in H.OPS.values() if b in H.op_buffers(o)}
        assert files <= H.BUFFER_USERS[b] and not files & reach, (b, "the exception is no longer needed")


def test_reads_is_the_state_that_run_sets():
    for o in H.OPS.values():
        assert set(o.reads) - {"field"} == H.state_set_by(o), (o.name, sorted(o.reads), sorted(H.state_set_by(o)))


def test_schedules_visit_every_operation_twice_in_each_size():
    visits = collections.Counter()
    for seed in range(H.SEEDS):
        steps = H.schedule(seed)
        assert steps == H.schedule(seed), "seeded"
        assert len(steps) == H.STEPS == 30 and steps[0][0] == "field"
        assert {s[1] for s in steps if s[0] == "field"} == set(H.FIELDS)       # every seed sees every field
        for s in steps:
            assert (s[0] == "field" and s[1] in H.FIELDS) or (s[0] == "op" and s[1] in H.OPS and s[2] in H.SIZES), s
            if s[0] == "op":
                visits[s[1:]] += 1
    assert H.SEEDS == 12
    short = {(n, z): visits[(n, z)] for n in H.OPS for z in H.SIZES if visits[(n, z)] < 2}
    assert not short, short


def test_sizes_and_fields():
    assert H.SIZES == {"small": (5, 3), "large": (130, 13), "odd": (65, 7)}
    assert [(f["grid"], f["res"], f["signed"]) for f in H.FIELDS.values()] == [
        ((40, 36, 20), 0.2, False), ((23, 50, 17), 0.25, False), ((40, 36, 20), 0.2, True)]
    assert H.MAX_SAMPLES <= 64 and H.GRID_SAMPLES <= 64 and H.MAX_EVALS <= 8
    for size, (lo, hi) in H.WINDOWS.items():
        for f in H.FIELDS.values():
            assert all(0 <= a <= b < n for a, b, n in zip(lo, hi, f["grid"])), (size, f["grid"])
