"""A used context gives a fresh context's bits, entry by entry.

Every family test builds one context and runs one family in one fixed order; this file asks the question none of them
asks: does a result depend on what the context did BEFORE the call?  One gtop_ctx is driven by 13 gtop_capi_*.cpp files
that share some 25 grow-only scratch buffers (seg_rep alone is packed in six layouts), GtopDevBuf::reserve drops the
contents when it grows, fresh device memory is usually zero — so a kernel that relies on zeroed scratch, a host form
that reads a region an earlier, larger call staged, a workspace whose padding rows should hold NaN, a counter that is
never reset and a knob that leaks into an entry that should ignore it all pass on a new context and can fail on a used
one.

The operations are those of tests/history_ops.py.  The REFERENCE of an (operation, size, field) is its run on a fresh
context that has done nothing but build that field; it is made lazily, once, and kept.  The family tests hold a fresh
context's results to their twins; here the only claim is that history changes nothing, so every comparison is on the
bytes (arrays viewed as uint8, so that NaNs compare), with no tolerance and no list of excused rows.

 (a) determinism first: every reference is made twice, on two fresh contexts, and the two must be equal;
 (b) 12 seeds x 30 steps on one long-lived context: "switch to field X" (a whole rebuild) or a draw of (operation,
     size), compared with the reference of the field in force after every operation step;
 (c) directed pairs, per shared buffer: for every ordered pair (P, Q) of operations that reach it from different files,
     P(large) -> Q(small) -> compare Q on the buffer's one context, and Q(small) -> P(large) -> Q(odd) -> compare P and Q
     on a context of the pair's own;
 (d) knob residue: a knob set, then an operation of a family whose header says it does not read that knob.

Deliberately out of scope:
 - graph capture and replay: a captured launch holds the addresses of context buffers, a later, larger call frees them
   when it grows, and a replay after growth is a use-after-free by the documented contract — testing it would provoke
   a fault on a shared machine, so this file has no torch.cuda.graph;
 - two streams or two host threads on one context (the contract is one context per thread / stream);
 - several contexts working at once (the harness makes its fresh contexts beside the used one, one call at a time);
 - `maxtime` stop rules: time-dependent by contract (every optimizer here runs with maxtime = 0)."""
import numpy as np
import pytest

from tests import history_ops as H

pytestmark = pytest.mark.gpu

_reference = {}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8),
                                                                          b.reshape(-1).view(np.uint8))


def differences(got, want):
    """The outputs that differ, each with the number of elements whose bytes differ: [] when all are the same."""
    out = []
    if sorted(got) != sorted(want):
        return [f"outputs {sorted(got)} != {sorted(want)}"]
    for k in sorted(want):
        a, b = got[k], want[k]
        if not same_bytes(a, b):
            if a.dtype == b.dtype and a.shape == b.shape and a.size:
                w = a.dtype.itemsize
                bad = (a.reshape(-1).view(np.uint8).reshape(-1, w) != b.reshape(-1).view(np.uint8).reshape(-1, w)).any(axis=1)
                first = int(np.flatnonzero(bad)[0])
                out.append(f"{k}: {int(bad.sum())} of {a.size} elements, first at flat index {first}: "
                           f"{a.reshape(-1)[first]!r} != {b.reshape(-1)[first]!r}")
            else:
                out.append(f"{k}: {a.dtype} {a.shape} != {b.dtype} {b.shape}")
    return out


def fresh_run(gtop, name, size, field):
    w = H.world(field)
    ctx = gtop.GtopContext(device=0)
    try:
        H.build_field(ctx, w)
        return H.OPS[name].run(ctx, w, size)
    finally:
        ctx.close()


def reference(gtop, name, size, field):
    """(a) lives here: the reference is made on two fresh contexts, and both runs must give the same bytes."""
    key = (name, size, field)
    if key not in _reference:
        first, second = fresh_run(gtop, *key), fresh_run(gtop, *key)
        diff = differences(second, first)
        assert not diff, f"{key} is not deterministic on two fresh contexts: {diff}"
        for a in first.values():
            a.setflags(write=False)
        _reference[key] = first
    return _reference[key]


class Used:
    """One long-lived context and what it did: every check's message carries the whole history."""

    def __init__(self, gtop, field, note=""):
        self.gtop, self.history, self.note = gtop, [], note
        self.ctx = gtop.GtopContext(device=0)
        self.switch(field)

    def switch(self, field):
        self.field = field
        self.history.append(("field", field))
        H.build_field(self.ctx, H.world(field))

    def run(self, name, size, compare=True):
        self.history.append(("op", name, size))
        o = H.OPS[name]
        got = o.run(self.ctx, H.world(self.field), size)
        if o.rebuilds:
            H.build_field(self.ctx, H.world(self.field))    # (not a step of its own: the window left another field)
        if compare:
            diff = differences(got, reference(self.gtop, name, size, self.field))
            assert not diff, f"{self.note}: {name}({size}) on field {self.field} differs from a fresh context's: " \
                             f"{diff}; history {self.history}"
        return got

    def close(self):
        self.ctx.close()


# ---- (a) ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(H.OPS))
def test_references_are_deterministic(gtop, name):
    for size in H.SIZES:
        ref = reference(gtop, name, size, "A")
        assert ref and all(a.size for a in ref.values()), (name, size, {k: a.shape for k, a in ref.items()})


# ---- (b) ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(H.SEEDS))
def test_random_histories(gtop, seed):
    steps = H.schedule(seed)
    u = Used(gtop, steps[0][1], note=f"seed {seed}")
    try:
        for step in steps[1:]:
            if step[0] == "field":
                u.switch(step[1])
            else:
                u.run(step[1], step[2])
    finally:
        u.close()


# ---- (c) ------------------------------------------------------------------------------------------------------------

def _pair_cases():
    """One case per shared buffer.  Buffers with the same list of pairs (d_T, d_Df and d_x; mma_lb and mma_ub) are one
    case: the same runs would prove the same thing again."""
    groups = {}
    for b in H.shared_buffers():
        groups.setdefault(tuple(H.pairs_for(b)), []).append(b)
    return [pytest.param(buffers, pairs, id="+".join(buffers)) for pairs, buffers in groups.items()]


@pytest.mark.parametrize("buffers, pairs", _pair_cases())
def test_directed_pairs(gtop, buffers, pairs):
    """The first sequence of every pair runs on ONE context per buffer, which so collects every layout that any user
    leaves in it.  The buffers only grow, so on that context P(large) can grow under Q's staging once at the most; the
    second sequence is about exactly that, and therefore starts on a context of its own, where Q(small) sizes the buffer
    first and P(large) then grows it."""
    shared = Used(gtop, "A", note=f"buffers {buffers}, first sequences")
    try:
        for p, q in pairs:
            shared.run(p, "large", compare=False)
            shared.run(q, "small")
            own = Used(gtop, "A", note=f"buffers {buffers}, second sequence of ({p}, {q})")
            try:
                own.run(q, "small", compare=False)
                own.run(p, "large")
                own.run(q, "odd")
            finally:
                own.close()
    finally:
        shared.close()


# ---- (d) ------------------------------------------------------------------------------------------------------------

def _boxes(u, kind, nbox):
    i = H.Inp("knob residue", "small", H.world(u.field))
    if kind == "polynomial":
        coef, scale, t_range = i.boxes_polynomial(nbox)
        u.ctx.set_moving_box_polynomials(coef, scale, t_range)
    else:
        u.ctx.set_moving_boxes(*i.boxes_const_vel(nbox))
    u.ctx.set_moving_cost(True)


def _fp32_evaluation(u):
    H.OPS["eval_device_f32"].run(u.ctx, H.world(u.field), "small")


# residue -> (how it is left, the operations behind it: of families whose headers do not name the knob)
REPORTS = ["validate_batch", "certify_batch", "certify_kinematics_batch", "trajectory_stats", "edt_query"]
RESIDUES = {
    **{f"launch_geometry_{s}": (lambda u, s=s: u.ctx.set_launch_geometry(0, s),
                                REPORTS + ["time_gradient_batch", "joint_gradient_batch", "separation_batch"])
       for s in (3, 6, 10, 30)},
    "optimizer_fusion_0": (lambda u: u.ctx.set_optimizer_fusion(0), ["eval_batch", "optimize_swarm", "optimize_times"]),
    "optimizer_fusion_1": (lambda u: u.ctx.set_optimizer_fusion(1), ["eval_device_f64", "optimize_swarm", "optimize_joint"]),
    "optimizer_precision_f32": (lambda u: u.ctx.set_optimizer_precision("f32"),
                                ["eval_batch", "eval_device_f64", "time_gradient_batch", "optimize_times"] + REPORTS),
    "gradient_mode_consistent": (lambda u: u.ctx.set_gradient_mode(True),
                                 ["time_gradient_batch", "optimize_times", "joint_gradient_batch", "optimize_joint",
                                  "time_gradient_moving_batch"] + REPORTS),
    "moving_cost_32_polynomial": (lambda u: _boxes(u, "polynomial", 32),
                                  ["validate_batch", "certify_batch", "certify_moving_batch", "trajectory_stats",
                                   "separation_batch", "certify_kinematics_batch", "insert_waypoints"]),
    "moving_cost_1_const_vel": (lambda u: _boxes(u, "const_vel", 1),
                                ["validate_batch", "certify_batch", "certify_moving_batch", "trajectory_stats",
                                 "separation_batch", "certify_kinematics_batch", "insert_waypoints"]),
    "start_times_B": (lambda u: u.ctx.set_start_times(np.linspace(0.5, 1.5, H.SIZES["odd"][0])),
                      ["edt_query", "edt_coarse_query", "trajectory_stats", "trajectory_samples", "coefficients_device",
                       "min_jerk_start", "fit_predictions_device", "set_paths"]),
    "fp32_in_use": (_fp32_evaluation, ["eval_batch", "eval_device_f64", "optimize_batch_ex_fusion2", "validate_batch",
                                       "update_sdf_map_window", "update_sdf_map_window_device", "time_gradient_batch"]),
}


@pytest.mark.parametrize("residue", sorted(RESIDUES))
def test_knob_residue(gtop, residue):
    leave, followers = RESIDUES[residue]
    for name in followers:
        u = Used(gtop, "A", note=f"residue {residue}")
        try:
            leave(u)
            u.history.append(("residue", residue))
            u.run(name, "odd")
            u.run(name, "small")
        finally:
            u.close()
