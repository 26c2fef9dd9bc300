"""The refinement tree of the continuous-time certificates (csrc/gtop_interval_tree.h) restated in numpy,
once for the three twins (tests/certify_twin.py, tests/certify_moving_twin.py, tests/kinematics_twin.py): a segment is
cut into 64 intervals; an OPEN interval is replaced by its 64 children, depth-first in ascending time, while the depth
and the trajectory's refinement budget allow.  A twin says what it adds as a node:

    node.evaluate(L, s, base, w, a) -> (64 statuses, 64 bounds)   the intervals [a[j], a[j] + w] of segment s at level L
    node.leaf(s, a, w, bound, status)                              the interval stays in the tree: commit its bound

Also here: the constants the certificates share (csrc/gtop_kernels.h) and a row's verdict."""
import numpy as np

MAX_DEPTH = 3
INFLATE = 1.0 + 2.0 ** -40
SLACK = 2.0 ** -40
CERTIFIED, OPEN, VIOLATION = 0, 1, 2


class Tree:
    """The options of one trajectory's tree and its running counts.  The two mutants of the tree itself: child32 (child
    width w / 32) and budget (max_refine ignored)."""

    def __init__(self, max_depth, max_refine, child32=False, budget=False):
        self.max_depth, self.max_refine = int(max_depth), int(max_refine)
        self.child = 0.03125 if child32 else 0.015625
        self.unbounded = budget
        self.nref = self.nund = 0


def walk(node, L, s, base, w, tree):
    """Level L of segment s: the 64 intervals from `base`, each of width w, evaluated; then, in ascending time, each one
    made a leaf, or — OPEN, and the depth and the budget allow — replaced by its children."""
    a = base + np.arange(64, dtype=np.float64) * w
    status, bound = node.evaluate(L, s, base, w, a)
    for j in range(64):
        if status[j] != OPEN:
            node.leaf(s, a[j], w, bound[j], status[j])
        elif L < MAX_DEPTH and L < tree.max_depth and (tree.nref < tree.max_refine or tree.unbounded):
            tree.nref += 1
            walk(node, L + 1, s, a[j], tree.child * w, tree)
        else:
            tree.nund += 1
            node.leaf(s, a[j], w, bound[j], OPEN)


def verdict(viol_t, nund):
    """(a row's verdict, the time of its first violation) from the earliest violating midpoint (inf: none)."""
    bad = viol_t != np.inf
    return (-1.0 if bad else (1.0 if nund == 0 else 0.0)), (viol_t if bad else -1.0)
