"""The walk of tests/interval_tree_twin.py alone, on a synthetic node whose statuses come from a table: at level L the
lanes OPEN_AT[L] are OPEN, lane 20 of level 0 is a VIOLATION, every other interval is CERTIFIED.  Level 0 has width 1
from 0, so every interval's ends are exact binary fractions and equalities below are exact."""
import numpy as np
import pytest

from tests import interval_tree_twin as it

OPEN_AT = {0: (3, 10, 40), 1: (5,), 2: (7,), 3: (1, 2)}


class TableNode:
    def __init__(self):
        self.evaluated = []        # (L, base, w) in the order of the calls
        self.leaves = []           # (a, w, bound, status) in the order of the calls

    def evaluate(self, L, s, base, w, a):
        assert s == 9 and np.array_equal(a, base + np.arange(64.0) * w)
        self.evaluated.append((L, base, w))
        status = [it.OPEN if j in OPEN_AT[L] else it.CERTIFIED for j in range(64)]
        if L == 0:
            status[20] = it.VIOLATION
        return status, [(L, j) for j in range(64)]

    def leaf(self, s, a, w, bound, status):
        assert s == 9
        self.leaves.append((a, w, bound, status))


def run(max_depth, max_refine, **mutant):
    node, tree = TableNode(), it.Tree(max_depth, max_refine, **mutant)
    it.walk(node, 0, 9, np.float64(0.0), np.float64(1.0), tree)
    return node, tree


def test_the_visiting_order_is_depth_first_and_ascending_in_time():
    node, tree = run(3, 1000)
    x1, x2 = 3 + 5 / 64, 3 + 5 / 64 + 7 / 4096
    assert node.evaluated[:6] == [(0, 0.0, 1.0), (1, 3.0, 1 / 64), (2, x1, 1 / 4096), (3, x2, 1 / 262144),
                                  (1, 10.0, 1 / 64), (2, 10 + 5 / 64, 1 / 4096)]
    # the leaves come in ascending time and tile [0, 64]: a refined interval's children are all visited before the
    # interval after it
    ends = [a + w for a, w, _, _ in node.leaves]
    assert node.leaves[0][0] == 0.0 and ends[-1] == 64.0
    assert all(node.leaves[i + 1][0] == ends[i] for i in range(len(ends) - 1))
    # a leaf carries the bound and the status its own evaluation gave it
    assert node.leaves[0][2:] == ((0, 0), it.CERTIFIED) and node.leaves[3][:2] == (3.0, 1 / 64) and node.leaves[3][2] == (1, 0)
    assert [lf[3] for lf in node.leaves if lf[2] == (0, 20)] == [it.VIOLATION]


@pytest.mark.parametrize("max_refine,evaluated,nund", [(0, 1, 3), (1, 2, 3), (2, 3, 3), (3, 4, 4), (4, 5, 4)])
def test_the_budget_stops_refinement_at_exactly_max_refine(max_refine, evaluated, nund):
    node, tree = run(3, max_refine)
    assert tree.nref == max_refine and len(node.evaluated) == evaluated == 1 + tree.nref and tree.nund == nund
    # the refinements went to the earliest OPEN intervals, depth first
    assert [e[0] for e in node.evaluated] == [0, 1, 2, 3, 1][:evaluated]


@pytest.mark.parametrize("max_depth,nref,nund", [(0, 0, 3), (1, 3, 3), (2, 6, 3), (3, 9, 6), (5, 9, 6)])
def test_the_depth_stops_refinement_at_the_lesser_of_max_depth_and_the_limit(max_depth, nref, nund):
    node, tree = run(max_depth, 1000)
    assert max(e[0] for e in node.evaluated) == min(max_depth, it.MAX_DEPTH)
    assert (tree.nref, tree.nund) == (nref, nund)


@pytest.mark.parametrize("max_depth,max_refine", [(0, 0), (1, 2), (3, 4), (3, 1000)])
def test_every_interval_is_a_leaf_once_unless_refined_and_nund_counts_the_open_leaves(max_depth, max_refine):
    node, tree = run(max_depth, max_refine)
    made = {(base + j * w, w) for _, base, w in node.evaluated for j in range(64)}
    refined = {(base, 64 * w) for L, base, w in node.evaluated if L > 0}
    leaves = [(a, w) for a, w, _, _ in node.leaves]
    assert len(made) == 64 * len(node.evaluated) and len(refined) == tree.nref and refined <= made
    assert len(leaves) == len(set(leaves)) and set(leaves) == made - refined
    assert sum(st == it.OPEN for _, _, _, st in node.leaves) == tree.nund


def test_the_two_mutants_of_the_tree():
    node, tree = run(3, 1, budget=True)
    assert tree.nref == 9
    node, tree = run(1, 1000, child32=True)
    assert [e[2] for e in node.evaluated] == [1.0, 1 / 32, 1 / 32, 1 / 32]
