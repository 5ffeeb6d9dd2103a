"""Host tests (no GPU): api.aggregate_level_jobs -- which nodes a level of the aggregation trees has, their children and the padding clamp
(vpbs_aggregate_level_jobs, the one statement of the rule Aggregator.aggregate and aggregate_many use) -- against a Python
restatement of the rule as DESIGN.md 8.14 words it: pad the leaves to 2^d with the last one, pair the positions, and a node whose children
are those of its left neighbour is that neighbour.  And the refusals of a many-run's arguments."""
import ctypes as C

import numpy as np
import pytest

from vpbs_amd import api


def tree_levels(c):
    """[the nodes of level 1, of level 2, ...] of one tree of c leaves, children as indices into the tree's own entries below"""
    ids = [min(i, c - 1) for i in range(1 << api.aggregate_depth(c))]   # which entry stands at each position of the padded level
    levels = []
    while len(ids) > 1:
        jobs, nxt = [], []
        for k in range(len(ids) // 2):
            ch = (ids[2 * k], ids[2 * k + 1])
            if not jobs or jobs[-1] != ch:
                jobs.append(ch)
            nxt.append(len(jobs) - 1)
        levels.append(jobs)
        ids = nxt
    return levels


def model(counts, level):
    """[(tree, left, right)] of `level`, children as indices into the list of level - 1 over all trees (level 1: the leaves)"""
    out, below = [], 0
    for t, c in enumerate(counts):
        lv = tree_levels(c)
        if level <= len(lv):
            out += [(t, below + a, below + b) for a, b in lv[level - 1]]
        below += c if level == 1 else len(lv[level - 2]) if level - 2 < len(lv) else 0
    return out


def jobs(counts, level):
    tree, left, right = api.aggregate_level_jobs(counts, level)
    assert tree.dtype == left.dtype == right.dtype == np.uint32
    return list(zip(tree.tolist(), left.tolist(), right.tolist()))


@pytest.mark.parametrize("counts", [[c] for c in range(1, 10)] + [[1, 3, 2], [5, 1]])
def test_level_jobs_are_the_padding_rule(counts):
    deepest = max(api.aggregate_depth(c) for c in counts)
    for level in range(1, deepest + 3):
        assert jobs(counts, level) == model(counts, level), (counts, level)
    # every node's children are entries of the level below, and every entry below is somebody's child exactly when its tree goes on
    below = sum(counts)
    for level in range(1, deepest + 1):
        got = jobs(counts, level)
        assert all(a <= b < below for _, a, b in got)
        below = len(got)


def test_five_leaves_are_three_two_one_nodes():
    assert [len(jobs([5], l)) for l in (1, 2, 3, 4)] == [3, 2, 1, 0]
    assert jobs([5], 1) == [(0, 0, 1), (0, 2, 3), (0, 4, 4)]
    assert jobs([5], 2) == [(0, 0, 1), (0, 2, 2)]
    assert jobs([5], 3) == [(0, 0, 1)]
    # three leaves: the padding node (2, 2); six leaves: (4, 5) and then (5, 5), both distinct
    assert jobs([3], 1) == [(0, 0, 1), (0, 2, 2)]
    assert jobs([6], 1) == [(0, 0, 1), (0, 2, 3), (0, 4, 5), (0, 5, 5)]


def test_one_leaf_is_one_node_of_the_leaf_with_itself():
    assert jobs([1], 1) == [(0, 0, 0)]
    assert jobs([1], 2) == []


def test_a_tree_contributes_nothing_above_its_depth():
    # [1, 3, 2]: depths 1, 2, 1 -- level 1 has 1 + 2 + 1 nodes over the leaves 0 | 1 2 3 | 4 5, level 2 only tree 1's, on ITS two level-1 nodes
    assert jobs([1, 3, 2], 1) == [(0, 0, 0), (1, 1, 2), (1, 3, 3), (2, 4, 5)]
    assert jobs([1, 3, 2], 2) == [(1, 1, 2)]
    assert jobs([1, 3, 2], 3) == []
    # [5, 1]: tree 1 ends at level 1; levels 2 and 3 are tree 0's alone
    assert jobs([5, 1], 1) == [(0, 0, 1), (0, 2, 3), (0, 4, 4), (1, 5, 5)]
    assert jobs([5, 1], 2) == [(0, 0, 1), (0, 2, 2)]
    assert jobs([5, 1], 3) == [(0, 0, 1)]
    assert jobs([5, 1], 4) == []


def test_a_capacity_below_the_count_writes_only_that_many():
    c = np.array([5, 1], np.uint64)
    cp = c.ctypes.data_as(C.POINTER(C.c_size_t))
    tree, left, right = (np.full(4, 77, np.uint32) for _ in range(3))
    assert api.lib().vpbs_aggregate_level_jobs(cp, 2, 1, tree.ctypes.data, left.ctypes.data, right.ctypes.data, 2) == 4
    assert tree.tolist() == [0, 0, 77, 77] and left.tolist() == [0, 2, 77, 77] and right.tolist() == [1, 3, 77, 77]


def test_the_refusals():
    L = api.lib()
    c = np.array([2, 0], np.uint64)
    cp = c.ctypes.data_as(C.POINTER(C.c_size_t))
    assert L.vpbs_aggregate_level_jobs(None, 1, 1, None, None, None, 0) < 0            # null counts
    assert L.vpbs_aggregate_level_jobs(cp, 0, 1, None, None, None, 0) < 0              # no tree
    assert L.vpbs_aggregate_level_jobs(cp, 1, 0, None, None, None, 0) < 0              # level 0 are the leaves
    assert L.vpbs_aggregate_level_jobs(cp, 2, 1, None, None, None, 0) < 0              # an empty tree
    assert L.vpbs_aggregate_level_jobs(cp, 1, 1, None, None, None, 1) < 0              # a capacity without arrays
    assert L.vpbs_aggregate_level_jobs(cp, 1, 1, None, None, None, 0) == 1
    # a many-run's arguments, as Aggregator.aggregate_many checks them before the library sees them (levels = 3: up to 8 leaves a tree)
    with pytest.raises(ValueError, match="non-empty list"):
        api.aggregate_many_args([], levels=3)
    with pytest.raises(ValueError, match="tree 1 is empty"):
        api.aggregate_many_args([2, 0], levels=3)
    with pytest.raises(ValueError, match=r"tree 2: 9 leaves exceed 2\^levels = 8"):
        api.aggregate_many_args([1, 8, 9], levels=3)
    with pytest.raises(ValueError, match="tree 0 is empty"):
        api.aggregate_level_jobs([0], 1)
    with pytest.raises(ValueError, match="level is at least 1"):
        api.aggregate_level_jobs([2], 0)
    assert api.aggregate_many_args([1, 3, 2], levels=3).tolist() == [0, 1, 4, 6]
    # ... and the library's own, for a caller of the C ABI: no aggregator, no run
    err = C.create_string_buffer(256)
    assert L.vpbs_aggregator_run_many(None, None, None, None, 0, api.AGGREGATE_TREE_FN(lambda *a: None), None, err, 256) < 0
    assert b"null aggregator" in err.value
    assert L.vpbs_aggregator_set_device_witness(None, 4, err, 256) < 0 and b"null aggregator" in err.value
    assert L.vpbs_aggregator_device_stats(None, None) < 0
