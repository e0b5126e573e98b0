"""host/bvh_pairs.hpp — the device layout of the BVH (sibling pairs, link words, big_leaf_n, the instances' leaf slots and root records) — at the smallest shapes
that can go wrong, through the oracle library's orc_fn_bvh_pairs (pure host code: no GPU). A walk of the pair layout must visit the same leaves in the same order
as a walk of the depth-first array, and every link word must decode to the node it was made from."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import oracle_py  # noqa: E402

LINK_LEAF, LINK_OTHER, LINK_INDEX_MASK, LINK_COUNT_SHIFT, LINK_COUNT_MAX, LINK_AXIS_SHIFT = 0x80000000, 0x40000000, 0x07FFFFFF, 27, 7, 29
SPHERE, INSTANCE = 0x80000000, 0x20000000  # shm/scene.h: PRIM_SPHERE_BIT, PRIM_INSTANCE_BIT
UNSEEN = 0xFFFFFFFF


def box(size):
    return (0.0, 0.0, 0.0), (float(size), float(size), float(size))


def leaf(offset, n, size=1.0):
    return box(size) + (offset, n, 0)


def interior(second_child, axis=0, size=2.0):
    return box(size) + (second_child, 0, axis)


def walk_depth_first(nodes, root=0):
    """[(first primitive slot, n_prims)] of the leaves in visit order: first child (o + 1), then second (offset)"""
    out, stack = [], [root]
    while stack:
        o = stack.pop()
        _, _, offset, n, _ = nodes[o]
        if n:
            out.append((offset, n))
        else:
            stack += [offset, o + 1]
    return out


def decode_leaf(link, res, kinds):
    """(first primitive slot, n_prims) of a leaf's link word"""
    assert link & LINK_LEAF
    count = (link >> LINK_COUNT_SHIFT) & 7
    if link & LINK_OTHER:
        if count == 0:  # an instance: its index in place of the slot, the slot in the instance's record
            slot = res["inst_slot"][link & LINK_INDEX_MASK]
            assert kinds[slot] == INSTANCE | (link & LINK_INDEX_MASK)
            return slot, 1
        assert count == 1 and kinds[link & LINK_INDEX_MASK] & SPHERE
        return link & LINK_INDEX_MASK, 1
    slot = link & LINK_INDEX_MASK
    if count == LINK_COUNT_MAX:
        return slot, res["big_leaf_n"][slot]
    return slot, count


def walk_pairs(res, kinds, root=0):
    out, stack = [], [root]
    while stack:
        i = stack.pop()
        _, _, link, n, _ = res["nodes"][i]
        if link & LINK_LEAF:
            out.append(decode_leaf(link, res, kinds))
            assert out[-1][1] == n  # (n_prims stays where it was)
        else:
            first = link & LINK_INDEX_MASK
            assert first % 2 == 0 and first + 1 < len(res["nodes"])
            stack += [first + 1, first]
    return out


def check(nodes, kinds, inst_roots=()):
    res = oracle_py.bvh_pairs(nodes, kinds, inst_roots)
    roots = sorted({0, *inst_roots})
    assert res["nodes"][1][2:] == (0, 0, 0)  # a root sits alone in its block: the odd slot is a zeroed record
    for k, r in enumerate(inst_roots):
        new_root = res["inst_root"][k]
        assert new_root % 2 == 0 and res["inst_root_rec"][k] == res["nodes"][new_root]
        assert walk_pairs(res, kinds, new_root) == walk_depth_first(nodes, r)
    assert walk_pairs(res, kinds, 0) == walk_depth_first(nodes, 0)
    # every reachable node once: boxes and axes carried over, an interior node's link names its axis
    reached = sum(len(walk_all(nodes, r)) for r in roots)
    assert len(res["nodes"]) == 2 * len(roots) + 2 * sum(1 for r in roots for o in walk_all(nodes, r) if nodes[o][3] == 0)
    assert sum(1 for n in res["nodes"] if n[3] or n[2]) == reached
    return res


def walk_all(nodes, root):
    out, stack = [], [root]
    while stack:
        o = stack.pop()
        out.append(o)
        if nodes[o][3] == 0:
            stack += [nodes[o][2], o + 1]
    return out


def test_single_leaf():
    res = check([leaf(0, 1)], [0])
    assert len(res["nodes"]) == 2 and res["nodes"][0][2] == LINK_LEAF | (1 << LINK_COUNT_SHIFT) | 0 and res["big_leaf_n"] is None


def test_one_interior_node_with_two_leaves():
    res = check([interior(2, axis=2), leaf(0, 2), leaf(2, 3)], [0] * 5)
    assert len(res["nodes"]) == 4
    assert res["nodes"][0][2] == (2 << LINK_AXIS_SHIFT) | 2
    assert res["nodes"][2][2] == LINK_LEAF | (2 << LINK_COUNT_SHIFT) | 0 and res["nodes"][3][2] == LINK_LEAF | (3 << LINK_COUNT_SHIFT) | 2


def test_leaves_of_seven_and_eight_primitives():
    """LINK_COUNT_MAX: a count of 7 in the link word means "read big_leaf_n", for a leaf of exactly 7 as for one of 8; 6 still rides in the word."""
    res = check([interior(2), leaf(0, 7), interior(4), leaf(7, 8), leaf(15, 6)], [0] * 21)
    big = res["big_leaf_n"]
    assert big[0:7] == [7, 6, 5, 4, 3, 2, 1] and big[7:15] == [8, 7, 6, 5, 4, 3, 2, 1] and big[15:21] == [0] * 6
    links = sorted(n[2] for n in res["nodes"] if n[2] & LINK_LEAF)
    assert links == sorted([LINK_LEAF | (7 << LINK_COUNT_SHIFT) | 0, LINK_LEAF | (7 << LINK_COUNT_SHIFT) | 7, LINK_LEAF | (6 << LINK_COUNT_SHIFT) | 15])


def test_no_big_leaf_table_below_seven():
    assert check([interior(2), leaf(0, 6), leaf(6, 6)], [0] * 12)["big_leaf_n"] is None


def test_one_primitive_leaf_holding_a_sphere():
    res = check([interior(2), leaf(0, 1), leaf(1, 2)], [SPHERE | 0, 0, SPHERE | 1])
    assert res["nodes"][2][2] == LINK_LEAF | LINK_OTHER | (1 << LINK_COUNT_SHIFT) | 0
    assert res["nodes"][3][2] == LINK_LEAF | (2 << LINK_COUNT_SHIFT) | 1  # (a sphere beside a triangle: an ordinary leaf)


def test_one_primitive_leaf_holding_an_instance():
    # tree 0: [interior, leaf(tri), leaf(instance 0)]; the instance's own tree: node 3
    res = check([interior(2), leaf(0, 1), leaf(1, 1), leaf(2, 2)], [0, INSTANCE | 0, 0, 0], inst_roots=[3])
    assert res["nodes"][3][2] == LINK_LEAF | LINK_OTHER | 0
    assert res["inst_slot"] == [1] and res["inst_root"] == [4]


def test_two_instances_of_one_tree():
    nodes = [interior(2), leaf(0, 1), leaf(1, 1), interior(5), leaf(2, 1), leaf(3, 1)]
    res = check(nodes, [INSTANCE | 0, INSTANCE | 1, 0, 0], inst_roots=[3, 3])
    assert res["inst_slot"] == [0, 1] and res["inst_root"] == [4, 4] and len(res["nodes"]) == 8
    assert res["nodes"][2][2] == LINK_LEAF | LINK_OTHER | 0 and res["nodes"][3][2] == LINK_LEAF | LINK_OTHER | 1


def test_an_instance_in_no_leaf_keeps_the_unseen_slot():
    res = check([leaf(0, 1), leaf(1, 1)], [0, 0], inst_roots=[1])
    assert res["inst_slot"] == [UNSEEN]


def test_the_larger_childs_block_comes_next():
    # root -> (a: small, b: large), each with two leaves: b's children take the block behind the root's children, a's the one after
    nodes = [interior(4, size=4.0), interior(3, size=1.0), leaf(0, 1), leaf(1, 1), interior(6, size=3.0), leaf(2, 1), leaf(3, 1)]
    res = check(nodes, [0] * 4)
    a, b = res["nodes"][2], res["nodes"][3]
    assert b[2] & LINK_INDEX_MASK == 4 and a[2] & LINK_INDEX_MASK == 6
    # equal areas: the first child's
    nodes[1], nodes[4] = interior(3, size=2.0), interior(6, size=2.0)
    res = check(nodes, [0] * 4)
    assert res["nodes"][2][2] & LINK_INDEX_MASK == 4 and res["nodes"][3][2] & LINK_INDEX_MASK == 6


def test_two_instance_primitives_sharing_one_record_are_refused():
    with pytest.raises(RuntimeError, match="two instance primitives share one ShmInstance record"):
        oracle_py.bvh_pairs([interior(2), leaf(0, 1), leaf(1, 1), leaf(2, 1)], [INSTANCE | 0, INSTANCE | 0, 0], inst_roots=[3])


def test_a_root_inside_another_tree_is_refused():
    with pytest.raises(RuntimeError, match="root node lies inside another tree"):
        oracle_py.bvh_pairs([interior(2), leaf(0, 1), leaf(1, 1)], [INSTANCE | 0, 0], inst_roots=[2])


def test_malformed_arrays_are_refused():
    with pytest.raises(RuntimeError, match="instance root node out of range"):
        oracle_py.bvh_pairs([leaf(0, 1)], [0], inst_roots=[5])
    with pytest.raises(RuntimeError, match="not a depth-first tree"):
        oracle_py.bvh_pairs([interior(7), leaf(0, 1), leaf(1, 1)], [0, 0])
