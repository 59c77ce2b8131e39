"""Binary forests for the tree-shape and index-hash tests, as (left, right) lists with -1 for a missing child, and a plain recursive
Python restatement of what csrc/tree_shape.h computes from them. A helper module: nothing here touches the library."""
import importlib
import sys

import numpy as np

T = importlib.import_module("mapreduce-plonky2_amd.table")


def sbbst(n):
    """ryhope's sbbst over positions 1..n from table.py's restatement; position k = node k - 1"""
    ch = [T.sbbst_children(n, k) for k in range(1, n + 1)]
    return [(-1 if l is None else l - 1) for l, _ in ch], [(-1 if r is None else r - 1) for _, r in ch]


def balanced(n):
    _, nodes, _ = T.balanced_bst(n)
    return [(-1 if nodes[k][0] is None else nodes[k][0]) for k in range(n)], [(-1 if nodes[k][1] is None else nodes[k][1]) for k in range(n)]


def random_bst(n, seed):
    """the BST that inserting a random permutation of n keys gives; node = order of insertion"""
    keys = np.random.default_rng(seed).permutation(n).tolist()
    left, right = [-1] * n, [-1] * n
    for i in range(1, n):
        at = 0
        while True:
            side = left if keys[i] < keys[at] else right
            if side[at] < 0:
                side[at] = i
                break
            at = side[at]
    return left, right


def chain(n, side):
    """node i's only child is i + 1, on the left (side 0) or the right (side 1)"""
    down = [i + 1 for i in range(n - 1)] + [-1]
    return (down, [-1] * n) if side == 0 else ([-1] * n, down)


def forest3():
    """three trees side by side: an sbbst of 5 (nodes 0..4), a single node (5) and a right chain of 3 (6..8)"""
    l, r = sbbst(5)
    return l + [-1, -1, -1, -1], r + [-1, 7, 8, -1]


def accepted(small):
    """{name: (left, right)}: the shapes of the host test; `small`: only those of at most 300 nodes (all but balanced1000)"""
    cases = {f"sbbst{n}": sbbst(n) for n in range(0, 71)}
    cases.update({f"balanced{n}": balanced(n) for n in list(range(1, 34)) + [64, 65] + ([] if small else [1000])})
    cases["random300"] = random_bst(300, 0x5EED)
    cases["left40"], cases["right40"] = chain(40, 0), chain(40, 1)
    cases["forest3"] = forest3()
    assert not small or all(len(l) <= 300 for l, _ in cases.values())
    return cases


# (name, left, right): each is refused
REFUSED = [
    ("child_is_n", [1, -1, -1], [2, 3, -1]),
    ("child_minus_2", [1, -1], [-2, -1]),
    ("self_child", [1, 1], [-1, -1]),
    ("two_parents", [2, 2, -1], [-1, -1, -1]),
    ("left_equals_right", [1, -1], [1, -1]),
    ("cycle_alone", [1, 0], [-1, -1]),
    ("cycle_beside_a_tree", [1, 0, 3, -1, -1], [-1, -1, 4, -1, -1]),
]


def describe(left, right):
    """heights, min_idx, max_idx, roots by the definitions, node by node (recursive on purpose: not the library's schedule)"""
    n = len(left)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 1000))
    height, mn, mx = [None] * n, [None] * n, [None] * n

    def h(i):
        if height[i] is None:
            height[i] = 1 + max([h(c) for c in (left[i], right[i]) if c >= 0], default=-1)
        return height[i]

    def lo(i):
        if mn[i] is None:
            mn[i] = lo(left[i]) if left[i] >= 0 else i
        return mn[i]

    def hi(i):
        if mx[i] is None:
            mx[i] = hi(right[i]) if right[i] >= 0 else i
        return mx[i]

    for i in range(n):
        h(i), lo(i), hi(i)
    children = {c for c in left + right if c >= 0}
    return height, mn, mx, [i for i in range(n) if i not in children]


def check_shape(left, right, got_left, got_right, height, mn, mx, roots):
    """what every accepted case must satisfy, against describe()"""
    want = describe(left, right)
    assert (list(got_left), list(got_right)) == (list(left), list(right))
    assert (list(height), list(mn), list(mx), list(roots)) == tuple(list(w) for w in want)
    assert list(roots) == sorted(roots)
    for i in range(len(left)):
        for c in (left[i], right[i]):
            assert c < 0 or height[c] < height[i]
