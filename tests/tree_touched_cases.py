"""What ryhope's touched() (ryhope/src/lib.rs:216-222) means for a forest given as (left, right) lists: the given nodes and all
their ancestors, by a plain parent walk, and the touched sets the tests of tree_shape_touched use. A helper module: nothing here
touches the library, and nothing here sorts or groups the way csrc/tree_shape.h does."""
import numpy as np

import tree_cases as TC


def parents(left, right):
    par = [-1] * len(left)
    for i, (l, r) in enumerate(zip(left, right)):
        for c in (l, r):
            if c >= 0:
                par[c] = i
    return par


def closure(left, right, touched):
    """(nodes by ascending height then ascending index, offsets of the heights that occur)"""
    par, taken = parents(left, right), set()
    for t in touched:
        i = int(t)
        while i >= 0:  # all the way up, every time: no early exit to share with the library
            taken.add(i)
            i = par[i]
    height = TC.describe(left, right)[0]
    nodes, off = [], [0]
    for h in sorted({height[i] for i in taken}):
        nodes += sorted(i for i in taken if height[i] == h)
        off.append(len(nodes))
    return nodes, off


def touched_sets(n, seed):
    """[(name, list)]: empty, random subsets, a list with duplicates, all nodes; each single node for n <= 70"""
    rng = np.random.default_rng(seed)
    sets = [("empty", [])]
    if n:
        sets += [(f"random{k}", rng.choice(n, size=min(n, k), replace=False).tolist()) for k in (1, 3, 17)]
        sets.append(("duplicates", rng.integers(0, n, size=2 * min(n, 9) + 1).tolist() * 2))
        sets.append(("all", list(range(n))))
        if n <= 70:
            sets += [(f"single{i}", [i]) for i in range(n)]
    return sets
