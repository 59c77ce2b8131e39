"""Case tables for the accumulated-digest kernels (csrc/tree_digest.hip): tree shapes, the points at their nodes and the touched
sets of the updates, with every node's expected digest from the CPU oracle. No GPU is used here and nothing here calls the code
under test: tests/test_tree_digest_cases.py checks the tables on the references alone, tests/test_gpu_tree_digests.py feeds the
same arrays to the device.

expected() accumulates the way SplitDigestPoint::accumulate does, node by node from the leaves up, each step one oracle sum of at
most three encodings; subtree_sum() is the oracle's sum over a node's whole subtree in one call. The host test proves the two equal
for every node of every case, so the GPU tests may use the cheap one.

The builders are seeded and cached: every caller gets the same arrays and must leave them unchanged."""
import functools

import numpy as np

import ec_cases as EC
import tree_cases as TC
import tree_touched_cases as TT


def isolated(n):
    return [-1] * n, [-1] * n


# name -> (left, right). IN_ORDER: the shapes whose node index is the in-order position, so that a subtree is the contiguous range
# [min_idx, max_idx] and curve_sum_ranges can sum it
SHAPES = {"empty": ([], []), "one": TC.sbbst(1)}
SHAPES.update({f"sbbst{n}": TC.sbbst(n) for n in (2, 3, 7, 8, 37, 300)})
SHAPES["right_only"] = ([-1, -1], [1, -1])
SHAPES["left40"], SHAPES["right40"] = TC.chain(40, 0), TC.chain(40, 1)
SHAPES.update({f"isolated{n}": isolated(n) for n in (127, 128, 129)})
SHAPES["forest3"] = TC.forest3()
SHAPES["random300"] = TC.random_bst(300, 0x5EED)
SHAPES["balanced33"] = TC.balanced(33)
IN_ORDER = ["one", "sbbst2", "sbbst3", "sbbst7", "sbbst8", "sbbst37", "sbbst300", "right_only", "right40", "isolated127", "isolated128",
            "isolated129", "forest3", "balanced33"]
PATTERNS = ["random", "neutral", "neutral_inner", "child_negates", "doubling", "subtrees_cancel"]
# the full-pass cases: every shape with random points, every pattern on the shapes that have the nodes the pattern needs
FULL_CASES = [(s, "random") for s in SHAPES] + [(s, p) for s in ("sbbst3", "sbbst7", "sbbst37", "right_only", "forest3", "left40") for p in PATTERNS[1:]]


def subtree(left, right, i):
    out, stack = [], [i]
    while stack:
        k = stack.pop()
        out.append(k)
        stack += [c for c in (left[k], right[k]) if c >= 0]
    return sorted(out)


def by_height(left, right):
    height = TC.describe(left, right)[0]
    return sorted(range(len(left)), key=lambda i: (height[i], i)), height


def _own(left, right, pattern, shift=0):
    """encodings [n][5]. The structured patterns plant their relation at the nodes whose (first) child is a leaf, where the child's
    accumulated digest is its own:
      neutral_inner    every node with a child holds the neutral point
      child_negates    own[i] = -own[c]: own[i] + acc[c] is the neutral point, made by cancellation, and meets the other child
      doubling         own[i] = own[c]: the first addition doubles through pt_add
      subtrees_cancel  two leaf children hold P and -P; a node with one leaf child holds -own[c] as in child_negates"""
    n = len(left)
    b = EC.base_points(512)
    own = b[(np.arange(n) + shift) % 512].copy() if n else np.zeros((0, 5), dtype=np.uint64)
    if pattern == "random":
        return own
    if pattern == "neutral":
        return np.zeros((n, 5), dtype=np.uint64)
    height = TC.describe(left, right)[0]
    for i in range(n):
        kids = [c for c in (left[i], right[i]) if c >= 0]
        if not kids:
            continue
        leaf_kids = [c for c in kids if height[c] == 0]
        if pattern == "neutral_inner":
            own[i] = 0
        elif pattern == "child_negates" and leaf_kids:
            own[i] = EC.negate(own[leaf_kids[0]])
        elif pattern == "doubling" and leaf_kids:
            own[i] = own[leaf_kids[0]]
        elif pattern == "subtrees_cancel" and leaf_kids:
            if len(leaf_kids) == 2:
                own[leaf_kids[1]] = EC.negate(own[leaf_kids[0]])
            else:
                own[i] = EC.negate(own[leaf_kids[0]])
    return own


@functools.lru_cache(maxsize=None)
def own_points(shape, pattern):
    own = _own(*SHAPES[shape], pattern)
    own.setflags(write=False)
    return own


def expected(left, right, own):
    """(encodings [n][5], Weierstrass [n][11]) of every node's accumulated digest, bottom-up by the oracle"""
    n = len(left)
    w, wei = np.zeros((n, 5), dtype=np.uint64), np.zeros((n, 11), dtype=np.uint64)
    for i in by_height(left, right)[0]:
        w[i], wei[i] = EC.orc_sum(np.stack([own[i]] + [w[c] for c in (left[i], right[i]) if c >= 0]))
    return w, wei


def subtree_sum(left, right, own, i):
    return EC.orc_sum(np.asarray(own)[subtree(left, right, i)])


@functools.lru_cache(maxsize=None)
def full_expected(shape, pattern):
    out = expected(*SHAPES[shape], own_points(shape, pattern))
    for a in out:
        a.setflags(write=False)
    return out


# ---- updates ----------------------------------------------------------------------------------------------------------------------
UPDATE_SHAPES = dict(SHAPES)
UPDATE_SHAPES["left300"] = TC.chain(300, 0)


def leaves(left, right):
    return [i for i in range(len(left)) if left[i] < 0 and right[i] < 0]


def width_touched(width):
    """`width` leaves of sbbst300 (it has 150): the closure's widest level is its lowest and has exactly `width` nodes"""
    lv = leaves(*SHAPES["sbbst300"])
    assert width <= len(lv)
    return lv[:width]


def update_cases(fused_width=None):
    """[(label, shape, touched)]; with fused_width = mp2g_tree_digests_update_fused_width() also the two cases around it (the last
    closure the fused kernel takes and the first that goes level by level)"""
    out = []
    for shape in ("one", "sbbst8", "sbbst37", "forest3", "right_only", "left40", "random300"):
        left, right = UPDATE_SHAPES[shape]
        roots = TC.describe(left, right)[3]
        lv = leaves(left, right)
        out += [(f"{shape}: nothing", shape, []), (f"{shape}: a leaf", shape, [lv[-1]]), (f"{shape}: the root", shape, [roots[0]]),
                (f"{shape}: duplicates", shape, [lv[0], roots[-1], lv[0], lv[-1], lv[-1]])]
    out += [(f"{shape}: every node", shape, list(range(len(UPDATE_SHAPES[shape][0])))) for shape in ("sbbst37", "isolated129", "sbbst300")]
    out.append(("left300: the end of the chain", "left300", [299]))
    if fused_width is not None:
        out += [(f"sbbst300: {w} leaves", "sbbst300", width_touched(w)) for w in (fused_width, fused_width + 1)]
    return out


def changed_own(shape, touched):
    """own after the change: the random points of the shape, fresh points at the touched nodes"""
    left, right = UPDATE_SHAPES[shape]
    own = _own(left, right, "random")
    t = sorted(set(int(x) for x in touched))
    if t:
        own[t] = _own(left, right, "random", shift=211)[t]
    return own


def old_own(shape):
    return _own(*UPDATE_SHAPES[shape], "random")


def closure_mask(left, right, touched):
    """(in the closure, may hold garbage on entry): garbage is allowed at the entries that are neither in the closure nor a child
    of a closure node, since the update reads nothing else"""
    n = len(left)
    inside = np.zeros(n, dtype=bool)
    inside[TT.closure(left, right, touched)[0]] = True
    read = inside.copy()
    for i in np.flatnonzero(inside):
        for c in (left[i], right[i]):
            if c >= 0:
                read[c] = True
    return inside, ~read


def insertion_case():
    """the index tree growing by one node: (old shape, new shape, touched) with touched = the new node and every node whose children
    differ between sbbst(36) and sbbst(37)"""
    old, new = TC.sbbst(36), TC.sbbst(37)
    touched = [36] + [i for i in range(36) if (old[0][i], old[1][i]) != (new[0][i], new[1][i])]
    return old, new, touched
