"""tests/tree_digest_cases.py says what it claims: the expected digests are the oracle's sums over the subtrees, they agree with
Python integers, the predicted closures are the library's (mp2g_tree_shape_touched is host work), and the width cases have the widest
levels they are named after. No GPU."""
import numpy as np
import pytest

import ec_cases as EC
import tree_cases as TC
import tree_digest_cases as TD
import tree_touched_cases as TT


@pytest.mark.parametrize("shape,pattern", TD.FULL_CASES, ids=lambda v: str(v))
def test_expected_is_the_oracles_sum_over_the_subtree(shape, pattern):
    left, right = TD.SHAPES[shape]
    own, (w, wei) = TD.own_points(shape, pattern), TD.full_expected(shape, pattern)
    assert own.shape == (len(left), 5) and w.shape == (len(left), 5) and wei.shape == (len(left), 11)
    for i in range(len(left)):
        sw, swei = TD.subtree_sum(left, right, own, i)
        assert np.array_equal(w[i], sw) and np.array_equal(wei[i], swei), (shape, pattern, i)


@pytest.mark.parametrize("shape,pattern", [c for c in TD.FULL_CASES if c[0] != "empty"], ids=lambda v: str(v))
def test_one_node_per_case_on_python_integers(shape, pattern):
    """the highest node whose subtree has at most 3 nodes: the one the structured patterns plant their relation at"""
    left, right = TD.SHAPES[shape]
    order, _ = TD.by_height(left, right)
    i = [k for k in order if len(TD.subtree(left, right, k)) <= 3][-1]
    own, (w, wei) = TD.own_points(shape, pattern), TD.full_expected(shape, pattern)
    ew, ewei = EC.exact_sum(own[TD.subtree(left, right, i)])
    assert [int(x) for x in w[i]] == ew and [int(x) for x in wei[i]] == ewei


def test_the_patterns_plant_what_they_name():
    left, right = TD.SHAPES["sbbst7"]  # node 1 has the leaves 0 and 2, node 3 is the root
    w = {p: TD.full_expected("sbbst7", p)[0] for p in TD.PATTERNS}
    own = {p: TD.own_points("sbbst7", p) for p in TD.PATTERNS}
    assert not w["neutral"].any()
    assert not own["neutral_inner"][[1, 3, 5]].any() and own["neutral_inner"][[0, 2, 4, 6]].any(axis=1).all()
    assert np.array_equal(w["child_negates"][1], own["child_negates"][2])  # own + left = 0, + right
    assert np.array_equal(own["doubling"][1], own["doubling"][0])
    assert np.array_equal(w["subtrees_cancel"][1], own["subtrees_cancel"][1])  # the two leaves cancel
    assert np.array_equal(own["subtrees_cancel"][2], EC.negate(own["subtrees_cancel"][0]))


@pytest.mark.parametrize("shape", TD.IN_ORDER)
def test_in_order_shapes_have_contiguous_subtrees(shape):
    left, right = TD.SHAPES[shape]
    _, mn, mx, _ = TC.describe(left, right)
    for i in range(len(left)):
        assert TD.subtree(left, right, i) == list(range(mn[i], mx[i] + 1))


def test_predicted_closures_are_the_librarys(mp2):
    W = mp2.tree_digests_update_fused_width()
    for label, shape, touched in TD.update_cases(W):
        left, right = TD.UPDATE_SHAPES[shape]
        s = mp2.TreeShape.from_children(left, right)
        assert s.touched(touched).tolist() == TT.closure(left, right, touched)[0], label
        s.free()
    old, new, touched = TD.insertion_case()
    s = mp2.TreeShape.from_children(*new)
    assert s.touched(touched).tolist() == TT.closure(*new, touched)[0]
    assert s.describe()["left"].tolist() == new[0] and len(old[0]) == 36
    s.free()


def test_width_cases_have_the_widest_levels_they_name(mp2):
    W = mp2.tree_digests_update_fused_width()
    left, right = TD.SHAPES["sbbst300"]
    for width in (W, W + 1):
        off = TT.closure(left, right, TD.width_touched(width))[1]
        assert max(b - a for a, b in zip(off, off[1:])) == width
    assert len(TT.closure(*TD.UPDATE_SHAPES["left300"], [299])[1]) - 1 == 300  # more levels than one fused launch takes
    labels = [c[0] for c in TD.update_cases(W)]
    assert f"sbbst300: {W} leaves" in labels and f"sbbst300: {W + 1} leaves" in labels


def test_update_expectations_differ_only_inside_the_closure(mp2):
    """the oracle's view of what a change reaches, and which entries an update may find garbage in"""
    for label, shape, touched in TD.update_cases(mp2.tree_digests_update_fused_width()):
        left, right = TD.UPDATE_SHAPES[shape]
        if len(left) > 40:
            continue
        before, after = TD.expected(left, right, TD.old_own(shape))[0], TD.expected(left, right, TD.changed_own(shape, touched))[0]
        inside, garbage = TD.closure_mask(left, right, touched)
        assert np.array_equal(before[~inside], after[~inside]), label
        assert not (inside & garbage).any()
        for i in np.flatnonzero(inside):
            assert not any(c >= 0 and garbage[c] for c in (left[i], right[i])), label
        if touched:
            assert (before[inside] != after[inside]).any(axis=1).all(), label
