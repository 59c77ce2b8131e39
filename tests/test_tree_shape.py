"""mp2g_tree_shape_* through libmp2gpu.so and indexing.TreeShape: the accepted and refused forests of tests/tree_cases.py at small
sizes against the Python restatement, and the argument refusals of the four node-hash calls that are decided before a context is
needed. The library loads without a GPU (as test_abi_symbols relies on); nothing here launches anything."""
import importlib

import numpy as np
import pytest

import tree_cases as TC

IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
P = 0xFFFFFFFF00000001


def check(shape, left, right):
    d = {k: v.tolist() for k, v in shape.describe().items()}
    TC.check_shape(left, right, d["left"], d["right"], d["height"], d["min_idx"], d["max_idx"], d["roots"])
    assert shape.size == len(left) and shape.num_roots == len(d["roots"])
    assert shape.num_levels == (max(d["height"]) + 1 if left else 0)


@pytest.mark.parametrize("name", list(TC.accepted(small=True)))
def test_accepted_shapes(mp2, name):
    left, right = TC.accepted(small=True)[name]
    check(IX.TreeShape.from_children(left, right), left, right)


def test_sbbst_is_table_py(mp2):
    for n in range(0, 71):
        left, right = TC.sbbst(n)
        s = IX.TreeShape.sbbst(n)
        check(s, left, right)
        assert s.describe()["roots"].tolist() == ([TC.T.sbbst_root(n) - 1] if n else [])


def test_deep_chain_needs_no_recursion(mp2):
    n = 1 << 16
    s = IX.TreeShape.from_children(*TC.chain(n, 1))
    d = s.describe()
    assert s.num_levels == n and d["height"][0] == n - 1 and d["max_idx"][0] == n - 1 and d["min_idx"][0] == 0


@pytest.mark.parametrize("name,left,right", TC.REFUSED, ids=[c[0] for c in TC.REFUSED])
def test_malformed_children_are_refused(mp2, name, left, right):
    with pytest.raises(mp2.Mp2gError, match="invalid tree shape"):
        IX.TreeShape.from_children(left, right)


def test_sbbst_size_limit(mp2):
    with pytest.raises(mp2.Mp2gError, match="n <="):
        IX.TreeShape.sbbst(1 << 31)


def test_cells_arguments_refused_without_a_context(mp2):
    v = np.zeros((3, 2, 8), dtype=np.uint32)
    with pytest.raises(mp2.Mp2gError, match="variant"):
        IX.cells_tree_hashes(None, [1, 2], v, variant=2)
    with pytest.raises(mp2.Mp2gError, match="n_cols"):
        IX.cells_tree_hashes(None, np.arange(257), np.zeros((1, 257, 8), dtype=np.uint32))
    with pytest.raises(mp2.Mp2gError, match="n_cols"):
        mp2.cells_tree_hashes_dev(None, 0, [], None, 3, None)
    with pytest.raises(mp2.Mp2gError, match="n_cols"):
        IX.cells_tree_hashes(None, [], np.zeros((3, 0, 8), dtype=np.uint32))
    for bad in (P, 2 ** 64 - 1):
        with pytest.raises(mp2.Mp2gError, match="not canonical"):
            IX.cells_tree_hashes(None, [1, bad], v)
        with pytest.raises(mp2.Mp2gError, match="not canonical"):
            mp2.cells_tree_hashes_dev(None, 0, [bad, 2], None, 3, None)
    with pytest.raises(mp2.Mp2gError, match="variant"):
        mp2.cells_tree_hashes_dev(None, -1, [1, 2], None, 3, None)
    with pytest.raises(mp2.Mp2gError, match="rows"):
        mp2.cells_tree_hashes_dev(None, 0, [1, 2], None, (1 << 31) + 1, None)
    # rows == 0 launches nothing and needs nothing
    assert IX.cells_tree_hashes(None, [1, P - 1], v[:0]).shape == (0, 4)
    # well-formed arguments get as far as the missing context
    with pytest.raises(mp2.Mp2gError, match="ctx"):
        IX.cells_tree_hashes(None, [1, P - 1], v)


def test_row_tree_arguments_refused_without_a_context(mp2):
    s = IX.TreeShape.sbbst(7)
    v = np.zeros((7, 8), dtype=np.uint32)
    with pytest.raises(mp2.Mp2gError, match="variant"):
        IX.row_tree_hashes(None, s, 5, v, variant=3)
    with pytest.raises(mp2.Mp2gError, match="not canonical"):
        IX.row_tree_hashes(None, s, P, v)
    with pytest.raises(mp2.Mp2gError, match="value_stride"):
        IX.row_tree_hashes(None, s, 5, v[:, :7])
    with pytest.raises(mp2.Mp2gError, match="value_stride"):
        mp2.row_tree_hashes_dev(None, 0, s, 5, None, 0, None, None)
    with pytest.raises(mp2.Mp2gError, match="not canonical"):
        mp2.row_tree_hashes_dev(None, 0, s, 2 ** 64 - 1, None, 8, None, None)
    assert IX.row_tree_hashes(None, IX.TreeShape.sbbst(0), 5, v[:0]).shape == (0, 4)  # the empty shape
    with pytest.raises(mp2.Mp2gError, match="ctx"):
        IX.row_tree_hashes(None, s, P - 1, v)
