"""mp2g_tree_shape_touched through libmp2gpu.so and TreeShape.touched against the plain parent walk of tests/tree_touched_cases.py,
and every refusal of the four update calls (mp2g_cells_tree_hashes_rows[_dev], mp2g_row_tree_hashes_update[_dev]): each is decided
on the host, with a message, before a context is needed. The library loads without a GPU; nothing here launches anything."""
import ctypes
import importlib

import numpy as np
import pytest

import tree_cases as TC
import tree_touched_cases as TT

IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
P = 0xFFFFFFFF00000001
U32 = ctypes.c_uint32


@pytest.mark.parametrize("name", ["sbbst0", "sbbst1", "sbbst7", "sbbst70", "balanced33", "balanced65", "random300", "left40", "right40", "forest3"])
def test_touched_is_the_parent_walk(mp2, name):
    left, right = TC.accepted(small=True)[name]
    s = IX.TreeShape.from_children(left, right)
    height = TC.describe(left, right)[0]
    for what, t in TT.touched_sets(len(left), 0x7C + len(left)):
        got = s.touched(t)
        assert got.dtype == np.uint32 and got.tolist() == TT.closure(left, right, t)[0], (name, what)
        keys = [(height[i], i) for i in got.tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), (name, what)  # by height, then by index, nothing twice


def test_count_only_and_cap_too_small(mp2):
    lib = mp2.load()
    left, right = TC.sbbst(70)
    s = IX.TreeShape.sbbst(70)
    t = np.array([0, 69, 33, 0], dtype=np.uint32)
    want = TT.closure(left, right, t)[0]
    n = U32(12345)
    assert lib.mp2g_tree_shape_touched(s.h, mp2._p(t), U32(4), None, U32(0), ctypes.byref(n)) == 0 and n.value == len(want)
    out = np.full(len(want) + 1, 0xABCD, dtype=np.uint32)
    n = U32(0)
    assert lib.mp2g_tree_shape_touched(s.h, mp2._p(t), U32(4), mp2._p(out), U32(len(want) - 1), ctypes.byref(n)) != 0
    assert b"cap" in lib.mp2g_last_error() and n.value == len(want) and (out == 0xABCD).all()  # the count is set, nothing is written
    assert lib.mp2g_tree_shape_touched(s.h, mp2._p(t), U32(4), mp2._p(out), U32(len(want)), ctypes.byref(n)) == 0
    assert out[:-1].tolist() == want and out[-1] == 0xABCD
    # the empty list, with and without a pointer
    n = U32(9)
    assert lib.mp2g_tree_shape_touched(s.h, None, U32(0), None, U32(0), ctypes.byref(n)) == 0 and n.value == 0
    assert s.touched([]).size == 0 and IX.TreeShape.sbbst(0).touched([]).size == 0


def test_touched_refusals(mp2):
    lib = mp2.load()
    s = IX.TreeShape.sbbst(7)
    n = U32(0)
    for bad in (7, 8, 2 ** 32 - 1):
        with pytest.raises(mp2.Mp2gError, match=f"touched index {bad} "):
            s.touched([3, bad])
    assert s.touched([3, 0]).tolist() == TT.closure(*TC.sbbst(7), [3, 0])[0]  # a refusal leaves nothing behind in the shape
    with pytest.raises(mp2.Mp2gError, match="touched index 0 "):
        IX.TreeShape.sbbst(0).touched([0])
    assert lib.mp2g_tree_shape_touched(s.h, None, U32(2), None, U32(0), ctypes.byref(n)) != 0 and b"touched list" in lib.mp2g_last_error()
    assert lib.mp2g_tree_shape_touched(None, None, U32(0), None, U32(0), ctypes.byref(n)) != 0 and b"shape" in lib.mp2g_last_error()
    assert lib.mp2g_tree_shape_touched(s.h, None, U32(0), None, U32(0), None) != 0 and b"n_nodes" in lib.mp2g_last_error()


def test_fused_width(mp2):
    w = mp2.row_tree_update_fused_width()
    assert w >= 16 and w == mp2.load().mp2g_row_tree_update_fused_width()


def test_cells_rows_arguments_refused_without_a_context(mp2):
    lib = mp2.load()
    v = np.zeros((3, 2, 8), dtype=np.uint32)
    roots = np.zeros((3, 4), dtype=np.uint64)
    host = lambda ids, idx, variant=0, values=v: IX.cells_tree_hashes_rows(None, ids, values, idx, np.zeros((values.shape[0], 4), dtype=np.uint64), None, variant)
    dev = lambda ids, idx, variant=0, rows=3, d_roots=None, d_nodes=None: mp2.cells_tree_hashes_rows_dev(None, variant, ids, None, rows, idx, d_roots, d_nodes)
    # what the full calls refuse
    for call in (host, dev):
        with pytest.raises(mp2.Mp2gError, match="variant"):
            call([1, 2], [0], variant=2)
        for bad in (P, 2 ** 64 - 1):
            with pytest.raises(mp2.Mp2gError, match="not canonical"):
                call([1, bad], [0])
    with pytest.raises(mp2.Mp2gError, match="n_cols"):
        host(np.arange(257), [0], values=np.zeros((1, 257, 8), dtype=np.uint32))
    with pytest.raises(mp2.Mp2gError, match="n_cols"):
        dev([], [0])
    with pytest.raises(mp2.Mp2gError, match="rows"):
        dev([1, 2], [0], rows=(1 << 31) + 1)
    # a row index out of range, named; a list that is missing
    for call in (host, dev):
        for bad in (3, 2 ** 32 - 1):
            with pytest.raises(mp2.Mp2gError, match=f"row index {bad} "):
                call([1, 2], [0, bad, 1])
    ids = np.array([1, 2], dtype=np.uint64)
    for f, extra in ((lib.mp2g_cells_tree_hashes_rows, (mp2._p(v),)), (lib.mp2g_cells_tree_hashes_rows_dev, (None,))):
        assert f(None, 0, mp2._p(ids), 2, *extra, U32(3), None, U32(2), mp2._p(roots), None) != 0
        assert b"row_idx" in lib.mp2g_last_error()
    # misaligned digest buffers (device addresses are never read here)
    with pytest.raises(mp2.Mp2gError, match="16-byte aligned"):
        dev([1, 2], [0], d_roots=0x1008)
    with pytest.raises(mp2.Mp2gError, match="16-byte aligned"):
        dev([1, 2], [0], d_roots=0x1000, d_nodes=0x2004)
    # an empty list launches nothing and needs nothing; a well-formed call gets as far as the missing context
    assert host([1, P - 1], []) is not None
    dev([1, P - 1], [])
    with pytest.raises(mp2.Mp2gError, match="ctx"):
        host([1, P - 1], [2, 2])
    with pytest.raises(mp2.Mp2gError, match="ctx"):
        dev([1, P - 1], [2, 2], d_roots=0x1000)


def test_row_update_arguments_refused_without_a_context(mp2):
    lib = mp2.load()
    s = IX.TreeShape.sbbst(7)
    v = np.zeros((7, 8), dtype=np.uint32)
    host = lambda ident, values, touched, variant=0: IX.row_tree_hashes_update(None, s, ident, values, None, touched, np.zeros((7, 4), dtype=np.uint64), variant)
    dev = lambda ident, stride, touched, variant=0, d_payload=None, d_hashes=None: mp2.row_tree_hashes_update_dev(None, variant, s, ident, None, stride, d_payload, touched, d_hashes)
    # what the full calls refuse
    with pytest.raises(mp2.Mp2gError, match="variant"):
        host(5, v, [0], variant=3)
    with pytest.raises(mp2.Mp2gError, match="variant"):
        dev(5, 8, [0], variant=-1)
    with pytest.raises(mp2.Mp2gError, match="not canonical"):
        host(P, v, [0])
    with pytest.raises(mp2.Mp2gError, match="not canonical"):
        dev(2 ** 64 - 1, 8, [0])
    with pytest.raises(mp2.Mp2gError, match="value_stride"):
        host(5, v[:, :7], [0])
    with pytest.raises(mp2.Mp2gError, match="value_stride"):
        dev(5, 0, [0])
    # a touched index out of range, named; a list that is missing
    for bad in (7, 2 ** 32 - 1):
        with pytest.raises(mp2.Mp2gError, match=f"touched index {bad} "):
            host(5, v, [1, bad])
        with pytest.raises(mp2.Mp2gError, match=f"touched index {bad} "):
            dev(5, 8, [bad])
    h = np.zeros((7, 4), dtype=np.uint64)
    assert lib.mp2g_row_tree_hashes_update(None, 0, s.h, ctypes.c_uint64(5), mp2._p(v), U32(8), None, None, U32(1), mp2._p(h)) != 0
    assert b"touched list" in lib.mp2g_last_error()
    assert lib.mp2g_row_tree_hashes_update_dev(None, 0, s.h, ctypes.c_uint64(5), None, U32(8), None, None, U32(1), None) != 0
    assert b"touched list" in lib.mp2g_last_error()
    # misaligned digest buffers
    with pytest.raises(mp2.Mp2gError, match="16-byte aligned"):
        dev(5, 8, [0], d_hashes=0x1008)
    with pytest.raises(mp2.Mp2gError, match="16-byte aligned"):
        dev(5, 8, [0], d_payload=0x2004, d_hashes=0x1000)
    # the empty list launches nothing and needs nothing, on the empty shape too; a well-formed call gets as far as the missing context
    assert not host(P - 1, v, []).any()
    dev(P - 1, 8, [])
    e = IX.TreeShape.sbbst(0)
    assert IX.row_tree_hashes_update(None, e, 5, v[:0], None, [], np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)
    with pytest.raises(mp2.Mp2gError, match="touched index 0 "):
        IX.row_tree_hashes_update(None, e, 5, v[:0], None, [0], np.zeros((0, 4), dtype=np.uint64))
    with pytest.raises(mp2.Mp2gError, match="ctx"):
        host(P - 1, v, [0, 0])
    with pytest.raises(mp2.Mp2gError, match="ctx"):
        dev(P - 1, 8, [6], d_hashes=0x1000)
