"""mp2g_row_tree_hashes_update / mp2g_cells_tree_hashes_rows (csrc/index_hash.hip, csrc/index_api.hip) and indexing.TableHashes
against the recursive Python walks of tests/test_gpu_index_hashes.py over the oracle's sponge. The walks hash every node of the
changed table from scratch; they share nothing with the library's closure (tree_shape_touched) or its schedule (one fused launch
for narrow closures under Poseidon2, one launch per closure level otherwise). Equality is exact everywhere.

Per row-tree case: H0 is the walk of a table T0, T1 is T0 with value and payload changed at the touched nodes, `want` the walk of
T1. (1) the update of a buffer holding H0 gives `want` at every node; (2) with junk in the closure's entries and `want` elsewhere
it gives `want`, so every closure node is rewritten; (3) with a sentinel in every entry outside the closure, those entries still
hold it afterwards, so nothing else is written."""
import importlib

import numpy as np
import pytest

import oracle as O
import tree_cases as TC
import tree_touched_cases as TT
from test_gpu_index_hashes import ZERO, cells_walk, edge_values, row_walk

pytestmark = pytest.mark.gpu

IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
T = TC.T
JUNK, SENTINEL = np.uint64(0x0BAD0BAD0BAD0BAD), np.uint64(0x5E5E5E5E5E5E5E5E)
SHAPES = [f"sbbst{n}" for n in (0, 1, 2, 3, 7, 8, 64, 65, 70)] + [f"balanced{n}" for n in (1, 2, 33, 65)] + ["random300", "left40", "right40", "forest3"]


def walk(left, right, ident, values, payload, variant):
    """row_walk over arrays: values uint32 [n][8], payload uint64 [n][4] or None"""
    return row_walk(left, right, ident, lambda i: [int(x) for x in values[i]], (lambda i: ZERO) if payload is None else (lambda i: [int(x) for x in payload[i]]), variant)


def changed(values, payload, touched, seed):
    """T1: fresh limbs and payload words at the touched nodes"""
    rng = np.random.default_rng(seed)
    v, p = values.copy(), payload.copy()
    t = sorted(set(int(x) for x in touched))
    v[t] = rng.integers(0, 1 << 32, size=(len(t), 8), dtype=np.uint32)
    p[t] = O.rand_field((len(t), 4), seed + 1)
    return v, p


class RowCase:
    """one shape with its table on the host; update() runs the _dev call on a given buffer and reads it back"""

    def __init__(self, ctx, mp2, left, right, seed):
        self.ctx, self.mp2, self.left, self.right, self.n = ctx, mp2, left, right, len(left)
        self.shape = IX.TreeShape.from_children(left, right)
        self.values = edge_values(self.n, 1, seed).reshape(self.n, 8)
        self.payload = O.rand_field((self.n, 4), seed + 1).reshape(self.n, 4)
        self.ident = int(O.rand_field(1, seed + 2)[0])
        self.h0 = {}

    def H0(self, variant):
        if variant not in self.h0:
            self.h0[variant] = walk(self.left, self.right, self.ident, self.values, self.payload, variant)
        return self.h0[variant]

    def update_dev(self, values, payload, touched, buf, variant):
        d_v, d_p, d_h = self.ctx.to_device(values), self.ctx.to_device(payload), self.ctx.to_device(buf)
        self.mp2.row_tree_hashes_update_dev(self.ctx, variant, self.shape, self.ident, d_v, 8, d_p, touched, d_h)
        out = d_h.download(buf.shape)
        for d in (d_v, d_p, d_h):
            d.free()
        return out

    def check(self, touched, variant, seed, what):
        n = self.n
        v1, p1 = changed(self.values, self.payload, touched, seed)
        want = walk(self.left, self.right, self.ident, v1, p1, variant) if len(touched) else self.H0(variant)
        closure = TT.closure(self.left, self.right, touched)[0]
        inside = np.zeros(n, dtype=bool)
        inside[closure] = True
        assert np.array_equal(self.H0(variant)[~inside], want[~inside]), what  # the walk's own view of what a change reaches
        # (1) from H0, device form and host form
        assert np.array_equal(self.update_dev(v1, p1, touched, self.H0(variant), variant), want), what
        host = self.H0(variant).copy()
        assert IX.row_tree_hashes_update(self.ctx, self.shape, self.ident, v1, p1, touched, host, variant) is host
        assert np.array_equal(host, want), what
        # (2) junk in the closure
        buf = want.copy()
        buf[inside] = JUNK
        assert np.array_equal(self.update_dev(v1, p1, touched, buf, variant), want), what
        # (3) a sentinel outside it
        buf = want.copy()
        buf[~inside] = SENTINEL
        got = self.update_dev(v1, p1, touched, buf, variant)
        assert (got[~inside] == SENTINEL).all(), what
        if not len(touched):
            assert np.array_equal(got, buf), what  # the empty list: the buffer as it was
        return want, v1, p1


@pytest.mark.parametrize("name", SHAPES)
def test_row_tree_updates(ctx, mp2, name):
    left, right = TC.accepted(small=True)[name]
    n = len(left)
    case = RowCase(ctx, mp2, left, right, 0x0DD + n)
    if n == 0:  # the empty shape: only the empty list, nothing launched
        assert IX.row_tree_hashes_update(ctx, case.shape, 5, np.zeros((0, 8), dtype=np.uint32), None, [], np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)
        return
    height, _, _, roots = TC.describe(left, right)
    leaf = max(i for i in range(n) if height[i] == 0)
    sets = {"one leaf": [leaf], "the root alone": [roots[0]], "all nodes": list(range(n)), "the empty list": []}
    if name == "forest3":
        sets["two of the three trees"] = [0, 8, 8]  # a leaf of the sbbst and the end of the right chain, one of them twice
    for variant in (0, 1):
        for j, (what, touched) in enumerate(sets.items()):
            want, v1, p1 = case.check(touched, variant, 0x5EED + 16 * j + variant, (name, what, variant))
            if what == "all nodes":
                assert np.array_equal(IX.row_tree_hashes(ctx, case.shape, case.ident, v1, p1, variant), want)
    case.shape.free()


@pytest.fixture(scope="module")
def balanced4097(ctx, mp2):
    case = RowCase(ctx, mp2, *TC.balanced(4097), 0xB16)
    yield case
    case.shape.free()


@pytest.mark.parametrize("extra", [0, 1])
def test_the_last_fused_and_the_first_per_level_closure(ctx, mp2, balanced4097, extra):
    """exactly W and W + 1 touched nodes of height 0 in balanced(4097): the closure's widest level is its lowest, so under
    Poseidon2 these are the widest closure the fused kernel takes and the narrowest that goes level by level"""
    case = balanced4097
    w = mp2.row_tree_update_fused_width()
    height = TC.describe(case.left, case.right)[0]
    leaves = [i for i in range(case.n) if height[i] == 0]
    touched = leaves[::len(leaves) // (w + 2)][:w + extra]
    assert len(touched) == w + extra
    _, off = TT.closure(case.left, case.right, touched)
    assert max(b - a for a, b in zip(off, off[1:])) == w + extra
    for variant in (0, 1):
        case.check(touched, variant, 0xF00 + extra, (len(touched), variant))


def test_a_chain_of_300_levels_goes_level_by_level(ctx, mp2):
    left, right = TC.chain(300, 0)
    case = RowCase(ctx, mp2, left, right, 0xC4A)
    assert len(TT.closure(left, right, [299])[1]) - 1 == 300  # more levels than one fused launch takes
    for variant in (0, 1):
        case.check([299], variant, 0xC4B, variant)
    case.shape.free()


def test_strides_and_bases_that_are_not_16_byte_aligned(ctx, mp2):
    """the table's column 0 read in place (value_stride = n_cols * 8), and a stride of 9 words from a base 4 bytes into its buffer"""
    left, right = TC.sbbst(70)
    shape = IX.TreeShape.from_children(left, right)
    touched = [0, 37, 69]
    payload = O.rand_field((70, 4), 0x51)
    for n_cols, words, base in ((3, 24, 0), (1, 9, 4)):
        table = edge_values(70, n_cols, 0x52 + n_cols)
        rows = np.concatenate([table.reshape(70, -1), np.full((70, words - 8 * n_cols), 0xDEADBEEF, dtype=np.uint32)], axis=1)
        col0 = np.ascontiguousarray(table[:, 0])
        for variant in (0, 1):
            h0 = walk(left, right, 9, col0, payload, variant)
            v1, p1 = changed(col0, payload, touched, 0x53)
            rows1 = rows.copy()
            rows1[:, :8] = v1
            want = walk(left, right, 9, v1, p1, variant)
            buf = ctx.alloc(rows1.nbytes + 16)
            buf.upload_at(rows1, base)
            d_p, d_h = ctx.to_device(p1), ctx.to_device(h0)
            mp2.row_tree_hashes_update_dev(ctx, variant, shape, 9, buf.ptr.value + base, words, d_p, touched, d_h)
            assert np.array_equal(d_h.download((70, 4)), want), (words, base, variant)
            if base == 0:
                host = h0.copy()
                IX.row_tree_hashes_update(ctx, shape, 9, rows1.reshape(70, n_cols, 8), p1, touched, host, variant)
                assert np.array_equal(host, want)
            for d in (buf, d_p, d_h):
                d.free()
    shape.free()


@pytest.mark.parametrize("calls", [2, 9])
def test_updates_queued_back_to_back(ctx, mp2, calls):
    """update calls with different touched lists queued with no synchronisation in between, every list passed in the SAME host
    array, which is overwritten as soon as its call has returned; then one download. 9 calls go round the context's ring of
    staging slots twice."""
    left, right = TC.balanced(65)
    shape = IX.TreeShape.from_children(left, right)
    values, payload = edge_values(65, 1, 0xB2B).reshape(65, 8), O.rand_field((65, 4), 0xB2C)
    lists = [[(7 * k + 3) % 65, (11 * k + 5) % 65, 64 - k] for k in range(calls)]
    v, p = values, payload
    for k, t in enumerate(lists):
        v, p = changed(v, p, t, 0xB2D + k)
    for variant in (0, 1):
        want = walk(left, right, 11, v, p, variant)
        d_v, d_p, d_h = ctx.to_device(v), ctx.to_device(p), ctx.to_device(walk(left, right, 11, values, payload, variant))
        lst = np.zeros(3, dtype=np.uint32)
        for t in lists:
            lst[:] = t
            mp2.row_tree_hashes_update_dev(ctx, variant, shape, 11, d_v, 8, d_p, lst, d_h)
            lst[:] = 0xFFFFFFFF  # what a later read of the caller's array would find
        assert np.array_equal(d_h.download((65, 4)), want), variant
        for d in (d_v, d_p, d_h):
            d.free()
    shape.free()


def test_the_index_tree_growing_block_by_block(ctx, mp2):
    """IndexNode::aggregate after each new block: the shape is sbbst(n), the buffer the result of step n - 1 with one entry
    appended, touched = {n - 1}; every child pointer that differs between sbbst(n - 1) and sbbst(n) belongs to an ancestor of the
    new node (asserted here), so that one entry is enough. The result is the full call's on sbbst(n)."""
    values, payload = edge_values(70, 1, 0x6B0).reshape(70, 8), O.rand_field((70, 4), 0x6B1)
    for variant in (0, 1):
        hashes = np.zeros((0, 4), dtype=np.uint64)
        prev = ([], [])
        for n in range(1, 71):
            left, right = TC.sbbst(n)
            ancestors = set(TT.closure(left, right, [n - 1])[0])
            assert all(i in ancestors for i in range(n - 1) if (left[i], right[i]) != (prev[0][i], prev[1][i]))
            prev = (left, right)
            shape = IX.TreeShape.sbbst(n)
            hashes = np.concatenate([hashes, np.full((1, 4), JUNK, dtype=np.uint64)])
            IX.row_tree_hashes_update(ctx, shape, 3, values[:n], payload[:n], [n - 1], hashes, variant)
            assert np.array_equal(hashes, IX.row_tree_hashes(ctx, shape, 3, values[:n], payload[:n], variant)), (n, variant)
            shape.free()
    assert np.array_equal(hashes, walk(left, right, 3, values, payload, 1))


# ---- cells trees of a row list --------------------------------------------------------------------------------------------------------
CELL_ROWS, CELL_COLS = (1, 65, 257), (1, 2, 5, 18)


@pytest.fixture(scope="module")
def cells_table():
    return O.rand_field(max(CELL_COLS), 0x1D7), edge_values(max(CELL_ROWS), max(CELL_COLS), 0xCE13)


@pytest.mark.parametrize("n_cols", CELL_COLS)
def test_cells_trees_of_a_row_list(ctx, mp2, cells_table, n_cols):
    ids, values = cells_table[0][:n_cols], np.ascontiguousarray(cells_table[1][:, :n_cols])
    top, cells = max(CELL_ROWS), n_cols - 1
    for variant in (0, 1):
        want_roots, want_nodes = np.zeros((top, 4), dtype=np.uint64), np.zeros((top, cells, 4), dtype=np.uint64)
        for r in range(top):  # the rows are independent: a shorter table is a prefix
            nodes, want_roots[r] = cells_walk(ids, values[r], variant)
            for k, h in nodes.items():
                want_nodes[r, k - 1] = h
        for rows in CELL_ROWS:
            rng = np.random.default_rng(0xCE14 + rows)
            subset = rng.integers(0, rows, size=max(1, rows // 3)).tolist()
            for what, idx in (("none", []), ("first", [0]), ("last", [rows - 1]), ("all", list(range(rows))), ("subset", subset + subset[:3])):
                listed = np.zeros(rows, dtype=bool)
                listed[idx] = True
                tag = (n_cols, rows, what, variant)
                # host form: roots and nodes, and roots alone
                roots, nodes = np.full((rows, 4), SENTINEL), np.full((rows, cells, 4), SENTINEL)
                IX.cells_tree_hashes_rows(ctx, ids, values[:rows], idx, roots, nodes, variant)
                roots2 = np.full((rows, 4), SENTINEL)
                IX.cells_tree_hashes_rows(ctx, ids, values[:rows], idx, roots2, None, variant)
                # device form
                d_v, d_r, d_n = ctx.to_device(values[:rows]), ctx.to_device(np.full((rows, 4), SENTINEL)), ctx.to_device(np.full((rows, max(cells, 1), 4), SENTINEL))
                mp2.cells_tree_hashes_rows_dev(ctx, variant, ids, d_v, rows, idx, d_r, d_n if cells else None)
                roots3, nodes3 = d_r.download((rows, 4)), d_n.download((rows, cells, 4))
                for d in (d_v, d_r, d_n):
                    d.free()
                for got in (roots, roots2, roots3):
                    assert np.array_equal(got[listed], want_roots[:rows][listed]) and (got[~listed] == SENTINEL).all(), tag
                for got in (nodes, nodes3):
                    assert np.array_equal(got[listed], want_nodes[:rows][listed]) and (got[~listed] == SENTINEL).all(), tag
        if n_cols == 1:
            assert not want_roots.any()  # row.rs:299-302: hash_no_pad(&[])


# ---- both halves, kept on the device ----------------------------------------------------------------------------------------------------
def test_table_hashes_kept_current(ctx, mp2):
    table = T.SyntheticTable(64, n_cols=4)
    left, right = TC.balanced(64)
    shape = IX.TreeShape.from_children(left, right)
    values = np.ascontiguousarray(table.values, dtype=np.uint32).copy()
    for variant in (0, 1):
        th = IX.TableHashes(ctx, table.col_ids, values, shape, variant)
        full = IX.table_hashes(ctx, table.col_ids, values, shape, variant)
        assert np.array_equal(th.row_hashes(), full[0]) and np.array_equal(th.cells_roots(), full[1]) and th.roots().tolist() == full[2].tolist()
        rows = [5, 40, 63]
        new = np.random.default_rng(0x7AB + variant).integers(0, 1 << 32, size=(3, values.shape[1], 8), dtype=np.uint32)
        touched = th.update(rows, new)
        assert touched.tolist() == TT.closure(left, right, rows)[0]
        now = values.copy()
        now[rows] = new
        full = IX.table_hashes(ctx, table.col_ids, now, shape, variant)
        assert np.array_equal(th.row_hashes(), full[0]) and np.array_equal(th.cells_roots(), full[1]) and th.roots().tolist() == full[2].tolist()
        assert th.update([], np.zeros((0, values.shape[1], 8), dtype=np.uint32)).size == 0
        assert np.array_equal(th.row_hashes(), full[0])
        th.free()
    shape.free()
