"""mp2g_cells_tree_hashes / mp2g_row_tree_hashes (csrc/index_hash.hip) against the oracle's sponge driven by plain recursive Python
walks of the trees: a missing child contributes the empty hash (all zero), min / max follow the children node by node
(row.rs:261-285). The walks are written here and share nothing with the library's level schedule. Equality is exact everywhere."""
import importlib
import sys

import numpy as np
import pytest

import oracle as O
import tree_cases as TC

pytestmark = pytest.mark.gpu

IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
T = TC.T
ZERO = [0, 0, 0, 0]
ROWS = (1, 63, 64, 65, 257)
MAX_COLS = 18


def H(words, variant):
    return [int(x) for x in O.hash_n_to_m_no_pad(np.array(words, dtype=np.uint64), 4, variant)]


def edge_values(rows, cols, seed):
    """uint32 [rows][cols][8]: uniform limbs, with 0, 2^256 - 1 and single all-ones limbs among the first rows"""
    v = np.random.default_rng(seed).integers(0, 1 << 32, size=(rows, cols, 8), dtype=np.uint32)
    if rows:
        v[0] = 0
    if rows > 1:
        v[1] = 0xFFFFFFFF
    for r in range(2, min(rows, 10)):
        v[r, :, (r - 2) % 8] = 0xFFFFFFFF
        v[r, :, (r - 1) % 8] = 0
    return v


# ---- cells trees ----------------------------------------------------------------------------------------------------------------------
def cells_walk(ids, row, variant):
    """every node's hash of one row's cells tree, {position: hash}, and the root's hash; row [n_cols][8]"""
    cells = len(ids) - 1
    out = {}

    def walk(k):
        if k is None:
            return ZERO
        left, right = T.sbbst_children(cells, k)
        out[k] = H(walk(left) + walk(right) + [int(ids[k])] + [int(x) for x in row[k]], variant)
        return out[k]

    return out, walk(T.sbbst_root(cells) if cells else None)


@pytest.fixture(scope="module")
def cells_table():
    return O.rand_field(MAX_COLS, 0x1D5), edge_values(max(ROWS), MAX_COLS, 0xCE11)


@pytest.mark.parametrize("n_cols", range(1, MAX_COLS + 1))
def test_cells_trees(ctx, mp2, cells_table, n_cols):
    ids, values = cells_table[0][:n_cols], np.ascontiguousarray(cells_table[1][:, :n_cols])
    for variant in (0, 1):
        want_nodes = np.zeros((max(ROWS), n_cols - 1, 4), dtype=np.uint64)
        want_roots = np.zeros((max(ROWS), 4), dtype=np.uint64)
        for r in range(max(ROWS)):
            nodes, want_roots[r] = cells_walk(ids, values[r], variant)
            for k, h in nodes.items():
                want_nodes[r, k - 1] = h
        for rows in ROWS:  # the rows are independent: a shorter table is a prefix
            roots = IX.cells_tree_hashes(ctx, ids, values[:rows], variant)
            roots2, nodes = IX.cells_tree_hashes(ctx, ids, values[:rows], variant, nodes=True)
            assert np.array_equal(roots, want_roots[:rows]) and np.array_equal(roots2, want_roots[:rows]), (n_cols, rows, variant)
            assert np.array_equal(nodes, want_nodes[:rows]), (n_cols, rows, variant)
    if n_cols == 1:
        assert not want_roots.any()  # row.rs:299-302: hash_no_pad(&[])


def test_cells_tree_of_255_cells(ctx, mp2):
    ids, values = O.rand_field(256, 0x1D6), edge_values(3, 256, 0xCE12)
    for variant in (0, 1):
        roots, nodes = IX.cells_tree_hashes(ctx, ids, values, variant, nodes=True)
        for r in range(3):
            want, root = cells_walk(ids, values[r], variant)
            assert roots[r].tolist() == root
            assert nodes[r].tolist() == [want[k] for k in range(1, 256)]
        assert np.array_equal(IX.cells_tree_hashes(ctx, ids, values, variant), roots)


# ---- row trees ------------------------------------------------------------------------------------------------------------------------
def row_walk(left, right, ident, value, payload, variant):
    """[n][4] by the definition: value(i) a list of 8 limbs, payload(i) a list of 4 words"""
    n = len(left)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 1000))
    out = [None] * n

    def walk(i):
        """(hash, min, max) of the subtree under i"""
        hl, mn, hr, mx = ZERO, value(i), ZERO, value(i)
        if left[i] >= 0:
            hl, mn, _ = walk(left[i])
        if right[i] >= 0:
            hr, _, mx = walk(right[i])
        out[i] = H(hl + hr + mn + mx + [ident] + value(i) + payload(i), variant)
        return out[i], mn, mx

    children = {c for c in left + right if c >= 0}
    for i in range(n):
        if i not in children:
            walk(i)
    return np.array(out, dtype=np.uint64).reshape(n, 4)


def row_case(ctx, left, right, n_cols, seed):
    n = len(left)
    shape = IX.TreeShape.from_children(left, right)
    if n == 0:  # the empty shape: nothing to hash, nothing launched
        assert IX.row_tree_hashes(ctx, shape, 5, np.zeros((0, 8), dtype=np.uint32)).shape == (0, 4)
        return
    table = edge_values(n, n_cols, seed)
    payload = O.rand_field((n, 4), seed + 1)
    ident = int(O.rand_field(1, seed + 2)[0])
    zero = lambda i: ZERO
    for variant in (0, 1):
        for values, value in ((np.ascontiguousarray(table[:, 0]), lambda i: [int(x) for x in table[i, 0]]), (table, lambda i: [int(x) for x in table[i, 0]])):
            want = row_walk(left, right, ident, value, lambda i: [int(x) for x in payload[i]], variant)
            assert np.array_equal(IX.row_tree_hashes(ctx, shape, ident, values, payload, variant), want), (n, variant, values.shape)
            want = row_walk(left, right, ident, value, zero, variant)
            assert np.array_equal(IX.row_tree_hashes(ctx, shape, ident, values, None, variant), want), (n, variant, values.shape)
    shape.free()


@pytest.mark.parametrize("name", list(TC.accepted(small=True)))
def test_row_trees(ctx, mp2, name):
    left, right = TC.accepted(small=True)[name]
    row_case(ctx, left, right, 3, 0x7EE + len(left))


def test_row_tree_of_4097_rows(ctx, mp2):
    """a balanced tree that crosses block boundaries at several levels; the table's column 0 read in place"""
    left, right = TC.balanced(4097)
    n, n_cols = 4097, 2
    shape = IX.TreeShape.from_children(left, right)
    table, payload = edge_values(n, n_cols, 0xB16), O.rand_field((n, 4), 0xB17)
    for variant in (0, 1):
        want = row_walk(left, right, 77, lambda i: [int(x) for x in table[i, 0]], lambda i: [int(x) for x in payload[i]], variant)
        assert np.array_equal(IX.row_tree_hashes(ctx, shape, 77, table, payload, variant), want)
    shape.free()


def test_values_that_are_not_16_byte_aligned(ctx, mp2):
    """a value_stride that is no multiple of 4 words, and a table that starts 4 bytes into its buffer: the scalar loads"""
    left, right = TC.sbbst(70)
    shape = IX.TreeShape.from_children(left, right)
    v9 = edge_values(70, 1, 0xA11).reshape(70, 8)
    v9 = np.concatenate([v9, np.full((70, 1), 0xDEADBEEF, dtype=np.uint32)], axis=1)  # stride 9
    want = row_walk(left, right, 5, lambda i: [int(x) for x in v9[i, :8]], lambda i: ZERO, 0)
    assert np.array_equal(IX.row_tree_hashes(ctx, shape, 5, v9, None, 0), want)
    ids, table = O.rand_field(6, 0xA12), edge_values(65, 6, 0xA13)
    buf = ctx.alloc(table.nbytes + 16)
    buf.upload_at(table, 4)
    d_roots = ctx.alloc(65 * 32)
    mp2.cells_tree_hashes_dev(ctx, 0, ids, buf.ptr.value + 4, 65, d_roots)
    assert np.array_equal(d_roots.download((65, 4)), IX.cells_tree_hashes(ctx, ids, table, 0))
    d_rows = ctx.alloc(65 * 32)
    s65 = IX.TreeShape.sbbst(65)
    mp2.row_tree_hashes_dev(ctx, 0, s65, 9, buf.ptr.value + 4, 48, d_roots, d_rows)
    assert np.array_equal(d_rows.download((65, 4)), IX.row_tree_hashes(ctx, s65, 9, table, d_roots.download((65, 4)), 0))
    for x in (buf, d_roots, d_rows, shape, s65):
        x.free()


# ---- the two halves chained, against the path bench.py trusts ------------------------------------------------------------------------
def test_table_hashes_is_the_per_level_python_path(ctx, mp2):
    table = T.SyntheticTable(64, n_cols=4)
    root, nodes, spans = T.balanced_bst(64)
    left, right = TC.balanced(64)
    shape = IX.TreeShape.from_children(left, right)
    row_h, cells_roots, roots = IX.table_hashes(ctx, table.col_ids, table.values, shape)
    assert roots.tolist() == [root]
    # the composition of indexing.cell_node_hashes / row_node_hashes that table.expected_root_public_inputs makes, restated
    rows, C = 64, 4
    ints = lambda a: [sum(int(x) << (32 * (7 - j)) for j, x in enumerate(v)) for v in a]
    empty = IX.empty_poseidon_hash(ctx)
    cell_h = {}
    for k in sorted(range(1, C + 1), key=lambda k: ((k & -k).bit_length(), k)):
        l, r = T.sbbst_children(C, k)
        lh = cell_h[l] if l is not None else np.tile(empty, (rows, 1))
        rh = cell_h[r] if r is not None else np.tile(empty, (rows, 1))
        cell_h[k] = IX.cell_node_hashes(ctx, lh, rh, np.full(rows, table.col_ids[k]), ints(table.values[:, k]))
    assert np.array_equal(cells_roots, cell_h[T.sbbst_root(C)])
    sec = ints(table.values[:, 0])
    height = TC.describe(left, right)[0]
    want = np.zeros((rows, 4), dtype=np.uint64)
    for lvl in range(max(height) + 1):
        ks = [k for k in range(rows) if height[k] == lvl]
        lh = np.stack([want[left[k]] if left[k] >= 0 else empty for k in ks])
        rh = np.stack([want[right[k]] if right[k] >= 0 else empty for k in ks])
        want[ks] = IX.row_node_hashes(ctx, lh, rh, [sec[spans[k][0]] for k in ks], [sec[spans[k][1] - 1] for k in ks],
                                      np.full(len(ks), table.col_ids[0]), [sec[k] for k in ks], cells_roots[ks])
    assert np.array_equal(row_h, want)
    # ... and the function itself: the root proof's first four public inputs
    wit = T.TableWitness(ctx, table, spans)
    assert np.array_equal(row_h[roots[0]], T.expected_root_public_inputs(ctx, table, wit, root, nodes, spans)[:4])
    # the _dev forms, read back, are the host forms
    roots_host, nodes_host = IX.cells_tree_hashes(ctx, table.col_ids, table.values, 0, nodes=True)
    assert np.array_equal(roots_host, cells_roots)
    assert np.array_equal(IX.row_tree_hashes(ctx, shape, table.col_ids[0], table.values, cells_roots, 0), row_h)
    d_values, d_roots, d_nodes, d_rows = ctx.to_device(table.values), ctx.alloc(rows * 32), ctx.alloc(rows * C * 32), ctx.alloc(rows * 32)
    for variant in (0, 1):
        mp2.cells_tree_hashes_dev(ctx, variant, table.col_ids, d_values, rows, d_roots, d_nodes)
        mp2.row_tree_hashes_dev(ctx, variant, shape, table.col_ids[0], d_values, (C + 1) * 8, d_roots, d_rows)
        got = d_roots.download((rows, 4)), d_nodes.download((rows, C, 4)), d_rows.download((rows, 4))
        host = IX.cells_tree_hashes(ctx, table.col_ids, table.values, variant, nodes=True)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
        assert np.array_equal(got[2], IX.row_tree_hashes(ctx, shape, table.col_ids[0], table.values, host[0], variant))
        assert np.array_equal(got[2], IX.table_hashes(ctx, table.col_ids, table.values, shape, variant)[0])
    for x in (d_values, d_roots, d_nodes, d_rows, shape):
        x.free()


def test_index_tree_use(ctx, mp2):
    """IndexNode::aggregate over a 7-node sbbst of blocks: id = a block-number column id, payload = the blocks' row-tree roots"""
    n = 7
    left, right = TC.sbbst(n)
    shape = IX.TreeShape.sbbst(n)
    block_id = int(O.hash_n_to_m_no_pad(np.frombuffer(b"BLOCK_NUMBER", dtype=np.uint8).astype(np.uint64), 4)[0])
    blocks = [1000 + 3 * i for i in range(n)]  # block numbers in order
    row_roots = O.rand_field((n, 4), 0x1DE)
    got = IX.row_tree_hashes(ctx, shape, block_id, mp2.u256_to_limbs(blocks), row_roots)
    empty = IX.empty_poseidon_hash(ctx)
    want, mm = {}, {}
    for k in (0, 2, 4, 6, 1, 5, 3):  # children first, by hand
        l, r = left[k], right[k]
        mm[k] = IX.index_node_min_max(blocks[k], mm[l] if l >= 0 else None, mm[r] if r >= 0 else None)
        want[k] = IX.index_node_hashes(ctx, (want[l] if l >= 0 else empty)[None], (want[r] if r >= 0 else empty)[None], [mm[k][0]], [mm[k][1]],
                                       [block_id], [blocks[k]], row_roots[k][None])[0]
    assert np.array_equal(got, np.stack([want[k] for k in range(n)]))
    assert mm[3] == (blocks[0], blocks[6])
    shape.free()
