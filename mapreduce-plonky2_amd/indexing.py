"""Off-circuit Merkle payload hashes of the cells / rows trees, batched per tree level on the GPU.

Mirrors mp2-v1/src/indexing/cell.rs:120-157 (`MerkleCell::aggregate`) and row.rs:257-317
(`RowPayload::aggregate`): the reference hashes one node per call while walking a ryhope work plan;
here all nodes of a level go through one `mp2g_hash_no_pad_batch` launch. Packing only -- the
arithmetic is the HIP sponge kernel.
"""
import importlib

import numpy as np

_mp2 = importlib.import_module(__name__.rsplit(".", 1)[0])


def empty_poseidon_hash(ctx, variant=0):
    """mp2-common/src/poseidon.rs:44-46: H::hash_no_pad(&[])  (= all-zero state squeezed)."""
    return ctx.hash_no_pad_batch(np.zeros((1, 0), dtype=np.uint64), 4, variant)[0]


def u256_limbs(values):
    """[count] python ints -> [count][8] field limbs (u256.rs:870-877: 8 big-endian u32 words)."""
    return _mp2.u256_to_limbs(values).astype(np.uint64)


def cell_node_hashes(ctx, left, right, ids, values, variant=0):
    """H(H(left) || H(right) || id || value): 4 + 4 + 1 + 8 = 17 limbs per node.
    left/right: [count][4] child hashes (use empty_poseidon_hash for a missing child)."""
    left, right = np.asarray(left, dtype=np.uint64), np.asarray(right, dtype=np.uint64)
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1, 1)
    inputs = np.concatenate([left, right, ids, u256_limbs(values)], axis=1)
    assert inputs.shape[1] == 17
    return ctx.hash_no_pad_batch(inputs, 4, variant)


def row_node_hashes(ctx, left, right, mins, maxs, ids, values, cells_root, variant=0):
    """H(hL || hR || min || max || id || value || cells_root): 4+4+8+8+1+8+4 = 37 limbs per node."""
    left, right = np.asarray(left, dtype=np.uint64), np.asarray(right, dtype=np.uint64)
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1, 1)
    inputs = np.concatenate([left, right, u256_limbs(mins), u256_limbs(maxs), ids, u256_limbs(values),
                             np.asarray(cells_root, dtype=np.uint64)], axis=1)
    assert inputs.shape[1] == 37
    return ctx.hash_no_pad_batch(inputs, 4, variant)


def cells_tree_root(ctx, ids, values, variant=0):
    """Root hash of a complete binary cells tree in heap order (node i has children 2i+1, 2i+2,
    missing children hash as empty): bottom-up, one batched launch per level."""
    n = len(ids)
    empty = empty_poseidon_hash(ctx, variant)
    hashes = np.tile(empty, (n, 1))
    depth = max(1, (n).bit_length())
    for level in range(depth - 1, -1, -1):
        lo, hi = (1 << level) - 1, min(n, (1 << (level + 1)) - 1)
        if lo >= hi:
            continue
        idx = np.arange(lo, hi)
        lch, rch = 2 * idx + 1, 2 * idx + 2
        left = np.where((lch < n)[:, None], hashes[np.minimum(lch, n - 1)], empty)
        right = np.where((rch < n)[:, None], hashes[np.minimum(rch, n - 1)], empty)
        hashes[idx] = cell_node_hashes(ctx, left, right, [ids[i] for i in idx], [values[i] for i in idx], variant)
    return hashes[0], hashes


def index_node_hashes(ctx, left, right, mins, maxs, ids, values, row_tree_hash, variant=0):
    """`IndexNode::aggregate` (mp2-v1/src/indexing/index.rs:61-101), the block / primary-index tree:
    H(hL || hR || min || max || id || value || row_tree_hash), the same 37-limb layout as a row node with the
    row tree's root hash in the place of the cells root. min / max follow the children as in the reference:
    no child -> (value, value); left only -> (left.min, value); both -> (left.min, right.max)."""
    return row_node_hashes(ctx, left, right, mins, maxs, ids, values, row_tree_hash, variant)


def index_node_min_max(value, left=None, right=None):
    """min / max bookkeeping of IndexNode::aggregate; left / right are (min, max) tuples or None"""
    if left is None and right is None:
        return value, value
    if right is None:
        return left[0], value
    if left is None:
        raise ValueError("ryhope sbbst is wrong")  # the reference panics: a right child without a left one
    return left[0], right[1]


# ---- whole trees on the device (csrc/index_hash.hip): one call per tree kind, one launch per level, no host round trip --------------
TreeShape = _mp2.TreeShape  # from_children(left, right), sbbst(n), describe()


def _table_values(values, n_cols):
    """uint32 [rows][n_cols][8]; without columns the array stays as it comes, and the library refuses n_cols = 0"""
    v = np.ascontiguousarray(values, dtype=np.uint32)
    return v.reshape(-1, n_cols, 8) if n_cols else v.reshape(v.shape[0] if v.ndim else 0, -1)


def cells_tree_hashes(ctx, col_ids, values, variant=0, nodes=False):
    """`MerkleCell::aggregate` (cell.rs:120-157) for every row's cells tree (mp2g_cells_tree_hashes): the sbbst over positions
    1..n_cols-1, the cell at position k has id col_ids[k] and value values[row][k]; column 0 is the secondary index and is not a cell.
    values: uint32 [rows][n_cols][8] as row_digests takes them. Returns roots [rows][4], and with nodes=True also every node's hash
    [rows][n_cols-1][4] (position k at index k - 1)."""
    ids = np.ascontiguousarray(col_ids, dtype=np.uint64).ravel()
    v = _table_values(values, ids.size)
    rows = v.shape[0]
    roots = np.zeros((rows, 4), dtype=np.uint64)
    all_nodes = np.zeros((rows, max(ids.size, 1) - 1, 4), dtype=np.uint64) if nodes else None
    _mp2._ck(_mp2.load().mp2g_cells_tree_hashes(ctx, int(variant), _mp2._p(ids), ids.size, _mp2._p(v), rows, _mp2._p(roots),
                                                 _mp2._p(all_nodes) if nodes else None))
    return (roots, all_nodes) if nodes else roots


def row_tree_hashes(ctx, shape, id, values, payload=None, variant=0):
    """`RowPayload::aggregate` (row.rs:257-317) / `IndexNode::aggregate` (index.rs:61-101) for every node of `shape`
    (mp2g_row_tree_hashes): H(hL || hR || min || max || id || value || payload) with min / max taken down the left / right spine.
    values: uint32 [n][8], or [n][n_cols][8] to read column 0 of a table in place; payload [n][4] (cells roots, or row-tree roots for
    the index tree) or None = the empty hash for every node. Returns hashes [n][4]."""
    n = shape.size
    v = np.ascontiguousarray(values, dtype=np.uint32).reshape(n, -1) if n else np.zeros((0, 8), dtype=np.uint32)
    pl = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint64).reshape(n, 4)
    out = np.zeros((n, 4), dtype=np.uint64)
    if ctx is not None:
        ctx._adopt(shape)  # a shape is freed before the context it was used with: closing the context frees it
    _mp2._ck(_mp2.load().mp2g_row_tree_hashes(ctx, int(variant), shape.h, int(id), _mp2._p(v), v.shape[1],
                                               None if pl is None else _mp2._p(pl), _mp2._p(out)))
    return out


def table_hashes(ctx, col_ids, values, shape, variant=0):
    """both halves for a block of rows: values [rows][n_cols][8] go up once, the cells trees' roots stay on the device as the row
    tree's payload (the two _dev calls, value_stride = n_cols * 8), one download at the end.
    Returns (row_hashes [rows][4], cells_roots [rows][4], roots = the row tree's root nodes, ascending)."""
    ids = np.ascontiguousarray(col_ids, dtype=np.uint64).ravel()
    v = _table_values(values, ids.size)
    rows = v.shape[0]
    if shape.size != rows:
        raise ValueError("the row tree's shape has not one node per row")
    roots = shape.describe()["roots"]
    if rows == 0:
        return np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), roots
    d_values, d_cells, d_rows = ctx.to_device(v), ctx.alloc(rows * 32), ctx.alloc(rows * 32)
    try:
        _mp2.cells_tree_hashes_dev(ctx, variant, ids, d_values, rows, d_cells)
        _mp2.row_tree_hashes_dev(ctx, variant, shape, ids[0], d_values, ids.size * 8, d_cells, d_rows)
        return d_rows.download((rows, 4)), d_cells.download((rows, 4)), roots
    finally:
        for d in (d_values, d_cells, d_rows):
            d.free()


# ---- the steady state: a block changes a handful of rows (MerkleTreeKvDb::aggregate over touched(), ryhope/src/lib.rs:179-222) ---------
def cells_tree_hashes_rows(ctx, col_ids, values, row_idx, roots, nodes=None, variant=0):
    """mp2g_cells_tree_hashes_rows: the complete cells trees of the rows `row_idx` recomputed from the current table `values`
    (uint32 [rows][n_cols][8], the whole table). roots [rows][4] and nodes ([rows][n_cols-1][4] or None) are uint64 arrays of the
    caller's, written in place at the listed rows only; duplicates in row_idx are allowed. Returns roots."""
    ids = np.ascontiguousarray(col_ids, dtype=np.uint64).ravel()
    v = _table_values(values, ids.size)
    rows = v.shape[0]
    idx = np.ascontiguousarray(row_idx, dtype=np.uint32).ravel()
    for a, shape in ((roots, (rows, 4)), (nodes, (rows, max(ids.size, 1) - 1, 4))):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags.c_contiguous and a.shape == shape):
            raise ValueError(f"roots / nodes: a contiguous uint64 array of shape {shape} that the call can write in place")
    _mp2._ck(_mp2.load().mp2g_cells_tree_hashes_rows(ctx, int(variant), _mp2._p(ids), ids.size, _mp2._p(v), rows, _mp2._p(idx),
                                                      idx.size, None if roots is None else _mp2._p(roots),
                                                      None if nodes is None else _mp2._p(nodes)))
    return roots


def row_tree_hashes_update(ctx, shape, id, values, payload, touched, hashes, variant=0):
    """mp2g_row_tree_hashes_update: re-hash the nodes `touched` and their ancestors (shape.touched(touched)) under the current
    values / payload, arguments as row_tree_hashes takes them. hashes: uint64 [n][4] of the caller's, valid outside that set on
    entry, written in place inside it and nowhere else. Returns hashes."""
    n = shape.size
    v = np.ascontiguousarray(values, dtype=np.uint32).reshape(n, -1) if n else np.zeros((0, 8), dtype=np.uint32)
    pl = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint64).reshape(n, 4)
    t = np.ascontiguousarray(touched, dtype=np.uint32).ravel()
    if hashes is not None and not (isinstance(hashes, np.ndarray) and hashes.dtype == np.uint64 and hashes.flags.c_contiguous and hashes.shape == (n, 4)):
        raise ValueError(f"hashes: a contiguous uint64 array of shape {(n, 4)} that the call can write in place")
    if ctx is not None:
        ctx._adopt(shape)
    _mp2._ck(_mp2.load().mp2g_row_tree_hashes_update(ctx, int(variant), shape.h, int(id), _mp2._p(v), v.shape[1],
                                                      None if pl is None else _mp2._p(pl), _mp2._p(t), t.size,
                                                      None if hashes is None else _mp2._p(hashes)))
    return hashes


class TableHashes:
    """A block of rows whose table, cells roots and row-tree hashes stay on the device between blocks: built by the two full calls
    (what table_hashes chains), then kept current by update(), which re-hashes the changed rows' cells trees
    (mp2g_cells_tree_hashes_rows_dev) and the changed nodes' lineages in the row tree (mp2g_row_tree_hashes_update_dev) -- where a
    Rust host calls MerkleTreeKvDb::aggregate. values: uint32 [rows][n_cols][8]; shape: the row tree, one node per row."""

    def __init__(self, ctx, col_ids, values, shape, variant=0):
        self.ctx, self.shape, self.variant = ctx, shape, int(variant)
        self.ids = np.ascontiguousarray(col_ids, dtype=np.uint64).ravel()
        v = _table_values(values, self.ids.size)
        self.rows = v.shape[0]
        if shape.size != self.rows:
            raise ValueError("the row tree's shape has not one node per row")
        self.d_values = self.d_cells = self.d_rows = None
        if self.rows:
            self.d_values, self.d_cells, self.d_rows = ctx.to_device(v), ctx.alloc(self.rows * 32), ctx.alloc(self.rows * 32)
            _mp2.cells_tree_hashes_dev(ctx, self.variant, self.ids, self.d_values, self.rows, self.d_cells)
            _mp2.row_tree_hashes_dev(ctx, self.variant, shape, self.ids[0], self.d_values, self.ids.size * 8, self.d_cells, self.d_rows)

    def update(self, rows, new_values):
        """rows: the indices of the changed rows (distinct); new_values: uint32 [len(rows)][n_cols][8]. Returns the row-tree nodes
        that were re-hashed (shape.touched(rows))."""
        idx = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        nv = np.ascontiguousarray(new_values, dtype=np.uint32).reshape(idx.size, self.ids.size, 8)
        if idx.size and int(idx.max()) >= self.rows:
            raise ValueError("row index outside the table")
        touched = self.shape.touched(idx)
        row_bytes = self.ids.size * 32
        for j, r in enumerate(idx.tolist()):
            self.d_values.upload_at(nv[j], r * row_bytes)
        _mp2.cells_tree_hashes_rows_dev(self.ctx, self.variant, self.ids, self.d_values, self.rows, idx, self.d_cells)
        _mp2.row_tree_hashes_update_dev(self.ctx, self.variant, self.shape, self.ids[0], self.d_values, self.ids.size * 8, self.d_cells, idx,
                                        self.d_rows)
        return touched

    def row_hashes(self):
        return self.d_rows.download((self.rows, 4)) if self.rows else np.zeros((0, 4), dtype=np.uint64)

    def cells_roots(self):
        return self.d_cells.download((self.rows, 4)) if self.rows else np.zeros((0, 4), dtype=np.uint64)

    def roots(self):
        """the row tree's root nodes, ascending"""
        return self.shape.describe()["roots"]

    def free(self):
        for d in (self.d_values, self.d_cells, self.d_rows):
            if d is not None:
                d.free()
        self.d_values = self.d_cells = self.d_rows = None


class TableDigests:
    """The Ecgfp5 digests of a block of rows, kept on the device between blocks beside TableHashes: every node of every row's cells
    tree (Cell::values_digest accumulated up the sbbst), every row's own digest row_id * (D(secondary cell) + cells root)
    (secondary_index_cell.rs:99-139) and its accumulation up the row tree (row_tree/full_node.rs:78-82) -- the fields of
    table.TableWitness, over any tree shape. Built by mp2g_cells_tree_digests_dev, mp2g_row_digests_dev with the cells roots and
    mp2g_tree_digests_dev; update() runs the listed-rows forms of the first two and mp2g_tree_digests_update_dev, so a block costs its
    touched closure. Points stay in fractional coordinates on the device; the accessors encode what they download.
    values: uint32 [rows][n_cols][8], column 0 the secondary index (the row's unique data); shape: the row tree, one node per row."""

    def __init__(self, ctx, col_ids, values, shape, variant=0):
        self.ctx, self.shape, self.variant = ctx, shape, int(variant)
        self.ids = np.ascontiguousarray(col_ids, dtype=np.uint64).ravel()
        v = _table_values(values, self.ids.size)
        self.rows, self.cells = v.shape[0], max(self.ids.size, 1) - 1
        if shape.size != self.rows:
            raise ValueError("the row tree's shape has not one node per row")
        self.d_values = self.d_cells = self.d_own = self.d_acc = None
        if self.rows:
            fb = _mp2.FRAC_BYTES
            self.d_values = ctx.to_device(v)
            self.d_cells = ctx.alloc(self.rows * self.cells * fb) if self.cells else None
            self.d_own, self.d_acc = ctx.alloc(self.rows * fb), ctx.alloc(self.rows * fb)
            _mp2.cells_tree_digests_dev(ctx, self.variant, self.ids, self.d_values, self.rows, self.d_cells)
            self._row_own(None)
            _mp2.tree_digests_dev(ctx, shape, self.d_own, self.d_acc)

    def _row_own(self, idx):
        # the unique column is column 0 of the resident table, read in place
        _mp2.row_digests_dev(self.ctx, self.variant, self.ids, self.d_values, self.d_values, self.ids.size * 8, 1, self.rows, self.d_own,
                             self.d_cells, idx)

    def update(self, rows, new_values):
        """rows: the indices of the changed rows (distinct); new_values: uint32 [len(rows)][n_cols][8]. Returns the row-tree nodes
        whose accumulated digest was recomputed (shape.touched(rows))."""
        idx = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        nv = np.ascontiguousarray(new_values, dtype=np.uint32).reshape(idx.size, self.ids.size, 8)
        if idx.size and int(idx.max()) >= self.rows:
            raise ValueError("row index outside the table")
        touched = self.shape.touched(idx)
        if not idx.size:
            return touched
        row_bytes = self.ids.size * 32
        for j, r in enumerate(idx.tolist()):
            self.d_values.upload_at(nv[j], r * row_bytes)
        _mp2.cells_tree_digests_dev(self.ctx, self.variant, self.ids, self.d_values, self.rows, self.d_cells, idx)
        self._row_own(idx)
        _mp2.tree_digests_update_dev(self.ctx, self.shape, self.d_own, idx, self.d_acc)
        return touched

    def _listed(self, which):
        idx = np.arange(self.rows, dtype=np.uint32) if which is None else np.ascontiguousarray(which, dtype=np.uint32).ravel()
        if idx.size and int(idx.max()) >= self.rows:
            raise ValueError("row index outside the table")
        return idx

    def cell_digests(self, rows=None):
        """Weierstrass [len(rows)][n_cols-1][11]: the accumulated digest of every node of the rows' cells trees (position k at index k - 1)"""
        idx = self._listed(rows)
        if not idx.size or not self.cells:
            return np.zeros((idx.size, self.cells, 11), dtype=np.uint64)
        flat = (idx.astype(np.uint64)[:, None] * np.uint64(self.cells) + np.arange(self.cells, dtype=np.uint64)[None, :]).astype(np.uint32)
        return _mp2.curve_emit_dev(self.ctx, self.d_cells, 0, flat)[1].reshape(idx.size, self.cells, 11)

    def row_own(self, rows=None):
        """Weierstrass [len(rows)][11]: the rows' own (individual) digests"""
        idx = self._listed(rows)
        return _mp2.curve_emit_dev(self.ctx, self.d_own, 0, idx)[1] if idx.size else np.zeros((0, 11), dtype=np.uint64)

    def row_digests(self, nodes=None):
        """(encodings [len(nodes)][5], Weierstrass [len(nodes)][11]): the accumulated digests of the row-tree nodes"""
        idx = self._listed(nodes)
        if not idx.size:
            return np.zeros((0, 5), dtype=np.uint64), np.zeros((0, 11), dtype=np.uint64)
        return _mp2.curve_emit_dev(self.ctx, self.d_acc, 0, idx)

    def root_digests(self):
        """row_digests of the row tree's root nodes, ascending"""
        return self.row_digests(self.shape.describe()["roots"])

    def free(self):
        for d in (self.d_values, self.d_cells, self.d_own, self.d_acc):
            if d is not None:
                d.free()
        self.d_values = self.d_cells = self.d_own = self.d_acc = None
