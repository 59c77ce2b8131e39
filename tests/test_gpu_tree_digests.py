"""mp2g_tree_digests* / mp2g_cells_tree_digests_dev / mp2g_row_digests_dev / mp2g_curve_{decode,emit}_dev (csrc/tree_digest.hip,
csrc/tree_digest_api.hip) and indexing.TableDigests against the CPU oracle (tests/tree_digest_cases.py, tests/table_oracle.py) and
the entry points that were there before them (curve_sum_ranges, row_digests, map_to_curve_batch through table.TableWitness).
Points are compared through their canonical encodings and the 11-limb Weierstrass form, word for word; buffers that a call must
not write are compared as raw words."""
import copy
import importlib

import numpy as np
import pytest

import ec_cases as EC
import table_oracle as TO
import tree_cases as TC
import tree_digest_cases as TD
import tree_touched_cases as TT

pytestmark = pytest.mark.gpu

MP2 = importlib.import_module("mapreduce-plonky2_amd")
IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
T = TC.T
GARBAGE = np.uint64(0x0BAD0BAD0BAD0BAD)
FB = MP2.FRAC_BYTES


def decoded(ctx, mp2, own_w):
    """the encodings as points on the device"""
    n = len(own_w)
    d = ctx.alloc(max(n, 1) * FB)
    mp2.curve_decode_dev(ctx, own_w, d)
    return d


def full_pass(ctx, mp2, shape, own_w):
    d_own, d_acc = decoded(ctx, mp2, own_w), ctx.alloc(max(shape.size, 1) * FB)
    mp2.tree_digests_dev(ctx, shape, d_own, d_acc)
    return d_own, d_acc


def free(*bufs):
    for d in bufs:
        d.free()


# ---- the full pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pattern", TD.FULL_CASES, ids=lambda v: str(v))
def test_full_pass(ctx, mp2, shape, pattern):
    left, right = TD.SHAPES[shape]
    n = len(left)
    own, (want_w, want_wei) = TD.own_points(shape, pattern), TD.full_expected(shape, pattern)
    s = IX.TreeShape.from_children(left, right)
    if n == 0:
        mp2.tree_digests_dev(ctx, s, None, None)  # nothing launched, nothing read
        w, wei = mp2.tree_digests(ctx, s, own)
        assert w.shape == (0, 5) and wei.shape == (0, 11)
        s.free()
        return
    d_own, d_acc = full_pass(ctx, mp2, s, own)
    w, wei = mp2.curve_emit_dev(ctx, d_acc, n)
    assert np.array_equal(w, want_w) and np.array_equal(wei, want_wei)
    w, wei = mp2.curve_emit_dev(ctx, d_own, n)  # own is read only
    assert np.array_equal(w, own)
    w, wei = mp2.tree_digests(ctx, s, own)
    assert np.array_equal(w, want_w) and np.array_equal(wei, want_wei)
    if shape in TD.IN_ORDER:
        _, mn, mx, _ = TC.describe(left, right)
        w, wei = mp2.curve_sum_ranges(ctx, own, [[mn[i], mx[i] + 1] for i in range(n)])
        assert np.array_equal(w, want_w) and np.array_equal(wei, want_wei)
    free(d_own, d_acc)
    s.free()


def test_decode_then_emit_is_the_identity(ctx, mp2):
    b = EC.base_points(300)
    pts = np.concatenate([b, EC.NEUTRAL_W[None], EC.negate(b[:20])])
    n = len(pts)
    d = decoded(ctx, mp2, pts)
    w, wei = mp2.curve_emit_dev(ctx, d, n)
    assert np.array_equal(w, pts)
    assert np.array_equal(wei, mp2.curve_sum_ranges(ctx, pts, [[i, i + 1] for i in range(n)])[1])
    assert np.array_equal(wei[300], EC.NEUTRAL_WEI)
    rng = np.random.default_rng(0x1D)
    idx = np.concatenate([rng.permutation(n), [7, 7, 300, 0, n - 1, 7]]).astype(np.uint32)
    w2, wei2 = mp2.curve_emit_dev(ctx, d, 0, idx)
    assert np.array_equal(w2, pts[idx]) and np.array_equal(wei2, wei[idx])
    assert mp2.curve_emit_dev(ctx, d, 0, [])[0].shape == (0, 5)
    d.free()


def test_decode_refuses_invalid_and_non_canonical_encodings(ctx, mp2):
    bad = EC.bad_encodings(4)
    for k, at in enumerate(EC.REFUSAL_INDICES):
        pts = EC.refusal_batch()
        pts[at] = bad[k]
        d = ctx.alloc(len(pts) * FB)
        with pytest.raises(mp2.Mp2gError, match="invalid point encoding"):
            mp2.curve_decode_dev(ctx, pts, d)
        d.free()
    sentinel = np.full((300, 20), GARBAGE)
    s300 = IX.TreeShape.from_children(*TD.isolated(300))
    for row in EC.noncanonical():
        pts = EC.refusal_batch()
        pts[128] = row
        d = ctx.to_device(sentinel)
        with pytest.raises(mp2.Mp2gError, match="not canonical.*point 128"):
            mp2.curve_decode_dev(ctx, pts, d)
        assert np.array_equal(d.download((300, 20)), sentinel)  # refused on the host: nothing uploaded, nothing launched
        with pytest.raises(mp2.Mp2gError, match="not canonical"):
            mp2.tree_digests(ctx, s300, pts)
        d.free()
    s300.free()


# ---- the update -------------------------------------------------------------------------------------------------------------------
def check_update(ctx, mp2, left, right, s, d_acc0, own1, touched, what):
    """d_acc0: valid digests of the state before the change (left as it is). (a) the update of a copy of it gives the full pass over
    own1 at every node; (b) with garbage where the contract allows it, the closure still comes out right and every raw word outside
    the closure is what it was."""
    n = len(left)
    want_w, want_wei = TD.expected(left, right, own1)
    inside, garbage = TD.closure_mask(left, right, touched)
    raw0 = d_acc0.download((n, 20))
    d_own = decoded(ctx, mp2, own1)
    d_acc = ctx.to_device(raw0)
    mp2.tree_digests_update_dev(ctx, s, d_own, touched, d_acc)
    w, wei = mp2.curve_emit_dev(ctx, d_acc, n)
    assert np.array_equal(w, want_w) and np.array_equal(wei, want_wei), what
    assert np.array_equal(d_acc.download((n, 20))[~inside], raw0[~inside]), what
    planted = raw0.copy()
    planted[garbage] = GARBAGE
    planted[inside] = GARBAGE  # every closure node is rewritten
    d_acc.upload(planted)
    mp2.tree_digests_update_dev(ctx, s, d_own, touched, d_acc)
    raw = d_acc.download((n, 20))
    assert np.array_equal(raw[~inside], planted[~inside]), what
    closure = np.flatnonzero(inside).astype(np.uint32)
    if closure.size:
        w, wei = mp2.curve_emit_dev(ctx, d_acc, 0, closure)
        assert np.array_equal(w, want_w[closure]) and np.array_equal(wei, want_wei[closure]), what
    else:
        assert np.array_equal(raw, planted), what
    free(d_own, d_acc)


def run_update_case(ctx, mp2, label, shape, touched):
    left, right = TD.UPDATE_SHAPES[shape]
    s = IX.TreeShape.from_children(left, right)
    d_own0, d_acc0 = full_pass(ctx, mp2, s, TD.old_own(shape))
    check_update(ctx, mp2, left, right, s, d_acc0, TD.changed_own(shape, touched), touched, label)
    free(d_own0, d_acc0)
    s.free()


UPDATE_CASES = TD.update_cases()


@pytest.mark.parametrize("label,shape,touched", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_update(ctx, mp2, label, shape, touched):
    run_update_case(ctx, mp2, label, shape, touched)


@pytest.mark.parametrize("extra", [0, 1])
def test_the_last_fused_and_the_first_per_level_closure(ctx, mp2, extra):
    """W and W + 1 leaves of sbbst300, W read from the library: the widest closure the fused kernel takes and the narrowest that
    goes level by level"""
    w = mp2.tree_digests_update_fused_width() + extra
    label, shape, touched = [c for c in TD.update_cases(w - extra) if c[0] == f"sbbst300: {w} leaves"][0]
    assert len(touched) == w
    run_update_case(ctx, mp2, label, shape, touched)


def test_update_after_an_insertion(ctx, mp2):
    """sbbst(36) grows to sbbst(37): a new shape, the old digests with one garbage entry appended, touched = the new node and the
    nodes whose children changed"""
    (ol, orr), (nl, nr), touched = TD.insertion_case()
    own = EC.base_points(37)
    s_old, s_new = IX.TreeShape.from_children(ol, orr), IX.TreeShape.from_children(nl, nr)
    d_own0, d_acc0 = full_pass(ctx, mp2, s_old, own[:36])
    grown = ctx.to_device(np.concatenate([d_acc0.download((36, 20)), np.full((1, 20), GARBAGE)]))
    check_update(ctx, mp2, nl, nr, s_new, grown, own, touched, "insertion")
    free(d_own0, d_acc0, grown)
    s_old.free()
    s_new.free()


# ---- cells trees and rows -----------------------------------------------------------------------------------------------------------
def check_table(ctx, mp2, table, variant, oracle):
    rows, C = table.rows, table.n_cols
    n_cols = C + 1
    wit = T.TableWitness(ctx, table, {0: (0, rows)}, variant)
    want_rw, want_rown = mp2.row_digests(ctx, table.col_ids, table.values, table.values[:, 0:1, :], variant)
    assert np.array_equal(want_rown, wit.row_own)
    if oracle:
        orc = TO.OracleTableWitness(table, {0: (0, rows)}, variant)
        assert np.array_equal(wit.cell_digest, orc.cell_digest) and np.array_equal(want_rw, orc.row_w) and np.array_equal(want_rown, orc.row_own)
    d_values = ctx.to_device(table.values)
    d_unique = ctx.to_device(np.ascontiguousarray(table.values[:, 0, :]))
    # every row
    d_nodes, d_own = ctx.alloc(rows * C * FB), ctx.alloc(rows * FB)
    mp2.cells_tree_digests_dev(ctx, variant, table.col_ids, d_values, rows, d_nodes)
    assert np.array_equal(mp2.curve_emit_dev(ctx, d_nodes, rows * C)[1].reshape(rows, C, 11), wit.cell_digest)
    for cells_nodes, unique, stride in ((None, d_unique, 8), (d_nodes, d_unique, 8), (d_nodes, d_values, n_cols * 8), (None, d_values, n_cols * 8)):
        d_own.upload(np.full((rows, 20), GARBAGE))
        mp2.row_digests_dev(ctx, variant, table.col_ids, d_values, unique, stride, 1, rows, d_own, cells_nodes)
        w, wei = mp2.curve_emit_dev(ctx, d_own, rows)
        assert np.array_equal(w, want_rw) and np.array_equal(wei, want_rown), (rows, C, variant, cells_nodes is None, stride)
    # listed rows only, with a duplicate
    listed = sorted({0, rows - 1, rows // 2})
    idx = np.array(listed + [listed[-1]], dtype=np.uint32)
    mask = np.zeros(rows, dtype=bool)
    mask[listed] = True
    planted_nodes, planted_own = np.full((rows, C, 20), GARBAGE), np.full((rows, 20), GARBAGE)
    d_nodes.upload(planted_nodes)
    mp2.cells_tree_digests_dev(ctx, variant, table.col_ids, d_values, rows, d_nodes, idx)
    assert np.array_equal(d_nodes.download((rows, C, 20))[~mask], planted_nodes[~mask])
    flat = (np.array(listed)[:, None] * C + np.arange(C)[None, :]).ravel().astype(np.uint32)
    assert np.array_equal(mp2.curve_emit_dev(ctx, d_nodes, 0, flat)[1].reshape(len(listed), C, 11), wit.cell_digest[listed])
    for cells_nodes in (None, d_nodes):
        d_own.upload(planted_own)
        mp2.row_digests_dev(ctx, variant, table.col_ids, d_values, d_values, n_cols * 8, 1, rows, d_own, cells_nodes, idx)
        assert np.array_equal(d_own.download((rows, 20))[~mask], planted_own[~mask])
        w, wei = mp2.curve_emit_dev(ctx, d_own, 0, np.array(listed, dtype=np.uint32))
        assert np.array_equal(w, want_rw[listed]) and np.array_equal(wei, want_rown[listed])
    # an empty list: nothing written
    d_own.upload(planted_own)
    d_nodes.upload(planted_nodes)
    mp2.cells_tree_digests_dev(ctx, variant, table.col_ids, d_values, rows, d_nodes, [])
    mp2.row_digests_dev(ctx, variant, table.col_ids, d_values, d_values, n_cols * 8, 1, rows, d_own, d_nodes, [])
    assert np.array_equal(d_own.download((rows, 20)), planted_own) and np.array_equal(d_nodes.download((rows, C, 20)), planted_nodes)
    free(d_values, d_unique, d_nodes, d_own)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 7])
def test_cells_and_rows_of_small_tables(ctx, mp2, C, variant):
    check_table(ctx, mp2, T.SyntheticTable(5, n_cols=C, seed=0xD16 + C), variant, oracle=True)


@pytest.mark.parametrize("variant", [0, 1])
def test_cells_and_rows_across_a_block_boundary(ctx, mp2, variant):
    check_table(ctx, mp2, T.SyntheticTable(129, n_cols=4, seed=0xD17), variant, oracle=False)


@pytest.mark.parametrize("variant", [0, 1])
def test_a_table_without_cells(ctx, mp2, variant):
    """n_cols == 1: d_nodes is not touched (not even looked at) and d_cells_nodes is ignored"""
    table = T.SyntheticTable(5, n_cols=2, seed=0xD18)
    ids, values = table.col_ids[:1], np.ascontiguousarray(table.values[:, :1])
    want_w, want_wei = mp2.row_digests(ctx, ids, values, values, variant)
    d_values, d_own, d_junk = ctx.to_device(values), ctx.alloc(5 * FB), ctx.to_device(np.full((5, 20), GARBAGE))
    mp2.cells_tree_digests_dev(ctx, variant, ids, d_values, 5, None)
    mp2.cells_tree_digests_dev(ctx, variant, ids, d_values, 5, d_junk)
    for cells_nodes in (None, d_junk):
        mp2.row_digests_dev(ctx, variant, ids, d_values, d_values, 8, 1, 5, d_own, cells_nodes)
        w, wei = mp2.curve_emit_dev(ctx, d_own, 5)
        assert np.array_equal(w, want_w) and np.array_equal(wei, want_wei)
    assert (d_junk.download((5, 20)) == GARBAGE).all()
    free(d_values, d_own, d_junk)


# ---- everything, kept on the device ---------------------------------------------------------------------------------------------------
def same_as_witness(td, wit, rows):
    assert np.array_equal(td.cell_digests(), wit.cell_digest)
    assert np.array_equal(td.row_own(), wit.row_own)
    w, wei = td.row_digests()
    for k in range(rows):
        assert np.array_equal(wei[k], wit.row_digest[k]) and np.array_equal(w[k], wit.root_digest_w[k]), k
    roots = td.shape.describe()["roots"]
    rw, rwei = td.root_digests()
    assert np.array_equal(rw, w[roots]) and np.array_equal(rwei, wei[roots])
    some = [rows - 1, 0, 3]
    assert np.array_equal(td.row_digests(some)[0], w[some]) and np.array_equal(td.row_own(some), wit.row_own[some])
    assert np.array_equal(td.cell_digests(some), wit.cell_digest[some])


@pytest.mark.parametrize("variant", [0, 1])
def test_table_digests_kept_current(ctx, mp2, variant):
    rows = 37
    table = T.SyntheticTable(rows, n_cols=4, seed=0xD19)
    root, _, spans = T.balanced_bst(rows)
    left, right = TC.balanced(rows)
    shape = IX.TreeShape.from_children(left, right)
    td = IX.TableDigests(ctx, table.col_ids, table.values, shape, variant)
    same_as_witness(td, T.TableWitness(ctx, table, spans, variant), rows)
    now = copy.copy(table)
    now.values = table.values.copy()
    rng = np.random.default_rng(0xD1A + variant)
    for changed in ([5], [2, 20, 36], [root]):
        new = rng.integers(0, 1 << 32, size=(len(changed), 5, 8), dtype=np.uint32)
        touched = td.update(changed, new)
        assert touched.tolist() == TT.closure(left, right, changed)[0] == shape.touched(changed).tolist()
        now.values[changed] = new
        same_as_witness(td, T.TableWitness(ctx, now, spans, variant), rows)
    assert td.update([], np.zeros((0, 5, 8), dtype=np.uint32)).size == 0
    td.free()
    shape.free()


def test_an_empty_table(ctx, mp2):
    shape = IX.TreeShape.from_children([], [])
    td = IX.TableDigests(ctx, np.array([7, 8, 9], dtype=np.uint64), np.zeros((0, 3, 8), dtype=np.uint32), shape)
    assert td.row_digests()[0].shape == (0, 5) and td.cell_digests().shape == (0, 2, 11) and td.row_own().shape == (0, 11)
    td.free()
    shape.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def refused(mp2, match, call, *args):
    """the wrapper raises / the raw entry returns non-zero, and the message names the fault"""
    if hasattr(call, "restype"):  # a raw library entry
        assert call(*args) != 0
        assert match in mp2.load().mp2g_last_error().decode(), mp2.load().mp2g_last_error().decode()
    else:
        with pytest.raises(mp2.Mp2gError, match=match):
            call(*args)


def test_refusals_launch_nothing(ctx, mp2):
    lib = mp2.load()
    table = T.SyntheticTable(5, n_cols=3, seed=0xD1B)
    ids, rows, n_cols = table.col_ids, 5, 4
    left, right = TC.sbbst(37)
    s = IX.TreeShape.from_children(left, right)
    sent_pts, sent_nodes, sent_own = np.full((38, 20), GARBAGE), np.full((rows, 3, 20), GARBAGE), np.full((rows, 20), GARBAGE)
    d_own, d_acc = ctx.to_device(sent_pts), ctx.to_device(sent_pts)
    d_values, d_nodes, d_rown = ctx.to_device(table.values), ctx.to_device(sent_nodes), ctx.to_device(sent_own)
    # the tree passes
    refused(mp2, "overlap", mp2.tree_digests_dev, ctx, s, d_own, d_own)
    refused(mp2, "overlap", mp2.tree_digests_dev, ctx, s, d_own, d_own.ptr.value + FB)
    refused(mp2, "overlap", mp2.tree_digests_update_dev, ctx, s, d_acc.ptr.value + 36 * FB, [3], d_acc)
    refused(mp2, "touched index 37 is outside the shape's 37 nodes", mp2.tree_digests_update_dev, ctx, s, d_own, [3, 37], d_acc)
    refused(mp2, "touched list missing", lib.mp2g_tree_digests_update_dev, ctx, s.h, d_own, None, 2, d_acc)
    refused(mp2, "shape", lib.mp2g_tree_digests_dev, ctx, None, d_own, d_acc)
    # the cells trees and the rows: what the hash calls refuse
    bad_ids = ids.copy()
    bad_ids[2] = EC.P
    cells = lambda *a: mp2.cells_tree_digests_dev(ctx, *a)  # noqa: E731
    refused(mp2, "variant", cells, 2, ids, d_values, rows, d_nodes)
    refused(mp2, "n_cols", cells, 0, ids[:0], d_values, rows, d_nodes)
    refused(mp2, "n_cols", cells, 0, np.zeros(257, dtype=np.uint64), d_values, rows, d_nodes)
    refused(mp2, "column identifier not canonical", cells, 0, bad_ids, d_values, rows, d_nodes)
    refused(mp2, "row index 5 is outside the table's 5 rows", cells, 0, ids, d_values, rows, d_nodes, [1, 5])
    refused(mp2, "row_idx list missing", lib.mp2g_cells_tree_digests_dev, ctx, 0, mp2._p(ids), n_cols, d_values, rows, None, 2, d_nodes)
    own = lambda variant, i, stride, n_unique, idx=None: mp2.row_digests_dev(ctx, variant, i, d_values, d_values, stride, n_unique, rows, d_rown, d_nodes, idx)  # noqa: E731
    refused(mp2, "variant", own, 3, ids, 32, 1)
    refused(mp2, "n_cols", own, 0, ids[:0], 32, 1)
    refused(mp2, "column identifier not canonical", own, 0, bad_ids, 32, 1)
    refused(mp2, "row index 9 is outside the table's 5 rows", own, 0, ids, 32, 1, [9])
    refused(mp2, "unique_stride 7 is below", own, 0, ids, 7, 1)
    refused(mp2, "unique_stride 8 is below", own, 0, ids, 8, 2)
    refused(mp2, "row_idx list missing", lib.mp2g_row_digests_dev, ctx, 0, mp2._p(ids), n_cols, d_values, d_values, 32, 1, rows, d_nodes, None, 1, d_rown)
    refused(mp2, "unique columns missing", lib.mp2g_row_digests_dev, ctx, 0, mp2._p(ids), n_cols, d_values, None, 32, 1, rows, d_nodes, None, 0, d_rown)
    # a shape that another context used first
    other = mp2.Context(0)
    o_own, o_acc = other.to_device(sent_pts), other.to_device(sent_pts)
    mp2.tree_digests_update_dev(ctx, s, d_own, [], d_acc)  # nothing touched: returns before the shape is bound
    d_pts = decoded(ctx, mp2, EC.base_points(37))
    d_out = ctx.alloc(37 * FB)
    mp2.tree_digests_dev(ctx, s, d_pts, d_out)  # binds the shape to ctx
    refused(mp2, "another context", lib.mp2g_tree_digests_dev, other, s.h, o_own, o_acc)
    refused(mp2, "another context", lib.mp2g_tree_digests_update_dev, other, s.h, o_own, mp2._p(np.array([1], dtype=np.uint32)), 1, o_acc)
    assert np.array_equal(o_own.download((38, 20)), sent_pts) and np.array_equal(o_acc.download((38, 20)), sent_pts)
    other.close()
    # nothing was written anywhere
    assert np.array_equal(d_own.download((38, 20)), sent_pts) and np.array_equal(d_acc.download((38, 20)), sent_pts)
    assert np.array_equal(d_nodes.download((rows, 3, 20)), sent_nodes) and np.array_equal(d_rown.download((rows, 20)), sent_own)
    free(d_own, d_acc, d_values, d_nodes, d_rown, d_pts, d_out)
    s.free()
