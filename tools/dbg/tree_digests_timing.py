"""time the accumulated Ecgfp5 digests of a table on the device (mp2g_cells_tree_digests_dev + mp2g_row_digests_dev +
mp2g_tree_digests_dev and the update forms, what indexing.TableDigests chains) beside the path that was there before them
(map_to_curve_batch + curve_sum_ranges for the cells trees, row_digests + curve_sum_ranges for the row tree, as table.TableWitness
chains them), in ONE run, at 2^14 and 2^20 rows x 4 cells with a balanced row tree:
    python tools/dbg/tree_digests_timing.py [log_rows ...]
Method of profiles/index_hashes.md: device events (mp2g_timer_*) around a window of repetitions sized to at least 300 ms after a
warm-up, three windows, median reported. The calls of the earlier path take and return host arrays and end in a synchronise, so their
windows include the copies and the host's packing, which is what a caller of that path pays. At each size the two paths' results
are compared word for word before anything is timed."""
import copy, importlib, math, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mp2 = importlib.import_module("mapreduce-plonky2_amd")
T = importlib.import_module("mapreduce-plonky2_amd.table")
IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
LOGS = [int(a) for a in sys.argv[1:]] or [14, 20]
CELLS, WINDOW_MS, FB = 4, 300.0, mp2.FRAC_BYTES


def balanced(n):
    """left / right / spans [n][2] of the BST a full rebuild gives (node = midpoint of its range), without recursion"""
    left, right = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    spans = np.zeros((n, 2), dtype=np.uint32)
    todo = [(0, n)]
    while todo:
        lo, hi = todo.pop()
        mid = (lo + hi) // 2
        spans[mid] = (lo, hi)
        if lo < mid:
            left[mid] = (lo + mid) // 2
            todo.append((lo, mid))
        if mid + 1 < hi:
            right[mid] = (mid + 1 + hi) // 2
            todo.append((mid + 1, hi))
    return left, right, spans


def windows(ctx, call):
    """(repetitions, per-call milliseconds of three windows), each window at least WINDOW_MS long"""
    call(); ctx.sync()  # warm-up: code objects, the shape's upload, the context's buffers
    ctx.timer_start(); call(); one = ctx.timer_stop()
    reps = max(3, math.ceil(WINDOW_MS / max(one, 1e-3)))
    out = []
    for _ in range(3):
        ctx.timer_start()
        for _ in range(reps):
            call()
        out.append(ctx.timer_stop() / reps)  # timer_stop waits for its event: the window ends in a synchronise
    return reps, out


def report(name, ms_reps):
    reps, ms = ms_reps
    med = statistics.median(ms)
    print(f"  {name}: {' '.join(f'{x:.4f}' for x in ms)} ms per call ({reps} calls per window), median {med:.4f} ms", flush=True)
    return med


def run(ctx, log_rows):
    rows = 1 << log_rows
    table = T.SyntheticTable(rows, n_cols=CELLS)
    n_cols = CELLS + 1
    ids = np.ascontiguousarray(table.col_ids, dtype=np.uint64)
    left, right, spans = balanced(rows)
    shape = IX.TreeShape.from_children(left, right)
    print(f"rows 2^{log_rows}, {CELLS} cells, balanced row tree of {shape.num_levels} levels", flush=True)

    # ---- the earlier path, stage by stage, as TableWitness chains it ----------------------------------------------------------------
    limbs = table.values.astype(np.uint64)
    cell_in = np.concatenate([np.broadcast_to(ids[None, 1:, None], (rows, CELLS, 1)), limbs[:, 1:, :]], axis=2).reshape(rows * CELLS, 9)
    cell_spans = [T.sbbst_span(CELLS, k) for k in range(1, CELLS + 1)]
    cell_rg = (np.arange(rows, dtype=np.uint32)[:, None, None] * CELLS + np.array([[lo - 1, hi] for lo, hi in cell_spans], dtype=np.uint32)[None]).reshape(-1, 2)
    unique = np.ascontiguousarray(table.values[:, 0:1, :])
    old = {}
    st_map = lambda: old.__setitem__("cell_w", mp2.map_to_curve_batch(ctx, cell_in, 0))
    st_cells = lambda: old.__setitem__("cell", mp2.curve_sum_ranges(ctx, old["cell_w"], cell_rg))
    st_rows = lambda: old.__setitem__("row", mp2.row_digests(ctx, ids, table.values, unique, 0))
    st_tree = lambda: old.__setitem__("acc", mp2.curve_sum_ranges(ctx, old["row"][0], spans))
    old_all = lambda: (st_map(), st_cells(), st_rows(), st_tree())
    old_all()

    # ---- the new path ------------------------------------------------------------------------------------------------------------------
    td = IX.TableDigests(ctx, ids, table.values, shape)
    assert np.array_equal(td.cell_digests(), old["cell"][1].reshape(rows, CELLS, 11)), "cells-tree digests differ"
    assert np.array_equal(td.row_own(), old["row"][1]), "rows' own digests differ"
    w, wei = td.row_digests()
    assert np.array_equal(w, old["acc"][0]) and np.array_equal(wei, old["acc"][1]), "row-tree digests differ"
    d_own2 = ctx.alloc(rows * FB)
    mp2.row_digests_dev(ctx, 0, ids, td.d_values, td.d_values, n_cols * 8, 1, rows, d_own2)
    assert np.array_equal(mp2.curve_emit_dev(ctx, d_own2, rows)[1], old["row"][1]), "rows' own digests without the cells roots differ"
    print("  results equal, word for word: cells-tree nodes, rows' own digests (with and without the cells roots), row-tree nodes", flush=True)

    print(" the earlier path (host arrays in and out, every call ends in a synchronise)")
    t_old = [report("map_to_curve_batch, cells", windows(ctx, st_map)), report("curve_sum_ranges, cells trees", windows(ctx, st_cells)),
             report("row_digests", windows(ctx, st_rows)), report("curve_sum_ranges, row tree", windows(ctx, st_tree))]
    t_old_all = report("all four", windows(ctx, old_all))
    print(f"  sum of the stages {sum(t_old):.4f} ms")

    print(" the new path (device resident, stream ordered)")
    cells = lambda: mp2.cells_tree_digests_dev(ctx, 0, ids, td.d_values, rows, td.d_cells)
    own_roots = lambda: mp2.row_digests_dev(ctx, 0, ids, td.d_values, td.d_values, n_cols * 8, 1, rows, td.d_own, td.d_cells)
    own_all = lambda: mp2.row_digests_dev(ctx, 0, ids, td.d_values, td.d_values, n_cols * 8, 1, rows, d_own2)
    tree = lambda: mp2.tree_digests_dev(ctx, shape, td.d_own, td.d_acc)
    full = lambda: (cells(), own_roots(), tree())
    emit = lambda: (td.cell_digests(), td.row_own(), td.row_digests())
    t_cells = report("cells_tree_digests_dev", windows(ctx, cells))
    t_own = report("row_digests_dev with the cells roots", windows(ctx, own_roots))
    t_own_all = report("row_digests_dev mapping every column", windows(ctx, own_all))
    t_tree = report("tree_digests_dev", windows(ctx, tree))
    t_full = report("full pass (the three calls)", windows(ctx, full))
    t_emit = report("encode + download everything (cells nodes, own, accumulated)", windows(ctx, emit))
    print(f"  full pass {t_full:.4f} ms + downloads {t_emit:.4f} ms = {t_full + t_emit:.4f} ms against the earlier path's {t_old_all:.4f} ms: "
          f"{t_old_all / (t_full + t_emit):.2f}x; device work alone {t_old_all / t_full:.2f}x", flush=True)
    print(f"  row_digests_dev: {t_own_all / t_own:.2f}x with the cells roots; tree pass against curve_sum_ranges over the row tree: {t_old[3] / t_tree:.2f}x")

    print(" updates (the earlier path recomputes the whole table: its 'all four' above)")
    rng = np.random.default_rng(0x71E + log_rows)
    for k in (1, 8, 64, 512):
        changed = rng.choice(rows, size=k, replace=False).astype(np.uint32)
        new = rng.integers(0, 1 << 32, size=(k, n_cols, 8), dtype=np.uint32)
        closure = shape.touched(changed).size
        t_upd = report(f"TableDigests.update of {k} rows (row uploads included), closure {closure} nodes", windows(ctx, lambda: td.update(changed, new)))
        dev = lambda: (mp2.cells_tree_digests_dev(ctx, 0, ids, td.d_values, rows, td.d_cells, changed),
                       mp2.row_digests_dev(ctx, 0, ids, td.d_values, td.d_values, n_cols * 8, 1, rows, td.d_own, td.d_cells, changed),
                       mp2.tree_digests_update_dev(ctx, shape, td.d_own, changed, td.d_acc))
        t_dev = report(f"  its three device calls alone", windows(ctx, dev))
        t_tr = report(f"  tree_digests_update_dev alone", windows(ctx, lambda: mp2.tree_digests_update_dev(ctx, shape, td.d_own, changed, td.d_acc)))
        print(f"    {k} rows: {t_old_all / t_upd:.0f}x the earlier path ({t_old_all:.3f} ms); full pass / update {t_full / t_dev:.1f}x")
    if log_rows <= 14:  # the table is as the updates left it: compare once more against the earlier path on the same values
        t2 = copy.copy(table)
        t2.values = td.d_values.download((rows, n_cols, 8), np.uint32)
        wit = T.TableWitness(ctx, t2, {k: tuple(int(x) for x in spans[k]) for k in range(rows)}, 0)
        w, wei = td.row_digests()
        assert all(np.array_equal(wei[k], wit.row_digest[k]) for k in range(rows)) and np.array_equal(td.cell_digests(), wit.cell_digest)
        print("  after the updates: equal to a TableWitness of the changed table")

    W = mp2.tree_digests_update_fused_width()
    height = shape.describe()["height"]
    leaves = np.flatnonzero(height == 0).astype(np.uint32)
    print(f" the fused width W = {W}: W and W + 1 leaves spread over the tree (tree_digests_update_dev alone)")
    for width in (W // 2, W, W + 1, 2 * W):
        if width > leaves.size:
            continue
        touched = leaves[::leaves.size // width][:width]
        nodes = shape.touched(touched)
        hs = height[nodes]
        widest, levels = int(np.bincount(hs).max()), int(np.unique(hs).size)
        path = "fused, one launch" if widest <= W and levels <= 256 else f"level by level, {levels} launches"
        report(f"{width} leaves: closure {nodes.size} nodes, {levels} levels, widest {widest} -> {path}",
               windows(ctx, lambda: mp2.tree_digests_update_dev(ctx, shape, td.d_own, touched, td.d_acc)))
    d_own2.free()
    td.free()
    shape.free()


ctx = mp2.Context(0)
for lr in LOGS:
    run(ctx, lr)
ctx.close()
