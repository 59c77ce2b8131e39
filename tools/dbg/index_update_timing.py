"""time the update of a table's node hashes after a block that changes k rows (mp2g_cells_tree_hashes_rows_dev +
mp2g_row_tree_hashes_update_dev, what indexing.TableHashes.update chains) beside the full rebuild (mp2g_cells_tree_hashes_dev +
mp2g_row_tree_hashes_dev) in the same run, on a balanced row tree over rows x 4 cells:
    python tools/dbg/index_update_timing.py [log_rows ...]        (default: 14 20)
per size: the full rebuild; Poseidon2 updates of k = 1, 8, 64, 512 random rows and of exactly W and W + 1 leaves of the row tree
(W = mp2g_row_tree_update_fused_width(): the last closure the fused kernel takes and the first that goes level by level); original
Poseidon at k = 8 (level by level at a size where Poseidon2 is fused); the host time of mp2g_tree_shape_touched for each list.
Method as tools/dbg/index_hashes_timing.py: device events (mp2g_timer_*) around a window of repetitions sized to at least 300 ms
after a warm-up, three windows. Before anything is timed, one update is compared word for word with a full rebuild of the changed
table."""
import importlib, math, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mp2 = importlib.import_module("mapreduce-plonky2_amd")
T = importlib.import_module("mapreduce-plonky2_amd.table")
IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
LOGS = [int(a) for a in sys.argv[1:]] or [14, 20]
CELLS, WINDOW_MS = 4, 300.0


def balanced_children(n):
    """left / right of the BST a full rebuild gives (node = midpoint of its range), without recursion"""
    left, right = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    todo = [(0, n)]
    while todo:
        lo, hi = todo.pop()
        mid = (lo + hi) // 2
        if lo < mid:
            left[mid] = (lo + mid) // 2
            todo.append((lo, mid))
        if mid + 1 < hi:
            right[mid] = (mid + 1 + hi) // 2
            todo.append((mid + 1, hi))
    return left, right


def windows(ctx, call):
    """per-call milliseconds of three windows of repetitions, each window at least WINDOW_MS long"""
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


def show(name, reps, ms, extra=""):
    print(f"{name}: {' '.join(f'{x:.4f}' for x in ms)} ms per call, median {statistics.median(ms):.4f} ms, {reps} calls per window{extra}", flush=True)


ctx = mp2.Context(0)
W = mp2.row_tree_update_fused_width()
for log_rows in LOGS:
    rows = 1 << log_rows
    table = T.SyntheticTable(rows, n_cols=CELLS)
    shape = IX.TreeShape.from_children(*balanced_children(rows))
    height = shape.describe()["height"]
    ids = np.ascontiguousarray(table.col_ids, dtype=np.uint64)
    values = np.ascontiguousarray(table.values, dtype=np.uint32)
    d_values, d_cells, d_rows = ctx.to_device(values), ctx.alloc(rows * 32), ctx.alloc(rows * 32)
    print(f"---- 2^{log_rows} rows x {CELLS} cells, balanced row tree of {shape.num_levels} levels, fused width W = {W}", flush=True)

    def full(variant=0):
        mp2.cells_tree_hashes_dev(ctx, variant, ids, d_values, rows, d_cells)
        mp2.row_tree_hashes_dev(ctx, variant, shape, ids[0], d_values, ids.size * 8, d_cells, d_rows)

    def update(idx, variant=0):
        mp2.cells_tree_hashes_rows_dev(ctx, variant, ids, d_values, rows, idx, d_cells)
        mp2.row_tree_hashes_update_dev(ctx, variant, shape, ids[0], d_values, ids.size * 8, d_cells, idx, d_rows)

    # one update against a full rebuild of the changed table, word for word
    rng = np.random.default_rng(0x71E + log_rows)
    full()
    idx = rng.choice(rows, size=8, replace=False).astype(np.uint32)
    for r in idx.tolist():
        values[r] = rng.integers(0, 1 << 32, size=values.shape[1:], dtype=np.uint32)
        d_values.upload_at(values[r], r * values.shape[1] * 32)
    update(idx)
    got = d_rows.download((rows, 4)), d_cells.download((rows, 4))
    full()
    assert np.array_equal(got[0], d_rows.download((rows, 4))) and np.array_equal(got[1], d_cells.download((rows, 4))), "update != full rebuild"
    print("update of 8 rows == full rebuild of the changed table", flush=True)

    reps, ms = windows(ctx, full)
    show("full rebuild (cells trees + row tree), Poseidon2", reps, ms)
    rebuild = statistics.median(ms)
    leaves = np.nonzero(height == 0)[0].astype(np.uint32)
    spread = lambda k: leaves[::len(leaves) // (k + 1)][:k]
    lists = [(f"k = {k} random rows", rng.choice(rows, size=k, replace=False).astype(np.uint32), 0) for k in (1, 8, 64, 512)]
    lists += [(f"W = {W} leaves", spread(W), 0), (f"W + 1 = {W + 1} leaves", spread(W + 1), 0)]
    lists.append(("k = 8 random rows, original Poseidon", lists[1][1], 1))
    for name, idx, variant in lists:
        closure = shape.touched(idx)
        levels = np.bincount(height[closure])
        widest, n_levels = int(levels.max()), int((levels > 0).sum())
        path = "fused, 1 launch" if variant == 0 and widest <= W and n_levels <= 256 else f"level by level, {n_levels} launches"
        t0 = time.perf_counter()
        for _ in range(200):
            shape.touched(idx)
        host_us = (time.perf_counter() - t0) / 200 * 1e6
        if variant:
            full(variant)  # the buffers hold this variant's hashes while it is timed
        reps, ms = windows(ctx, lambda: update(idx, variant))
        show(f"update, {name}", reps, ms, f"; closure {closure.size} nodes in {n_levels} levels, widest {widest}: {path}; "
             f"{statistics.median(ms) / rebuild:.4f} of the Poseidon2 rebuild; TreeShape.touched {host_us:.1f} us on the host")
        if variant:
            reps, ms = windows(ctx, lambda: full(variant))
            show("full rebuild, original Poseidon", reps, ms)
            full(0)
    for d in (d_values, d_cells, d_rows):
        d.free()
    shape.free()
ctx.close()
