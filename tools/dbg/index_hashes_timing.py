"""time the node hashes of a table's trees on the device (mp2g_cells_tree_hashes_dev + mp2g_row_tree_hashes_dev, what
indexing.table_hashes chains) at 2^20 rows x 4 cells with a balanced row tree, and in the same call the per-level Python path
(indexing.cell_node_hashes / row_node_hashes as table.expected_root_public_inputs drives them) at 2^14 rows:
    python tools/dbg/index_hashes_timing.py [log_rows [log_rows_python]]
device: device events (mp2g_timer_*) around a window of repetitions sized to a few hundred milliseconds after a warm-up, three
windows; the python path: wall clock around calls that each end in a download (a synchronise), one warm-up, then three runs.
Prints permutations per second as 17 * rows / time (4 cells x 3 + 5 per row) and its ratio to README's lone-commitment leaf-sponge
rate (2.4 - 2.8 G perm/s). At 2^14 rows the two paths' results are compared word for word before anything is timed."""
import importlib, math, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mp2 = importlib.import_module("mapreduce-plonky2_amd")
T = importlib.import_module("mapreduce-plonky2_amd.table")
IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
LOG_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
LOG_PY = int(sys.argv[2]) if len(sys.argv) > 2 else 14
CELLS, WINDOW_MS, README_RATE = 4, 300.0, (2.4e9, 2.8e9)


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


def python_path(ctx, table, left, right, height, spans):
    """the composition table.expected_root_public_inputs makes: one batched launch per tree level, packed with numpy"""
    rows, C = table.rows, table.n_cols
    empty = IX.empty_poseidon_hash(ctx)
    ints = lambda a: [sum(int(x) << (32 * (7 - j)) for j, x in enumerate(v)) for v in a]
    cell_h = {}
    for k in sorted(range(1, C + 1), key=lambda k: ((k & -k).bit_length(), k)):
        l, r = T.sbbst_children(C, k)
        lh = cell_h[l] if l is not None else np.tile(empty, (rows, 1))
        rh = cell_h[r] if r is not None else np.tile(empty, (rows, 1))
        cell_h[k] = IX.cell_node_hashes(ctx, lh, rh, np.full(rows, table.col_ids[k]), ints(table.values[:, k]))
    cells_root = cell_h[T.sbbst_root(C)]
    sec = ints(table.values[:, 0])
    row_h = np.zeros((rows, 4), dtype=np.uint64)
    for lvl in range(int(height.max()) + 1):
        ks = np.nonzero(height == lvl)[0]
        lh = np.where((left[ks] >= 0)[:, None], row_h[np.maximum(left[ks], 0)], empty)
        rh = np.where((right[ks] >= 0)[:, None], row_h[np.maximum(right[ks], 0)], empty)
        row_h[ks] = IX.row_node_hashes(ctx, lh, rh, [sec[spans[k][0]] for k in ks], [sec[spans[k][1] - 1] for k in ks],
                                       np.full(len(ks), table.col_ids[0]), [sec[k] for k in ks], cells_root[ks])
    return row_h, cells_root


def windows(ctx, call):
    """per-call milliseconds of three windows of repetitions, each window at least WINDOW_MS long"""
    call(); ctx.sync()  # warm-up: code objects, the shape's upload, the context's working buffer
    ctx.timer_start(); call(); one = ctx.timer_stop()
    reps = max(3, math.ceil(WINDOW_MS / max(one, 1e-3)))
    out = []
    for _ in range(3):
        ctx.timer_start()
        for _ in range(reps):
            call()
        out.append(ctx.timer_stop() / reps)  # timer_stop waits for its event: the window ends in a synchronise
    return reps, out


def report(name, rows, perms_per_row, ms):
    med = statistics.median(ms)
    rate = perms_per_row * rows / (med * 1e-3)
    print(f"{name}: {' '.join(f'{x:.3f}' for x in ms)} ms per call, median {med:.3f} ms; {rate / 1e9:.3f} G perm/s = "
          f"{rate / README_RATE[1]:.2f} - {rate / README_RATE[0]:.2f} of the lone-commitment leaf sponge (2.8 - 2.4 G perm/s)")


ctx = mp2.Context(0)
# ---- 2^LOG_PY rows: both paths, compared, then the python path timed --------------------------------------------------------------
rows = 1 << LOG_PY
table = T.SyntheticTable(rows, n_cols=CELLS)
_, _, spans = T.balanced_bst(rows)
left, right = balanced_children(rows)
shape = IX.TreeShape.from_children(left, right)
height = shape.describe()["height"]
want = python_path(ctx, table, left, right, height, spans)
got = IX.table_hashes(ctx, table.col_ids, table.values, shape)
assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "device path != per-level python path"
py = []
for _ in range(3):
    t0 = time.perf_counter()
    python_path(ctx, table, left, right, height, spans)
    py.append((time.perf_counter() - t0) * 1e3)
print(f"rows 2^{LOG_PY}, {CELLS} cells, balanced row tree of {shape.num_levels} levels: results equal")
report(f"per-level python path (wall clock, host packing included), 2^{LOG_PY} rows", rows, 3 * CELLS + 5, py)
t0 = time.perf_counter()
IX.table_hashes(ctx, table.col_ids, table.values, shape)
print(f"indexing.table_hashes end to end (upload, two calls, download), 2^{LOG_PY} rows: {(time.perf_counter() - t0) * 1e3:.3f} ms wall clock")
shape.free()

# ---- 2^LOG_ROWS rows: the two _dev calls between device events -----------------------------------------------------------------------
rows = 1 << LOG_ROWS
table = T.SyntheticTable(rows, n_cols=CELLS)
t0 = time.perf_counter()
shape = IX.TreeShape.from_children(*balanced_children(rows))
t1 = time.perf_counter()
shape2 = IX.TreeShape.from_children(shape.describe()["left"], shape.describe()["right"])
print(f"rows 2^{LOG_ROWS}: children arrays in python {(t1 - t0) * 1e3:.1f} ms; mp2g_tree_shape_create alone {(time.perf_counter() - t1) * 1e3:.1f} ms (host), "
      f"{shape.num_levels} levels")
shape2.free()
ids = np.ascontiguousarray(table.col_ids, dtype=np.uint64)
d_values, d_cells, d_rows = ctx.to_device(table.values), ctx.alloc(rows * 32), ctx.alloc(rows * 32)
cells = lambda: mp2.cells_tree_hashes_dev(ctx, 0, ids, d_values, rows, d_cells)
rowt = lambda: mp2.row_tree_hashes_dev(ctx, 0, shape, ids[0], d_values, ids.size * 8, d_cells, d_rows)
both = lambda: (cells(), rowt())
for name, call, perms in (("cells trees", cells, 3 * CELLS), ("row tree", rowt, 5), ("both (table_hashes' device work)", both, 3 * CELLS + 5)):
    reps, ms = windows(ctx, call)
    report(f"{name}, 2^{LOG_ROWS} rows, {reps} calls per window", rows, perms, ms)
for d in (d_values, d_cells, d_rows):
    d.free()
shape.free()
ctx.close()
