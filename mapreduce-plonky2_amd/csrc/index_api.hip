// C ABI of the tree shapes and the node hashes of a table's trees (include/mp2g.h), over tree_shape.h and the kernels of
// index_hash.hip. Every argument is judged on the host before anything is launched.
#include "index_api.h"
#include <algorithm>

using namespace mp2g;

static int shape_new(const int32_t* left, const int32_t* right, uint32_t n, mp2g_tree_shape** out) {
  mp2g_tree_shape* t = new (std::nothrow) mp2g_tree_shape();
  if (!t) return fail("out of memory");
  const char* err;
  try {
    err = tree_shape_build(left, right, n, t->s);
  } catch (...) {
    delete t;
    throw;  // to guarded()
  }
  if (err) { delete t; return fail("invalid tree shape: %s", err); }
  *out = t;
  return 0;
}

extern "C" {

int mp2g_tree_shape_create(const int32_t* left, const int32_t* right, uint32_t n, mp2g_tree_shape** out) {
  NEED(out && ((left && right) || !n), "out / left / right");
  return guarded([&] { return shape_new(left, right, n, out); });
}
int mp2g_tree_shape_sbbst(uint32_t n, mp2g_tree_shape** out) {
  NEED(out, "out");
  NEED(n <= 0x7FFFFFFFu, "n <= 2^31 - 1");
  return guarded([&] {
    std::vector<int32_t> l(n), r(n);
    sbbst_fill(n, l.data(), r.data());
    return shape_new(l.data(), r.data(), n, out);
  });
}
uint32_t mp2g_tree_shape_size(const mp2g_tree_shape* t) { return t ? t->s.size() : 0; }
uint32_t mp2g_tree_shape_num_levels(const mp2g_tree_shape* t) { return t ? t->s.levels() : 0; }
uint32_t mp2g_tree_shape_num_roots(const mp2g_tree_shape* t) { return t ? (uint32_t)t->s.roots.size() : 0; }
int mp2g_tree_shape_describe(const mp2g_tree_shape* t, int32_t* left, int32_t* right, uint32_t* height, uint32_t* min_idx,
                             uint32_t* max_idx, uint32_t* roots) {
  NEED(t, "shape");
  const size_t n = t->s.size();
  for (size_t i = 0; i < n; i++) {
    if (left) left[i] = t->s.left[i];
    if (right) right[i] = t->s.right[i];
    if (height) height[i] = t->s.height[i];
    if (min_idx) min_idx[i] = t->s.min_idx[i];
    if (max_idx) max_idx[i] = t->s.max_idx[i];
  }
  if (roots)
    for (size_t i = 0; i < t->s.roots.size(); i++) roots[i] = t->s.roots[i];
  return 0;
}
int mp2g_tree_shape_touched(const mp2g_tree_shape* t, const uint32_t* touched, uint32_t n_touched, uint32_t* nodes, uint32_t cap,
                            uint32_t* n_nodes) {
  NEED(t && n_nodes, "shape / n_nodes");
  NEED(touched || !n_touched, "touched list missing");
  return guarded([&] {
    TreeTouched c;
    if (tree_shape_touched(t->s, touched, n_touched, c)) return fail("invalid argument: %s", c.err);
    *n_nodes = (uint32_t)c.nodes.size();
    if (!nodes) return 0;
    if (cap < c.nodes.size()) return fail("invalid argument: cap %u is below the closure's %zu nodes", cap, c.nodes.size());
    std::copy(c.nodes.begin(), c.nodes.end(), nodes);
    return 0;
  });
}
uint32_t mp2g_row_tree_update_fused_width(void) { return MP2G_ROW_UPDATE_FUSED_WIDTH; }
void mp2g_tree_shape_free(mp2g_tree_shape* t) {
  delete t;  // hipFree of the device arrays waits for every kernel that may still read them
}

// ---- cells trees -----------------------------------------------------------------------------
// the context's working buffer, grown when a call needs more
static int cells_work(mp2g_ctx* c, size_t work_bytes) {
  if (c->index_work.bytes < work_bytes) {
    CK(hipStreamSynchronize(c->stream));  // a kernel queued earlier may still use the old buffer
    CK(c->index_work.alloc(work_bytes));
  }
  return 0;
}
int mp2g_cells_tree_hashes_dev(mp2g_ctx* c, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* d_values,
                               uint32_t rows, uint64_t* d_roots, uint64_t* d_nodes) {
  int rc = cells_args(variant, col_ids, n_cols, rows);
  if (rc) return rc;
  if (!rows) return 0;
  NEED(c && d_roots, "ctx / roots");
  NEED(aligned16(d_roots) && aligned16(d_nodes), "digest buffers must be 16-byte aligned");
  const uint32_t cells = n_cols - 1;
  if (!cells) {  // row.rs:299-302: a row without cells carries hash_no_pad(&[])
    CK(cells_empty_roots(c->stream, (u64*)d_roots, rows));
    return 0;
  }
  NEED(d_values, "values");
  rc = cells_work(c, (size_t)cells * rows * 4 * sizeof(u64));
  if (rc) return rc;
  return cells_levels(col_ids, cells, [&](const CellsLevel& lv, uint32_t count, int root) {
    CK(cells_level_hash(c->stream, variant, lv, count, d_values, n_cols, rows, c->index_work.p, (u64*)d_nodes, (u64*)d_roots, root));
    return 0;
  });
}
// the listed rows only: the schedule above with a row indirection and a compact working buffer
int mp2g_cells_tree_hashes_rows_dev(mp2g_ctx* c, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* d_values,
                                    uint32_t rows, const uint32_t* row_idx, uint32_t n_idx, uint64_t* d_roots, uint64_t* d_nodes) {
  int rc = cells_rows_args(variant, col_ids, n_cols, rows, row_idx, n_idx);
  if (rc) return rc;
  if (!n_idx) return 0;
  NEED(aligned16(d_roots) && aligned16(d_nodes), "digest buffers must be 16-byte aligned");
  NEED(c && d_roots, "ctx / roots");
  const uint32_t cells = n_cols - 1;
  NEED(d_values || !cells, "values");
  const u32* d_idx;
  rc = stage_lists(c, row_idx, n_idx, nullptr, 0, &d_idx);
  if (rc) return rc;
  if (!cells) {  // row.rs:299-302
    CK(cells_rows_empty_roots(c->stream, (u64*)d_roots, d_idx, n_idx));
    return 0;
  }
  rc = cells_work(c, (size_t)cells * n_idx * 4 * sizeof(u64));
  if (rc) return rc;
  return cells_levels(col_ids, cells, [&](const CellsLevel& lv, uint32_t count, int root) {
    CK(cells_rows_level_hash(c->stream, variant, lv, count, d_values, n_cols, d_idx, n_idx, c->index_work.p, (u64*)d_nodes, (u64*)d_roots,
                             root));
    return 0;
  });
}
int mp2g_cells_tree_hashes_rows(mp2g_ctx* c, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* values, uint32_t rows,
                                const uint32_t* row_idx, uint32_t n_idx, uint64_t* roots, uint64_t* nodes) {
  int rc = cells_rows_args(variant, col_ids, n_cols, rows, row_idx, n_idx);
  if (rc) return rc;
  if (!n_idx) return 0;
  NEED(c && roots && (values || n_cols == 1), "ctx / roots / values");
  const size_t cells = n_cols - 1, vbytes = (size_t)rows * n_cols * 32;
  // the device's view of roots / nodes: only the listed rows of it are meaningful, and only they are copied out. Declared before
  // the device buffers, whose release waits for the device: a copy still in flight on an error path ends before these go
  std::vector<u64> hr, hn;
  DevBuf dv, dr, dn;
  rc = guarded([&] {
    hr.resize((size_t)rows * 4);
    if (nodes && cells) hn.resize((size_t)rows * cells * 4);
    return 0;
  });
  if (rc) return rc;
  if (cells) CK(dv.alloc(vbytes));
  CK(dr.alloc((size_t)rows * 32));
  if (nodes && cells) CK(dn.alloc(rows * cells * 32));
  if (cells) CK(hipMemcpyAsync(dv.p, values, vbytes, hipMemcpyHostToDevice, c->stream));
  rc = mp2g_cells_tree_hashes_rows_dev(c, variant, col_ids, n_cols, (const u32*)dv.p, rows, row_idx, n_idx, dr.p, dn.p);
  if (rc) return rc;
  CK(hipMemcpyAsync(hr.data(), dr.p, (size_t)rows * 32, hipMemcpyDeviceToHost, c->stream));
  if (dn.p) CK(hipMemcpyAsync(hn.data(), dn.p, rows * cells * 32, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  for (uint32_t j = 0; j < n_idx; j++) {
    const size_t r = row_idx[j];
    std::copy(hr.begin() + r * 4, hr.begin() + r * 4 + 4, roots + r * 4);
    if (dn.p) std::copy(hn.begin() + r * cells * 4, hn.begin() + (r + 1) * cells * 4, nodes + r * cells * 4);
  }
  return 0;
}
int mp2g_cells_tree_hashes(mp2g_ctx* c, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* values, uint32_t rows,
                           uint64_t* roots, uint64_t* nodes) {
  int rc = cells_args(variant, col_ids, n_cols, rows);
  if (rc) return rc;
  if (!rows) return 0;
  NEED(c && roots && (values || n_cols == 1), "ctx / roots / values");
  const size_t cells = n_cols - 1, vbytes = (size_t)rows * n_cols * 32;
  DevBuf dv, dr, dn;
  if (cells) CK(dv.alloc(vbytes));  // a table without cells is neither uploaded nor read
  CK(dr.alloc((size_t)rows * 32));
  if (nodes && cells) CK(dn.alloc(rows * cells * 32));
  if (cells) CK(hipMemcpyAsync(dv.p, values, vbytes, hipMemcpyHostToDevice, c->stream));
  rc = mp2g_cells_tree_hashes_dev(c, variant, col_ids, n_cols, (const u32*)dv.p, rows, dr.p, dn.p);
  if (rc) return rc;
  CK(hipMemcpyAsync(roots, dr.p, (size_t)rows * 32, hipMemcpyDeviceToHost, c->stream));
  if (dn.p) CK(hipMemcpyAsync(nodes, dn.p, rows * cells * 32, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- row tree / index tree ---------------------------------------------------------------------
// words of `values` a shape of n nodes reads: (n - 1) * stride + 8; refused when the byte count does not fit 64 bits
static int row_args(int variant, const mp2g_tree_shape* t, uint64_t id, uint32_t value_stride, size_t* value_words) {
  NEED(variant == 0 || variant == 1, "variant");
  NEED(t, "shape");
  NEED(id < GL_P, "identifier not canonical (>= p)");
  NEED(value_stride >= 8, "value_stride >= 8 (a value is 8 words)");
  const uint64_t n = t->s.size();
  *value_words = n ? (size_t)((n - 1) * value_stride + 8) : 0;  // n < 2^31, stride < 2^32: below 2^63 words
  NEED(*value_words <= (SIZE_MAX >> 2), "values size overflows");
  return 0;
}
int mp2g_row_tree_hashes_dev(mp2g_ctx* c, int variant, const mp2g_tree_shape* t, uint64_t id, const uint32_t* d_values,
                             uint32_t value_stride, const uint64_t* d_payload, uint64_t* d_hashes) {
  size_t words;
  int rc = row_args(variant, t, id, value_stride, &words);
  if (rc) return rc;
  const size_t n = t->s.size();
  if (!n) return 0;
  NEED(c && d_values && d_hashes, "ctx / values / hashes");
  NEED(aligned16(d_payload) && aligned16(d_hashes), "digest buffers must be 16-byte aligned");
  const u32* d;
  rc = shape_on_device(t, c, &d);
  if (rc) return rc;
  const int32_t *left = (const int32_t*)d, *right = (const int32_t*)(d + n);
  const u32 *mn = d + 2 * n, *mx = d + 3 * n, *order = d + 4 * n;
  for (uint32_t h = 0; h < t->s.levels(); h++) {
    const uint32_t lo = t->s.level_off[h], count = t->s.level_off[h + 1] - lo;
    CK(row_level_hash(c->stream, variant, order + lo, count, left, right, mn, mx, id, d_values, value_stride, (const u64*)d_payload,
                      (u64*)d_hashes));
  }
  return 0;
}
int mp2g_row_tree_hashes(mp2g_ctx* c, int variant, const mp2g_tree_shape* t, uint64_t id, const uint32_t* values, uint32_t value_stride,
                         const uint64_t* payload, uint64_t* hashes) {
  size_t words;
  int rc = row_args(variant, t, id, value_stride, &words);
  if (rc) return rc;
  const size_t n = t->s.size();
  if (!n) return 0;
  NEED(c && values && hashes, "ctx / values / hashes");
  DevBuf dv, dp, dh;
  CK(dv.alloc(words * sizeof(u32)));
  CK(dh.alloc(n * 32));
  if (payload) CK(dp.alloc(n * 32));
  CK(hipMemcpyAsync(dv.p, values, words * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  if (payload) CK(hipMemcpyAsync(dp.p, payload, n * 32, hipMemcpyHostToDevice, c->stream));
  rc = mp2g_row_tree_hashes_dev(c, variant, t, id, (const u32*)dv.p, value_stride, dp.p, dh.p);
  if (rc) return rc;
  CK(hipMemcpyAsync(hashes, dh.p, n * 32, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the touched nodes and their ancestors only (MerkleTreeKvDb::aggregate over touched(), ryhope/src/lib.rs:179-222) ----------------
// everything that is decided on the host: the full call's refusals, the list, the closure
static int row_update_args(int variant, const mp2g_tree_shape* t, uint64_t id, uint32_t value_stride, const uint32_t* touched,
                           uint32_t n_touched, size_t* value_words, TreeTouched& closure) {
  int rc = row_args(variant, t, id, value_stride, value_words);
  if (rc) return rc;
  NEED(touched || !n_touched, "touched list missing");
  return guarded([&] { return tree_shape_touched(t->s, touched, n_touched, closure) ? fail("invalid argument: %s", closure.err) : 0; });
}
static int row_update_launch(mp2g_ctx* c, int variant, const mp2g_tree_shape* t, uint64_t id, const uint32_t* d_values,
                             uint32_t value_stride, const uint64_t* d_payload, const TreeTouched& closure, uint64_t* d_hashes) {
  const size_t n = t->s.size();
  const u32* d;
  int rc = shape_on_device(t, c, &d);
  if (rc) return rc;
  const int32_t *left = (const int32_t*)d, *right = (const int32_t*)(d + n);
  const u32 *mn = d + 2 * n, *mx = d + 3 * n;
  const u32* d_order;
  rc = stage_lists(c, closure.nodes.data(), closure.nodes.size(), closure.level_off.data(), closure.level_off.size(), &d_order);
  if (rc) return rc;
  if (variant == MP2G_POSEIDON2 && closure.widest <= MP2G_ROW_UPDATE_FUSED_WIDTH && closure.levels() <= MP2G_ROW_UPDATE_FUSED_LEVELS) {
    CK(row_update_fused(c->stream, d_order, d_order + closure.nodes.size(), closure.levels(), left, right, mn, mx, id, d_values, value_stride,
                        (const u64*)d_payload, (u64*)d_hashes));
    return 0;
  }
  for (uint32_t l = 0; l < closure.levels(); l++) {
    const uint32_t lo = closure.level_off[l], count = closure.level_off[l + 1] - lo;
    CK(row_level_hash(c->stream, variant, d_order + lo, count, left, right, mn, mx, id, d_values, value_stride, (const u64*)d_payload,
                      (u64*)d_hashes));
  }
  return 0;
}
int mp2g_row_tree_hashes_update_dev(mp2g_ctx* c, int variant, const mp2g_tree_shape* t, uint64_t id, const uint32_t* d_values,
                                    uint32_t value_stride, const uint64_t* d_payload, const uint32_t* touched, uint32_t n_touched,
                                    uint64_t* d_hashes) {
  size_t words;
  TreeTouched closure;
  int rc = row_update_args(variant, t, id, value_stride, touched, n_touched, &words, closure);
  if (rc) return rc;
  if (closure.nodes.empty()) return 0;
  NEED(aligned16(d_payload) && aligned16(d_hashes), "digest buffers must be 16-byte aligned");
  NEED(c && d_values && d_hashes, "ctx / values / hashes");
  return row_update_launch(c, variant, t, id, d_values, value_stride, d_payload, closure, d_hashes);
}
int mp2g_row_tree_hashes_update(mp2g_ctx* c, int variant, const mp2g_tree_shape* t, uint64_t id, const uint32_t* values,
                                uint32_t value_stride, const uint64_t* payload, const uint32_t* touched, uint32_t n_touched,
                                uint64_t* hashes) {
  size_t words;
  TreeTouched closure;
  int rc = row_update_args(variant, t, id, value_stride, touched, n_touched, &words, closure);
  if (rc) return rc;
  if (closure.nodes.empty()) return 0;
  NEED(c && values && hashes, "ctx / values / hashes");
  const size_t n = t->s.size();
  std::vector<u64> back;  // the device's hashes: only the closure's entries are copied out to the caller's (declared first: see above)
  DevBuf dv, dp, dh;
  rc = guarded([&] { back.resize(n * 4); return 0; });
  if (rc) return rc;
  CK(dv.alloc(words * sizeof(u32)));
  CK(dh.alloc(n * 32));
  if (payload) CK(dp.alloc(n * 32));
  CK(hipMemcpyAsync(dv.p, values, words * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  CK(hipMemcpyAsync(dh.p, hashes, n * 32, hipMemcpyHostToDevice, c->stream));
  if (payload) CK(hipMemcpyAsync(dp.p, payload, n * 32, hipMemcpyHostToDevice, c->stream));
  rc = row_update_launch(c, variant, t, id, (const u32*)dv.p, value_stride, dp.p, closure, dh.p);
  if (rc) return rc;
  CK(hipMemcpyAsync(back.data(), dh.p, n * 32, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  for (uint32_t i : closure.nodes) std::copy(back.begin() + (size_t)i * 4, back.begin() + (size_t)i * 4 + 4, hashes + (size_t)i * 4);
  return 0;
}

}  // extern "C"
