// What the C ABI files over a table's trees share (index_api.hip: shapes and node hashes; tree_digest_api.hip: accumulated digests):
// the shape handle with its device copy, the exception guard, the staging of host index lists, the level schedule of a cells tree and
// the argument checks of the cells-tree calls.
#pragma once
#include "ctx.h"
#include "index_hash.h"
#include "tree_shape.h"
#include <cstring>
#include <exception>
#include <new>

struct mp2g_tree_shape {
  mp2g::TreeShape s;
  // the shape's arrays on the device (left, right, min_idx, max_idx, order: 5 n words of 32 bits), uploaded by the first hashing
  // call that uses the shape, on that context's stream, and kept until mp2g_tree_shape_free
  mutable mp2g::DevBuf dev;
  mutable const mp2g_ctx* bound = nullptr;
};

namespace mp2g {
// No exception crosses the C ABI: the entry points that build vectors (a shape of up to 2^31 - 1 nodes is gigabytes of them) run
// inside guarded(), which turns bad_alloc and anything else into the library's error code + mp2g_last_error().
template <class F> inline int guarded(F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail("out of memory");
  } catch (const std::exception& e) {
    return fail("internal error: %s", e.what());
  } catch (...) {
    return fail("internal error");
  }
}

// the device copy, made once
inline int shape_on_device(const mp2g_tree_shape* t, mp2g_ctx* c, const u32** d) {
  const size_t n = t->s.size();
  if (!t->bound) {
    CK(hipSetDevice(c->device));
    CK(t->dev.alloc(5 * n * sizeof(u32)));
    u32* p = (u32*)t->dev.p;
    const void* src[5] = {t->s.left.data(), t->s.right.data(), t->s.min_idx.data(), t->s.max_idx.data(), t->s.order.data()};
    for (int k = 0; k < 5; k++) {  // the host arrays live as long as the handle, and freeing the handle waits for the device
      hipError_t e = hipMemcpyAsync(p + k * n, src[k], n * sizeof(u32), hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) { t->dev.release(); return fail("tree shape upload: %s", hipGetErrorString(e)); }
    }
    t->bound = c;
  }
  NEED(t->bound == c, "the tree shape was first used with another context (its device arrays belong to that context's stream)");
  *d = (const u32*)t->dev.p;
  return 0;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// a[0..na) followed by b[0..nb), host words, to the context's list buffer on its stream (ctx.h: one device copy, a ring of pinned
// slots under it); *d is the device address of a[0]
inline int stage_lists(mp2g_ctx* c, const u32* a, size_t na, const u32* b, size_t nb, const u32** d) {
  const size_t need = (na + nb) * sizeof(u32);
  CK(hipSetDevice(c->device));
  mp2g_ctx::IndexStage& slot = c->index_stage[c->index_stage_next++ % mp2g_ctx::INDEX_STAGE_SLOTS];
  if (slot.pending) {  // the upload that last read this slot
    CK(hipEventSynchronize(slot.done));
    slot.pending = false;
  }
  if (!slot.done) CK(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
  if (slot.bytes < need) {
    if (slot.host) (void)hipHostFree(slot.host);
    slot.host = nullptr;
    slot.bytes = 0;
    const size_t cap = need < 4096 ? 4096 : need + need / 2;
    CK(hipHostMalloc((void**)&slot.host, cap, hipHostMallocDefault));
    slot.bytes = cap;
  }
  if (c->index_lists.bytes < need) {
    CK(hipStreamSynchronize(c->stream));  // a kernel queued earlier may still read the old buffer
    CK(c->index_lists.alloc(need < 4096 ? 4096 : need + need / 2));
  }
  if (na) memcpy(slot.host, a, na * sizeof(u32));
  if (nb) memcpy(slot.host + na, b, nb * sizeof(u32));
  CK(hipMemcpyAsync(c->index_lists.p, slot.host, need, hipMemcpyHostToDevice, c->stream));
  CK(hipEventRecord(slot.done, c->stream));
  slot.pending = true;
  *d = (const u32*)c->index_lists.p;
  return 0;
}

// the level schedule of the sbbst over `cells` positions: launch(lv, count, root) for the cells of each height, lowest first
template <class F> inline int cells_levels(const uint64_t* col_ids, uint32_t cells, F&& launch) {
  TreeShape s;
  int rc = guarded([&] {  // at most 255 nodes
    std::vector<int32_t> l(cells), r(cells);
    sbbst_fill(cells, l.data(), r.data());
    const char* err = tree_shape_build(l.data(), r.data(), cells, s);
    return err ? fail("cells tree: %s", err) : 0;
  });
  if (rc) return rc;
  const int root = (int)sbbst_root(cells) - 1;
  for (uint32_t h = 0; h < s.levels(); h++) {
    const uint32_t lo = s.level_off[h], count = s.level_off[h + 1] - lo;
    NEED(count <= MP2G_CELLS_PER_LAUNCH, "cells of one height");  // 255 cells: at most 128
    CellsLevel lv = {};
    for (uint32_t j = 0; j < count; j++) {
      const uint32_t node = s.order[lo + j];
      lv.id[j] = col_ids[node + 1];
      lv.node[j] = (int16_t)node;
      lv.left[j] = (int16_t)s.left[node];
      lv.right[j] = (int16_t)s.right[node];
    }
    rc = launch(lv, count, root);
    if (rc) return rc;
  }
  return 0;
}

// what every cells-tree call refuses before it launches anything
inline int cells_args(int variant, const uint64_t* col_ids, uint32_t n_cols, uint32_t rows) {
  NEED(variant == 0 || variant == 1, "variant");
  NEED(n_cols >= 1 && n_cols <= 256, "1 <= n_cols <= 256");
  NEED(col_ids, "col_ids");
  for (uint32_t k = 0; k < n_cols; k++) NEED(col_ids[k] < GL_P, "column identifier not canonical (>= p)");
  NEED(rows <= 0x80000000u, "rows <= 2^31");  // one lane per row along grid.x
  return 0;
}
inline int cells_rows_args(int variant, const uint64_t* col_ids, uint32_t n_cols, uint32_t rows, const uint32_t* row_idx, uint32_t n_idx) {
  int rc = cells_args(variant, col_ids, n_cols, rows);
  if (rc) return rc;
  NEED(row_idx || !n_idx, "row_idx list missing");
  for (uint32_t j = 0; j < n_idx; j++)
    if (row_idx[j] >= rows) return fail("invalid argument: row index %u is outside the table's %u rows", row_idx[j], rows);
  return 0;
}
}  // namespace mp2g
