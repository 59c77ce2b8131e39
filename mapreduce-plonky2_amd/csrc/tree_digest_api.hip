// C ABI of the accumulated Ecgfp5 digests of a table's trees (include/mp2g.h), over the kernels of tree_digest.hip and the decode
// kernel of ecgfp5.hip. Every argument is judged on the host before anything is launched.
#include "index_api.h"
#include "ecgfp5.h"
#include "tree_digest.h"

using namespace mp2g;

static const size_t PT_BYTES = 20 * sizeof(u64);

static bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}
// what both tree passes refuse; *n is the shape's size
static int tree_args(const mp2g_tree_shape* t, const uint64_t* d_own, const uint64_t* d_acc, size_t* n) {
  NEED(t, "shape");
  *n = t->s.size();
  if (!*n) return 0;
  NEED(d_own && d_acc, "own / acc");
  NEED(!overlap(d_own, d_acc, *n * PT_BYTES), "own and acc overlap");
  return 0;
}
static int emit_to_host(mp2g_ctx* c, const u64* d_frac, const u32* d_idx, uint32_t count, uint64_t* out_w, uint64_t* out_wei) {
  DevBuf dw, dwei;
  if (out_w) CK(dw.alloc((size_t)count * 5 * sizeof(u64)));
  if (out_wei) CK(dwei.alloc((size_t)count * 11 * sizeof(u64)));
  CK(emit_indexed(c->stream, d_frac, d_idx, count, out_w ? dw.p : nullptr, out_wei ? dwei.p : nullptr));
  if (out_w) CK(hipMemcpyAsync(out_w, dw.p, (size_t)count * 5 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (out_wei) CK(hipMemcpyAsync(out_wei, dwei.p, (size_t)count * 11 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" {

int mp2g_curve_decode_dev(mp2g_ctx* c, const uint64_t* pts_w, uint32_t count, uint64_t* d_frac) {
  if (!count) return 0;
  NEED(c && pts_w && d_frac, "ctx / pts / frac");
  // a limb >= p never reaches the kernel: the field routines behind pt_decode take canonical values only (ec_api.hip, decode_host)
  for (size_t i = 0; i < (size_t)count * 5; i++)
    if (pts_w[i] >= GL_P)
      return fail("point encoding is not canonical: limb %u of point %zu is 0x%016llx >= p", (unsigned)(i % 5), i / 5,
                  (unsigned long long)pts_w[i]);
  DevBuf dw, dbad;
  CK(dw.alloc((size_t)count * 5 * sizeof(u64)));
  CK(dbad.alloc(8));
  CK(hipMemsetAsync(dbad.p, 0, 8, c->stream));
  CK(hipMemcpyAsync(dw.p, pts_w, (size_t)count * 5 * sizeof(u64), hipMemcpyHostToDevice, c->stream));
  CK(ec_decode(c->stream, dw.p, count, (u64*)d_frac, (u32*)dbad.p));
  u32 bad = 0;
  CK(hipMemcpyAsync(&bad, dbad.p, 4, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  if (bad) return fail("invalid point encoding (Point::decode failed)");
  return 0;
}

int mp2g_curve_emit_dev(mp2g_ctx* c, const uint64_t* d_frac, const uint32_t* idx, uint32_t count, uint64_t* out_w, uint64_t* out_wei) {
  if (!count || (!out_w && !out_wei)) return 0;
  NEED(c && d_frac, "ctx / frac");
  const u32* d_idx = nullptr;
  if (idx) {
    int rc = stage_lists(c, idx, count, nullptr, 0, &d_idx);
    if (rc) return rc;
  }
  return emit_to_host(c, (const u64*)d_frac, d_idx, count, out_w, out_wei);
}

int mp2g_tree_digests_dev(mp2g_ctx* c, const mp2g_tree_shape* t, const uint64_t* d_own, uint64_t* d_acc) {
  size_t n;
  int rc = tree_args(t, d_own, d_acc, &n);
  if (rc || !n) return rc;
  NEED(c, "ctx");
  const u32* d;
  rc = shape_on_device(t, c, &d);
  if (rc) return rc;
  const int32_t *left = (const int32_t*)d, *right = (const int32_t*)(d + n);
  const u32* order = d + 4 * n;
  for (uint32_t h = 0; h < t->s.levels(); h++) {
    const uint32_t lo = t->s.level_off[h], count = t->s.level_off[h + 1] - lo;
    CK(digest_level(c->stream, order + lo, count, left, right, (const u64*)d_own, (u64*)d_acc));
  }
  return 0;
}

int mp2g_tree_digests(mp2g_ctx* c, const mp2g_tree_shape* t, const uint64_t* own_w, uint64_t* out_w, uint64_t* out_wei) {
  NEED(t, "shape");
  const size_t n = t->s.size();
  if (!n) return 0;
  NEED(c && own_w, "ctx / own");
  DevBuf own, acc;
  CK(own.alloc(n * PT_BYTES));
  CK(acc.alloc(n * PT_BYTES));
  int rc = mp2g_curve_decode_dev(c, own_w, (uint32_t)n, own.p);
  if (rc) return rc;
  rc = mp2g_tree_digests_dev(c, t, own.p, acc.p);
  if (rc) return rc;
  if (!out_w && !out_wei) return 0;
  return emit_to_host(c, acc.p, nullptr, (uint32_t)n, out_w, out_wei);
}

uint32_t mp2g_tree_digests_update_fused_width(void) { return MP2G_TREE_DIGEST_FUSED_WIDTH; }

int mp2g_tree_digests_update_dev(mp2g_ctx* c, const mp2g_tree_shape* t, const uint64_t* d_own, const uint32_t* touched, uint32_t n_touched,
                                 uint64_t* d_acc) {
  NEED(t, "shape");
  NEED(touched || !n_touched, "touched list missing");
  TreeTouched closure;
  int rc = guarded([&] { return tree_shape_touched(t->s, touched, n_touched, closure) ? fail("invalid argument: %s", closure.err) : 0; });
  if (rc) return rc;
  if (closure.nodes.empty()) return 0;
  size_t n;
  rc = tree_args(t, d_own, d_acc, &n);
  if (rc) return rc;
  NEED(c, "ctx");
  const u32* d;
  rc = shape_on_device(t, c, &d);
  if (rc) return rc;
  const int32_t *left = (const int32_t*)d, *right = (const int32_t*)(d + n);
  const u32* d_order;
  rc = stage_lists(c, closure.nodes.data(), closure.nodes.size(), closure.level_off.data(), closure.level_off.size(), &d_order);
  if (rc) return rc;
  if (closure.widest <= MP2G_TREE_DIGEST_FUSED_WIDTH && closure.levels() <= MP2G_ROW_UPDATE_FUSED_LEVELS) {
    CK(digest_update_fused(c->stream, d_order, d_order + closure.nodes.size(), closure.levels(), left, right, (const u64*)d_own, (u64*)d_acc));
    return 0;
  }
  for (uint32_t l = 0; l < closure.levels(); l++) {
    const uint32_t lo = closure.level_off[l], count = closure.level_off[l + 1] - lo;
    CK(digest_level(c->stream, d_order + lo, count, left, right, (const u64*)d_own, (u64*)d_acc));
  }
  return 0;
}

// row_idx NULL with n_idx == 0 = every row; a list with n_idx == 0 = no row
int mp2g_cells_tree_digests_dev(mp2g_ctx* c, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* d_values, uint32_t rows,
                                const uint32_t* row_idx, uint32_t n_idx, uint64_t* d_nodes) {
  int rc = cells_rows_args(variant, col_ids, n_cols, rows, row_idx, n_idx);
  if (rc) return rc;
  const uint32_t n = row_idx ? n_idx : rows, cells = n_cols - 1;
  if (!n || !cells) return 0;
  NEED(c && d_values && d_nodes, "ctx / values / nodes");
  const u32* d_idx = nullptr;
  if (row_idx) {
    rc = stage_lists(c, row_idx, n_idx, nullptr, 0, &d_idx);
    if (rc) return rc;
  }
  return cells_levels(col_ids, cells, [&](const CellsLevel& lv, uint32_t count, int) {
    CK(cells_digest_level(c->stream, variant, lv, count, d_values, n_cols, d_idx, n, (u64*)d_nodes));
    return 0;
  });
}

int mp2g_row_digests_dev(mp2g_ctx* c, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* d_values, const uint32_t* d_unique,
                         uint32_t unique_stride, uint32_t n_unique, uint32_t rows, const uint64_t* d_cells_nodes, const uint32_t* row_idx,
                         uint32_t n_idx, uint64_t* d_own) {
  int rc = cells_rows_args(variant, col_ids, n_cols, rows, row_idx, n_idx);
  if (rc) return rc;
  NEED(d_unique || !n_unique, "unique columns missing");
  if ((uint64_t)unique_stride < 8ull * n_unique)
    return fail("invalid argument: unique_stride %u is below the %llu words of %u unique columns", unique_stride, 8ull * n_unique, n_unique);
  const uint32_t n = row_idx ? n_idx : rows, cells = n_cols - 1;
  if (!n) return 0;
  NEED(c && d_values && d_own, "ctx / values / own");
  if (!cells) d_cells_nodes = nullptr;  // no cells: the row's sum is D(id_0 || value_0) alone
  // the identifiers (two words each) and the row list go up as one staged list; the identifiers first, so they stay 8-byte aligned
  const u32* d_lists;
  rc = stage_lists(c, (const u32*)col_ids, 2 * (size_t)n_cols, row_idx, row_idx ? n_idx : 0, &d_lists);
  if (rc) return rc;
  const u32* d_idx = row_idx ? d_lists + 2 * (size_t)n_cols : nullptr;
  CK(row_own(c->stream, variant, (const u64*)d_lists, n_cols, d_values, d_unique, unique_stride, n_unique, (const u64*)d_cells_nodes,
             (int)sbbst_root(cells) - 1, d_idx, n, (u64*)d_own));
  return 0;
}

}  // extern "C"
