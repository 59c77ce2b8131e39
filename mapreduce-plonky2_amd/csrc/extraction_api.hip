// C ABI of the storage-leaf digests and the cut of EVM words (include/mp2g.h), over the kernels of extraction.hip and the sum /
// emit kernels of ecgfp5.hip. Every argument is judged on the host before anything is uploaded or launched.
#include "ctx.h"
#include "ecgfp5.h"
#include "extraction.h"

using namespace mp2g;

static const size_t PT_BYTES = 20 * sizeof(u64);

// layout[n][3] = (byte offset, bit offset, length in bits) of every column, judged as extract_value's own assertions and array
// bounds judge it (column_gadget.rs:326-368); cuts receives the shifts
static int layout_args(const uint32_t* layout, uint32_t n, const char* n_name, LeafCut* cuts) {
  if (n > MP2G_LEAF_MAX_COLS) return fail("invalid argument: %s %u is above the %d columns of one EVM word", n_name, n, MP2G_LEAF_MAX_COLS);
  NEED(layout || !n, "layout");
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t byte = layout[3 * c], bit = layout[3 * c + 1], len = layout[3 * c + 2];
    if (len == 0 || len > 256) return fail("invalid argument: layout: length %u of column %u is outside 1..256", len, c);
    if (bit > 8) return fail("invalid argument: layout: bit offset %u of column %u is above 8", bit, c);
    if ((uint64_t)byte + (len + 7) / 8 > 32)
      return fail("invalid argument: layout: byte_offset %u + %u bytes of column %u end past the 32-byte word", byte, (len + 7) / 8, c);
    cuts->cut[c] = leaf_cut(byte, bit, len);
  }
  return 0;
}
static int aligned16(const void* p, const char* name) {
  if ((uintptr_t)p & 15) return fail("invalid argument: %s is not 16-byte aligned", name);
  return 0;
}
// everything mp2g_leaf_values_digests[_dev] refuses but its pointers to the leaves
static int leaf_args(int variant, const uint64_t* col_ids, const uint32_t* layout, uint32_t n_extracted, uint32_t n_table_columns,
                     const uint64_t* key_ids, uint32_t n_keys, uint32_t evm_word, LeafColumns* cols) {
  NEED(variant == 0 || variant == 1, "variant");
  int rc = layout_args(layout, n_extracted, "n_extracted", &cols->cuts);
  if (rc) return rc;
  if (n_keys > MP2G_LEAF_MAX_KEYS) return fail("invalid argument: n_keys %u is above %d (outer and inner mapping key)", n_keys, MP2G_LEAF_MAX_KEYS);
  if (n_table_columns < n_extracted)
    return fail("invalid argument: n_table_columns %u is below n_extracted %u", n_table_columns, n_extracted);
  NEED(col_ids || !n_extracted, "col_ids");
  NEED(key_ids || !n_keys, "key_ids");
  for (uint32_t c = 0; c < n_extracted; c++) {
    if (col_ids[c] >= GL_P) return fail("invalid argument: col_ids: column identifier not canonical: entry %u is 0x%016llx >= p", c, (unsigned long long)col_ids[c]);
    cols->id[c] = col_ids[c];
  }
  for (uint32_t j = 0; j < n_keys; j++) {
    if (key_ids[j] >= GL_P) return fail("invalid argument: key_ids: key column identifier not canonical: entry %u is 0x%016llx >= p", j, (unsigned long long)key_ids[j]);
    cols->key_id[j] = key_ids[j];
  }
  cols->n_extracted = n_extracted;
  cols->n_keys = n_keys;
  cols->add_keys = evm_word == 0;
  cols->n_row_cols = (u64)n_table_columns + n_keys;  // compute_row_id's num_actual_columns (mod.rs:333, :384, :461)
  return 0;
}
static void neutral_out(uint64_t* w, uint64_t* wei) {
  if (w) for (int k = 0; k < 5; k++) w[k] = 0;
  if (wei) { for (int k = 0; k < 10; k++) wei[k] = 0; wei[10] = 1; }
}
// the leaves' digests into frac (the caller's or a buffer of the call's), then what the caller asked for
static int leaf_run(mp2g_ctx* c, int variant, const LeafColumns& cols, const uint8_t* d_words, const uint8_t* d_keys, uint32_t count,
                    uint64_t* d_frac_out, uint64_t* out_w, uint64_t* out_wei, uint64_t* sum_w, uint64_t* sum_wei) {
  DevBuf frac, scratch, dw, dwei, dsw, dswei;
  u64* f = (u64*)d_frac_out;
  if (!f) { CK(frac.alloc((size_t)count * PT_BYTES)); f = frac.p; }
  CK(leaf_values_digest(c->stream, variant, cols, d_words, d_keys, count, f));
  const bool each = out_w || out_wei, sum = sum_w || sum_wei;
  if (each) {
    if (out_w) CK(dw.alloc((size_t)count * 5 * sizeof(u64)));
    if (out_wei) CK(dwei.alloc((size_t)count * 11 * sizeof(u64)));
    CK(ec_emit(c->stream, f, count, out_w ? dw.p : nullptr, out_wei ? dwei.p : nullptr));
    if (out_w) CK(hipMemcpyAsync(out_w, dw.p, (size_t)count * 5 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (out_wei) CK(hipMemcpyAsync(out_wei, dwei.p, (size_t)count * 11 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  }
  if (sum) {
    CK(scratch.alloc(20 * 1025 * sizeof(u64)));
    CK(dsw.alloc(5 * sizeof(u64)));
    CK(dswei.alloc(11 * sizeof(u64)));
    CK(ec_sum(c->stream, f, count, scratch.p));
    CK(ec_emit(c->stream, scratch.p, 1, sum_w ? dsw.p : nullptr, sum_wei ? dswei.p : nullptr));
    if (sum_w) CK(hipMemcpyAsync(sum_w, dsw.p, 5 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (sum_wei) CK(hipMemcpyAsync(sum_wei, dswei.p, 11 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  }
  if (each || sum || !d_frac_out) CK(hipStreamSynchronize(c->stream));  // host outputs, or buffers of this call that are freed on return
  return 0;
}

extern "C" {

int mp2g_extract_values_dev(mp2g_ctx* c, const uint8_t* d_words, const uint32_t* layout, uint32_t n_cols, uint32_t count, uint32_t* d_out) {
  LeafCut cuts = {};
  int rc = layout_args(layout, n_cols, "n_cols", &cuts);
  if (rc) return rc;
  if (!count || !n_cols) return 0;
  NEED(c, "ctx");
  NEED(d_words, "words");
  NEED(d_out, "out");
  rc = aligned16(d_words, "words");
  if (rc) return rc;
  CK(leaf_extract(c->stream, cuts, n_cols, d_words, count, d_out));
  return 0;
}

int mp2g_extract_values(mp2g_ctx* c, const uint8_t* words, const uint32_t* layout, uint32_t n_cols, uint32_t count, uint32_t* out) {
  LeafCut cuts = {};
  int rc = layout_args(layout, n_cols, "n_cols", &cuts);
  if (rc) return rc;
  if (!count || !n_cols) return 0;
  NEED(c, "ctx");
  NEED(words, "words");
  NEED(out, "out");
  DevBuf dwords, dout;
  CK(dwords.alloc((size_t)count * 32));
  CK(dout.alloc((size_t)count * n_cols * 32));
  CK(hipMemcpyAsync(dwords.p, words, (size_t)count * 32, hipMemcpyHostToDevice, c->stream));
  CK(leaf_extract(c->stream, cuts, n_cols, (const uint8_t*)dwords.p, count, (u32*)dout.p));
  CK(hipMemcpyAsync(out, dout.p, (size_t)count * n_cols * 32, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

int mp2g_leaf_values_digests_dev(mp2g_ctx* c, int variant, const uint64_t* col_ids, const uint32_t* layout, uint32_t n_extracted,
                                 uint32_t n_table_columns, const uint8_t* d_words, const uint8_t* d_keys, const uint64_t* key_ids,
                                 uint32_t n_keys, uint32_t evm_word, uint32_t count, uint64_t* d_frac_out, uint64_t* out_w,
                                 uint64_t* out_wei, uint64_t* sum_w, uint64_t* sum_wei) {
  LeafColumns cols = {};
  int rc = leaf_args(variant, col_ids, layout, n_extracted, n_table_columns, key_ids, n_keys, evm_word, &cols);
  if (rc) return rc;
  if (!count) {  // the empty sum
    neutral_out(sum_w, sum_wei);
    return 0;
  }
  NEED(c, "ctx");
  NEED(d_words || !n_extracted, "words");
  NEED(d_keys || !n_keys, "keys");
  if (n_extracted && (rc = aligned16(d_words, "words"))) return rc;
  if (n_keys && (rc = aligned16(d_keys, "keys"))) return rc;
  return leaf_run(c, variant, cols, d_words, d_keys, count, d_frac_out, out_w, out_wei, sum_w, sum_wei);
}

int mp2g_leaf_values_digests(mp2g_ctx* c, int variant, const uint64_t* col_ids, const uint32_t* layout, uint32_t n_extracted,
                             uint32_t n_table_columns, const uint8_t* words, const uint8_t* keys, const uint64_t* key_ids, uint32_t n_keys,
                             uint32_t evm_word, uint32_t count, uint64_t* out_w, uint64_t* out_wei, uint64_t* sum_w, uint64_t* sum_wei) {
  LeafColumns cols = {};
  int rc = leaf_args(variant, col_ids, layout, n_extracted, n_table_columns, key_ids, n_keys, evm_word, &cols);
  if (rc) return rc;
  if (!count) {
    neutral_out(sum_w, sum_wei);
    return 0;
  }
  NEED(c, "ctx");
  NEED(words || !n_extracted, "words");
  NEED(keys || !n_keys, "keys");
  DevBuf dwords, dkeys;
  if (n_extracted) {
    CK(dwords.alloc((size_t)count * 32));
    CK(hipMemcpyAsync(dwords.p, words, (size_t)count * 32, hipMemcpyHostToDevice, c->stream));
  }
  if (n_keys) {
    CK(dkeys.alloc((size_t)count * n_keys * 32));
    CK(hipMemcpyAsync(dkeys.p, keys, (size_t)count * n_keys * 32, hipMemcpyHostToDevice, c->stream));
  }
  return leaf_run(c, variant, cols, (const uint8_t*)dwords.p, (const uint8_t*)dkeys.p, count, nullptr, out_w, out_wei, sum_w, sum_wei);
}

}  // extern "C"
