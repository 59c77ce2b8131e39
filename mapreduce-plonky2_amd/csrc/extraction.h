// Launchers of the storage-leaf kernels (extraction.hip): the cut of bit fields out of 32-byte EVM words and the values digest of
// every MPT storage leaf of a table. What is the same for every leaf travels by value in the kernel's arguments, as CellsLevel does.
#pragma once
#include "gl.cuh"

namespace mp2g {
#define MP2G_LEAF_MAX_COLS 32
#define MP2G_LEAF_MAX_KEYS 2
// extract_value (column_gadget.rs:326-368) of column c as two shifts of the word read as a 256-bit big-endian integer V:
// ((V << shl) mod 2^256) >> shr, then the low byte shifted right by tail. cut[c] = shl | shr << 16 | tail << 24 with
// shl = 8 * byte_offset + bit_offset (0..256), shr = 256 - 8 * ceil(length / 8) (0..248), tail = (8 - length % 8) % 8.
struct LeafCut {
  u32 cut[MP2G_LEAF_MAX_COLS];
};
inline u32 leaf_cut(u32 byte_offset, u32 bit_offset, u32 length) {
  return (8 * byte_offset + bit_offset) | (256 - 8 * ((length + 7) / 8)) << 16 | ((8 - length % 8) % 8) << 24;
}
struct LeafColumns {
  LeafCut cuts;
  u64 id[MP2G_LEAF_MAX_COLS];      // identifiers of the extracted columns
  u64 key_id[MP2G_LEAF_MAX_KEYS];  // identifiers of the key columns, outer first
  u64 n_row_cols;  // n_table_columns + n_keys: what compute_row_id hashes
  u32 n_extracted, n_keys;
  u32 add_keys;  // evm_word == 0: the key columns belong to this leaf's digest
};
// out[leaf][col][0..8) = the cut of words[leaf] by cuts.cut[col], 8 big-endian u32 words. words 16-byte aligned.
hipError_t leaf_extract(hipStream_t st, const LeafCut& cuts, u32 n_cols, const uint8_t* words, u32 count, u32* out);
// frac_out[leaf] = row_id * (sum_c D(id_c || cut_c(words[leaf])) [+ sum_j D(key_id_j || keys[leaf][j])]), mod.rs:327-341, :374-406,
// :450-496. words [count][32] and keys [count][n_keys][32] 16-byte aligned; frac_out [count][20].
hipError_t leaf_values_digest(hipStream_t st, int variant, const LeafColumns& cols, const uint8_t* words, const uint8_t* keys, u32 count,
                              u64* frac_out);
}  // namespace mp2g
