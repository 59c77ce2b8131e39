// Tables that live in contract storage, for gfx950: the values digest of every MPT storage leaf and the cut of its columns out of
// the leaf's 32-byte EVM word.
//
// Replaces, on the value (non-circuit) side:
//   mp2-v1/src/values_extraction/gadgets/column_gadget.rs:326-368   extract_value
//   mp2-v1/src/values_extraction/gadgets/column_gadget.rs:301-323   ColumnGadgetData::digest
//   mp2-v1/src/values_extraction/mod.rs:298-314                     row_unique_data_for_{single,mapping,mapping_of_mappings}_leaf
//   mp2-v1/src/values_extraction/mod.rs:327-341, :374-406, :450-496 compute_leaf_{single,mapping,mapping_of_mappings}_values_digest
// (the three metadata digests, mod.rs:316-325, :343-372, :408-445, are per table and are composed on the host side from
// mp2g_hash_no_pad_batch, mp2g_map_to_curve_batch and mp2g_curve_sum: extraction.py).
//
// ALU-bound like row_digest_kernel (ecgfp5.hip), whose shape this has: one lane per leaf, per extracted column one sponge and one
// simple_swu, then two permutations for the row id and one 128-bit scalar multiplication. The columns' identifiers and layouts are
// the same for every leaf and arrive by value in the kernel's arguments (LeafColumns), so the column loop, both shift amounts and
// the evm_word branch are uniform over the grid and are read through the scalar cache.
//
// The cut: extract_value's byte loop is ((V << shl) mod 2^256) >> shr on the word as a 256-bit big-endian integer V, then the low
// byte shifted right by `tail` (extraction.h). The word is eight registers; a shift by a uniform amount is a barrel shifter over
// whole words (every index static after unrolling, the conditions scalar) and a funnel shift for the bits left over. No private
// array is indexed by a runtime value, so nothing of it goes to scratch: what scratch the digest kernel has comes from the
// out-of-line EC bodies, as row_digest_kernel's does.
#include "extraction.h"
#include "poseidon.cuh"
#include "gl5.cuh"
#include "ec_curve.cuh"

namespace mp2g {

// 32 bytes at p (16-byte aligned) as the eight big-endian u32 words of pack(Endianness::Big): w[0] is the most significant
GLD void load_be_words(const uint8_t* p, u32 w[8]) {
  const uint4 a = ((const uint4*)p)[0], b = ((const uint4*)p)[1];
  w[0] = __builtin_bswap32(a.x); w[1] = __builtin_bswap32(a.y); w[2] = __builtin_bswap32(a.z); w[3] = __builtin_bswap32(a.w);
  w[4] = __builtin_bswap32(b.x); w[5] = __builtin_bswap32(b.y); w[6] = __builtin_bswap32(b.z); w[7] = __builtin_bswap32(b.w);
}
// one stage of a barrel shifter over whole words: by B words when the (uniform) count n has that bit
template <int B>
GLD void words_left(u32 w[8], u32 n) {
  if (n & B) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = i + B < 8 ? w[i + B] : 0;
  }
}
template <int B>
GLD void words_right(u32 w[8], u32 n) {
  if (n & B) {
#pragma unroll
    for (int i = 7; i >= 0; i--) w[i] = i - B >= 0 ? w[i - B] : 0;  // descending: a source is read before it is written
  }
}
// w = ((w << shl) mod 2^256) >> shr, then the low byte >> tail; cut as leaf_cut() packs it, the same for every lane
GLD void cut_words(u32 w[8], u32 cut) {
  const u32 shl = cut & 0xFFFF, shr = (cut >> 16) & 0xFF, tail = cut >> 24;
  // left by shl >> 5 whole words (0..8): one conditional stage per bit of the count
  words_left<1>(w, shl >> 5); words_left<2>(w, shl >> 5); words_left<4>(w, shl >> 5); words_left<8>(w, shl >> 5);
  const u32 lb = shl & 31;
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = (u32)(((((u64)w[i] << 32) | (i < 7 ? w[i + 1] : 0)) << lb) >> 32);
  // right by shr >> 5 whole words (0..7)
  words_right<1>(w, shr >> 5); words_right<2>(w, shr >> 5); words_right<4>(w, shr >> 5);
  const u32 rb = shr & 31;
#pragma unroll
  for (int i = 7; i >= 0; i--) w[i] = (u32)((((u64)(i > 0 ? w[i - 1] : 0) << 32) | w[i]) >> rb);
  w[7] = (w[7] & 0xFFFFFF00u) | ((w[7] & 0xFFu) >> tail);
}

// blockIdx.y = column: the cut is uniform over the block
__global__ void __launch_bounds__(128) extract_values_kernel(const LeafCut cuts, u32 n_cols, const uint8_t* __restrict__ words, u32 count,
                                                             u32* __restrict__ out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const u32 c = blockIdx.y;
  u32 w[8];
  load_be_words(words + 32 * i, w);
  cut_words(w, cuts.cut[c]);
  u32* o = out + (i * n_cols + c) * 8;
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = w[j];
}

// one lane per leaf
template <int V>
__global__ void __launch_bounds__(128) leaf_values_digest_kernel(const LeafColumns cols, const uint8_t* __restrict__ words,
                                                                 const uint8_t* __restrict__ keys, u32 count, u64* __restrict__ frac_out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  // ColumnGadgetData::digest: sum over the extracted columns of D(identifier || pack(extract_value))   (column_gadget.rs:301-323)
  pt vd = pt_neutral();
  for (u32 c = 0; c < cols.n_extracted; c++) {
    u32 w[8];
    load_be_words(words + 32 * i, w);  // read again per column (a cache hit): no word is kept live across the EC calls
    cut_words(w, cols.cuts.cut[c]);
    u64 in[9];
    in[0] = cols.id[c];
#pragma unroll
    for (int j = 0; j < 8; j++) in[1 + j] = w[j];
    vd = pt_add(vd, map_to_curve<V>(in, 9));
  }
  // evm_word == 0: + D(key_id || pack(left_pad32(key))) per key   (mod.rs:389-400, :474-488)
  const uint8_t* key = keys + 32 * i * cols.n_keys;
  if (cols.add_keys)
    for (u32 j = 0; j < cols.n_keys; j++) {
      u32 w[8];
      load_be_words(key + 32 * j, w);
      u64 in[9];
      in[0] = cols.key_id[j];
#pragma unroll
      for (int k = 0; k < 8; k++) in[1 + k] = w[k];
      vd = pt_add(vd, map_to_curve<V>(in, 9));
    }
  // row_unique_data = H(pack(key_0) || pack(key_1)); no key: the hash of the empty input, all zero   (mod.rs:298-314, :499-510)
  u64 s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  for (u32 j = 0; j < cols.n_keys; j++) {
    u32 w[8];
    load_be_words(key + 32 * j, w);
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = w[k];
    perm<V>(s);
  }
  // compute_row_id: H(row_unique_data(4) || num_actual_columns)[0..2] -> 128-bit scalar   (mod.rs:512-523)
  u64 h[4] = {s[0], s[1], s[2], s[3]};
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  s[0] = h[0]; s[1] = h[1]; s[2] = h[2]; s[3] = h[3]; s[4] = cols.n_row_cols;
  perm<V>(s);
  u32 k128[4] = {(u32)s[0], (u32)(s[0] >> 32), (u32)s[1], (u32)(s[1] >> 32)};
  pt_store(frac_out + 20 * i, pt_mul128(vd, k128));
}

// ---- launchers --------------------------------------------------------------------------------
hipError_t leaf_extract(hipStream_t st, const LeafCut& cuts, u32 n_cols, const uint8_t* words, u32 count, u32* out) {
  if (!count || !n_cols) return hipSuccess;
  if (n_cols > MP2G_LEAF_MAX_COLS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(extract_values_kernel, dim3((count + 127) / 128, n_cols), dim3(128), 0, st, cuts, n_cols, words, count, out);
  return hipGetLastError();
}
hipError_t leaf_values_digest(hipStream_t st, int variant, const LeafColumns& cols, const uint8_t* words, const uint8_t* keys, u32 count,
                              u64* frac_out) {
  if (!count) return hipSuccess;
  if (cols.n_extracted > MP2G_LEAF_MAX_COLS || cols.n_keys > MP2G_LEAF_MAX_KEYS) return hipErrorInvalidValue;
  const dim3 grid((count + 127) / 128);
  if (variant == MP2G_POSEIDON2) hipLaunchKernelGGL((leaf_values_digest_kernel<MP2G_POSEIDON2>), grid, dim3(128), 0, st, cols, words, keys, count, frac_out);
  else if (variant == MP2G_POSEIDON) hipLaunchKernelGGL((leaf_values_digest_kernel<MP2G_POSEIDON>), grid, dim3(128), 0, st, cols, words, keys, count, frac_out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
}  // namespace mp2g
