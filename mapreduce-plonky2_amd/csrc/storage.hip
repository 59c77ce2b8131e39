// Keccak-256 on the device, for gfx950: what lies between an eth_getProof answer and the 32-byte EVM word that the storage-leaf
// digests (extraction.hip) start from.
//
// Replaces, on the value (non-circuit) side:
//   mp2-common/src/eth.rs:233-266                          StorageSlot::location
//   mp2-common/src/eth.rs:267-276                          StorageSlot::mpt_key / mpt_nibbles (the K public input)
//   keccak256(node).pack(Endianness::Little)               values_extraction/leaf_single.rs:279, leaf_mapping.rs:340,
//                                                          leaf_mapping_of_mappings.rs:390, branch.rs:318,397, extension.rs:183,217
//   mp2-common/src/mpt_sequential/leaf_or_extension.rs:49-87, utils.rs:41-67   the leaf node's RLP opened, left_pad_leaf_value
//
// Three kernels, one lane per message / leaf, over the one permutation of keccak.cuh; all ALU-bound (a permutation is ~10^4 VALU
// instructions against at most a few hundred bytes read). The slot-keys kernel builds its 64- and 32-byte messages in registers and
// runs the leaf's three or four permutations back to back: nothing but its outputs touches memory. The leaf kernel hashes the node
// from global memory and then opens it by byte reads from global memory at run-time offsets (cache hits: the sponge has just read
// the row), never from a register array, so the decode stays out of scratch; every offset is below min(len, stride) before it is
// used, so a hostile length byte cannot read outside the node's row.
#include "storage.h"
#include "keccak.cuh"
#include "mp2g.h"

namespace mp2g {

GLD void store_digest(uint8_t* out, u64 i, const u64 h[4]) {
  u64* o = (u64*)(out + 32 * i);
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = h[k];
}

__global__ void __launch_bounds__(128) keccak256_batch_kernel(const uint8_t* __restrict__ msgs, u32 stride, const u32* __restrict__ lens,
                                                              u32 len, u32 count, uint8_t* __restrict__ out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  u32 n = lens ? lens[i] : len;
  if (n > stride) n = stride;  // the host cannot see device lengths: a lane never reads past its row
  u64 h[4];
  keccak256_lanes((const u64*)(msgs + (u64)stride * i), n, h);
  store_digest(out, i, h);
}

// the 16 nibbles of a lane's 8 bytes, high nibble first, as two little-endian words of 8 nibble bytes
GLD u64 nibbles_of(u32 x) {
  u64 t = x;
  t = (t | (t << 16)) & 0x0000FFFF0000FFFFULL;
  t = (t | (t << 8)) & 0x00FF00FF00FF00FFULL;  // byte k in the low half of 16-bit slot k
  return ((t >> 4) & 0x000F000F000F000FULL) | ((t & 0x000F000F000F000FULL) << 8);
}

__global__ void __launch_bounds__(128) storage_slot_keys_kernel(u64 slot, const uint8_t* __restrict__ parents, const uint8_t* __restrict__ keys,
                                                                u32 n_keys, u32 evm_offset, u32 count, uint8_t* __restrict__ locations,
                                                                uint8_t* __restrict__ mpt_keys, uint8_t* __restrict__ nibbles,
                                                                u32* __restrict__ n_overflow) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  // loc: 32 bytes as four little-endian lanes, lane 0 = the most significant eight bytes of the big-endian integer
  u64 loc[4] = {0, 0, 0, __builtin_bswap64(slot)};
  if (parents) {
    const u64* p = (const u64*)(parents + 32 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) loc[k] = p[k];
  }
#pragma unroll 1
  for (u32 j = 0; j < n_keys; j++) {  // keccak256(left_pad32(key) || loc), the outer key first   (eth.rs:236-252)
    const u64* key = (const u64*)(keys + 32 * (i * n_keys + j));
    u64 m[8];
#pragma unroll
    for (int k = 0; k < 4; k++) { m[k] = key[k]; m[4 + k] = loc[k]; }
    keccak256_regs<8>(m, loc);
  }
  // + evm_offset on the 256-bit big-endian integer (eth.rs:253-264); checked_add's overflow is counted, the leaf zeroed
  u64 q3 = __builtin_bswap64(loc[3]), q2 = __builtin_bswap64(loc[2]), q1 = __builtin_bswap64(loc[1]), q0 = __builtin_bswap64(loc[0]);
  q3 += evm_offset;
  u64 carry = q3 < (u64)evm_offset;
  q2 += carry; carry = carry & (q2 == 0);
  q1 += carry; carry = carry & (q1 == 0);
  q0 += carry; carry = carry & (q0 == 0);
  loc[0] = __builtin_bswap64(q0); loc[1] = __builtin_bswap64(q1); loc[2] = __builtin_bswap64(q2); loc[3] = __builtin_bswap64(q3);
  u64 h[4];
  keccak256_regs<4>(loc, h);
  if (carry) {
#pragma unroll
    for (int k = 0; k < 4; k++) loc[k] = h[k] = 0;
    if (n_overflow) atomicAdd(n_overflow, 1u);
  }
  if (locations) store_digest(locations, i, loc);
  if (mpt_keys) store_digest(mpt_keys, i, h);
  if (nibbles) {
    u64* o = (u64*)(nibbles + 64 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      o[2 * k] = carry ? 0 : nibbles_of((u32)h[k]);
      o[2 * k + 1] = carry ? 0 : nibbles_of((u32)(h[k] >> 32));
    }
  }
}

// The leaf node opened as RLP: list [hex-prefix path, rlp(value)]. Every byte read is at an offset below n. On MP2G_MPT_LEAF_OK:
// where the value's bytes start, how many they are (0..32), the path's first byte offset and its nibble count.
struct LeafParts {
  u32 status, path_off, n_nibbles, val_off, val_len;
};
GLD LeafParts open_leaf(const uint8_t* __restrict__ node, u32 n) {
  LeafParts r = {MP2G_MPT_LEAF_MALFORMED, 0, 0, 0, 0};
  if (n < 1) return r;
  // the list header: 0xc0 + L, or 0xf8 L with L >= 56; the payload ends exactly at n
  const u32 h = node[0];
  u32 off, L;
  if (h >= 0xc0 && h <= 0xf7) { off = 1; L = h - 0xc0; }
  else if (h == 0xf8 && n >= 2) { off = 2; L = node[1]; if (L < 56) return r; }
  else return r;
  if (off + L != n || off >= n) return r;
  // item 0, the path: one byte below 0x80, or 0x80 + k followed by k bytes; 1..33 bytes
  u32 b = node[off], p_off, p_len;
  if (b < 0x80) { p_off = off; p_len = 1; }
  else if (b <= 0xb7) { p_off = off + 1; p_len = b - 0x80; }
  else return r;
  const u32 next = p_off + p_len;
  if (p_len < 1 || p_len > 33 || next >= n) return r;  // next >= n: no room for item 1
  // item 1, a string that ends the list: nothing follows it, so the list holds exactly two items
  b = node[next];
  u32 v_off, v_len;
  if (b < 0x80) { v_off = next; v_len = 1; }
  else if (b <= 0xb7) { v_off = next + 1; v_len = b - 0x80; }
  else if (b == 0xb8 && next + 1 < n) { v_off = next + 2; v_len = node[next + 1]; if (v_len < 56) return r; }
  else return r;
  if (v_off + v_len != n) return r;
  // the hex prefix: 2 = leaf with an even path, 3 = leaf with an odd path whose first nibble is the byte's low one
  const u32 flag = (u32)node[p_off] >> 4;
  if (flag != 2 && flag != 3) { r.status = MP2G_MPT_LEAF_NOT_A_LEAF; return r; }
  if (2 * (p_len - 1) + (flag & 1) > 64) return r;  // 33 bytes with an odd prefix: 65 nibbles, longer than a key
  // item 1's payload is the RLP of the value: one byte below 0x80, or 0x80 + k followed by k <= 32 bytes that fill the item
  r.status = MP2G_MPT_LEAF_BAD_VALUE;
  if (v_len < 1) return r;
  const u32 c = node[v_off];
  if (c < 0x80) { if (v_len != 1) return r; r.val_off = v_off; r.val_len = 1; }
  else if (c <= 0x80 + 32) { if (v_len != 1 + (c - 0x80)) return r; r.val_off = v_off + 1; r.val_len = c - 0x80; }
  else return r;
  r.status = MP2G_MPT_LEAF_OK;
  r.path_off = p_off;
  r.n_nibbles = 2 * (p_len - 1) + (flag & 1);
  return r;
}

__global__ void __launch_bounds__(128) mpt_storage_leaves_kernel(const uint8_t* __restrict__ nodes, u32 stride, const u32* __restrict__ lens,
                                                                 const uint8_t* __restrict__ mpt_keys, u32 count, uint8_t* __restrict__ hashes,
                                                                 uint8_t* __restrict__ words, u32* __restrict__ n_nibbles,
                                                                 u32* __restrict__ status) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint8_t* node = nodes + (u64)stride * i;
  u32 n = lens[i];
  if (n > stride) n = stride;
  if (hashes) {
    u64 h[4];
    keccak256_lanes((const u64*)node, n, h);
    store_digest(hashes, i, h);
  }
  LeafParts p = open_leaf(node, n);
  if (p.status == MP2G_MPT_LEAF_OK && mpt_keys) {
    // the path's nibbles against the last n_nibbles nibbles of the key
    const uint8_t* key = mpt_keys + 32 * i;
    const u32 odd = p.n_nibbles & 1, first = 64 - p.n_nibbles;
    u32 diff = 0;
    for (u32 t = 0; t < p.n_nibbles; t++) {
      const u32 pn = t + 2 - odd;  // nibble index inside the path's bytes: past the flag, and past the padding of an even path
      const u32 pb = node[p.path_off + pn / 2], kb = key[(first + t) / 2];
      diff |= ((pn & 1) ? pb & 15 : pb >> 4) ^ (((first + t) & 1) ? kb & 15 : kb >> 4);
    }
    if (diff) p.status = MP2G_MPT_LEAF_KEY_MISMATCH;
  }
  const bool ok = p.status == MP2G_MPT_LEAF_OK;
  if (words) {
    // left_pad32(value): output byte k is value byte k - (32 - val_len), built in four lanes whose indices are static
    u64 w[4] = {0, 0, 0, 0};
    const u32 pad = ok ? 32 - p.val_len : 32;
#pragma unroll
    for (int k = 0; k < 32; k++)
      if ((u32)k >= pad) w[k / 8] |= (u64)node[p.val_off + k - pad] << (8 * (k % 8));
    store_digest(words, i, w);
  }
  if (n_nibbles) n_nibbles[i] = ok ? p.n_nibbles : 0;
  if (status) status[i] = p.status;
}

// ---- launchers --------------------------------------------------------------------------------
hipError_t keccak256_batch(hipStream_t st, const uint8_t* msgs, u32 stride, const u32* lens, u32 len, u32 count, uint8_t* out) {
  if (!count) return hipSuccess;
  if (!stride || stride % 8 || stride > MP2G_KECCAK_MAX_STRIDE) return hipErrorInvalidValue;
  hipLaunchKernelGGL(keccak256_batch_kernel, dim3((count + 127) / 128), dim3(128), 0, st, msgs, stride, lens, len, count, out);
  return hipGetLastError();
}
hipError_t storage_slot_keys(hipStream_t st, u64 slot, const uint8_t* parents, const uint8_t* keys, u32 n_keys, u32 evm_offset, u32 count,
                             uint8_t* locations, uint8_t* mpt_keys, uint8_t* nibbles, u32* n_overflow) {
  if (n_overflow) {
    hipError_t e = hipMemsetAsync(n_overflow, 0, sizeof(u32), st);
    if (e != hipSuccess) return e;
  }
  if (!count) return hipSuccess;
  if (n_keys > MP2G_LEAF_MAX_KEYS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(storage_slot_keys_kernel, dim3((count + 127) / 128), dim3(128), 0, st, slot, parents, keys, n_keys, evm_offset, count,
                     locations, mpt_keys, nibbles, n_overflow);
  return hipGetLastError();
}
hipError_t mpt_storage_leaves(hipStream_t st, const uint8_t* nodes, u32 stride, const u32* lens, const uint8_t* mpt_keys, u32 count,
                              uint8_t* hashes, uint8_t* words, u32* n_nibbles, u32* status) {
  if (!count) return hipSuccess;
  if (!stride || stride % 8 || stride > MP2G_KECCAK_MAX_STRIDE) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mpt_storage_leaves_kernel, dim3((count + 127) / 128), dim3(128), 0, st, nodes, stride, lens, mpt_keys, count, hashes,
                     words, n_nibbles, status);
  return hipGetLastError();
}
}  // namespace mp2g
