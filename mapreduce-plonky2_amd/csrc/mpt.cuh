// MPT inclusion proofs (include/mp2g.h, "MPT inclusion proofs"): the opening of one node of any kind and the walk of one path from
// the root to its leaf, one body for the kernels of mpt.hip and for the host test (tools/hosttest/mpt_host_test.cpp).
// Replaces, on the value (non-circuit) side:
//   mp2-common/src/eth.rs:345-399                  ProofQuery::verify_storage_proof / verify_state_proof
//   mp2-common/src/mpt_sequential/utils.rs:69-121  visit_proof / visit_node
//   mp2-common/src/mpt_sequential/mod.rs:163-234   Circuit::verify_mpt_proof, whose key pointer counts from the other end
//
// A node is read by byte loads from global memory at run-time offsets (cache hits after the sponge in stage 1; dependent loads in
// stage 2), never from a register array: no private array is indexed by a run-time value, so nothing goes to scratch. Every offset
// is below the node's clamped length before it is used. That holds in the walk too, which trusts no bit of an info word for a
// read: it checks what the word implies against the node's length and calls the node BAD_NODE otherwise.
//
// The bodies are GLHD, as keccak.cuh's are.
#pragma once
#include "keccak.cuh"
#include "mp2g.h"

namespace mp2g {

// one RLP item whose header byte is at off < end: a string (one byte below 0x80, 0x80 + k with k <= 55, 0xb8 k with k >= 56) or a
// short list 0xc0 + k, which is recognised, not entered. ok is 0 for any other header byte and for an item that runs past end.
struct MptItem {
  u32 ok, is_list, p_off, p_len, next;
};
GLHD MptItem mpt_item(const uint8_t* __restrict__ node, u32 off, u32 end) {
  MptItem it = {0, 0, 0, 0, 0};
  const u32 b = node[off];
  if (b < 0x80) { it.p_off = off; it.p_len = 1; }
  else if (b <= 0xb7) { it.p_off = off + 1; it.p_len = b - 0x80; }
  else if (b == 0xb8) {
    if (off + 1 >= end) return it;
    it.p_off = off + 2; it.p_len = node[off + 1];
    if (it.p_len < 56) return it;
  }
  else if (b >= 0xc0 && b <= 0xf7) { it.p_off = off + 1; it.p_len = b - 0xc0; it.is_list = 1; }
  else return it;
  it.next = it.p_off + it.p_len;
  it.ok = it.next <= end;
  return it;
}

// the list header of a node of n bytes: 0xc0 + L, 0xf8 L (L >= 56) or 0xf9 hi lo (L >= 256), the payload ending exactly at n.
// Returns the header's length, 0 when the node is MALFORMED.
GLHD u32 mpt_list_header(const uint8_t* __restrict__ node, u32 n) {
  if (n < 1) return 0;
  const u32 h = node[0];
  u32 off, L;
  if (h >= 0xc0 && h <= 0xf7) { off = 1; L = h - 0xc0; }
  else if (h == 0xf8 && n >= 2) { off = 2; L = node[1]; if (L < 56) return 0; }
  else if (h == 0xf9 && n >= 3) { off = 3; L = (u32)node[1] << 8 | node[2]; if (L < 256) return 0; }
  else return 0;
  return off + L == n ? off : 0;
}

GLHD u32 mpt_info_invalid(u32 reason) { return MP2G_MPT_NODE_INVALID | reason << 2; }

// The info word of the node of n bytes (include/mp2g.h gives the rules in this order and the word bit by bit).
GLHD u32 mpt_open_node(const uint8_t* __restrict__ node, u32 n) {
  const u32 hl = mpt_list_header(node, n);
  if (!hl) return mpt_info_invalid(MP2G_MPT_NODE_MALFORMED);
  // the items, in order: the first bad one decides; an 18th item ends the scan. What a branch and what a two-item node need of
  // them is kept in scalars as the scan passes, since the count is known only at its end.
  u32 off = hl, count = 0, mask = 0, branch_bad = 0;
  u32 i0_str = 0, i0_off = 0, i0_len = 0, i1_hdr = 0, i1_list = 0, i1_len = 0;
  while (off < n) {
    if (count == 17) return mpt_info_invalid(MP2G_MPT_NODE_ITEM_COUNT);
    const MptItem it = mpt_item(node, off, n);
    if (!it.ok) return mpt_info_invalid(MP2G_MPT_NODE_MALFORMED);
    if (count == 0) { i0_str = !it.is_list; i0_off = it.p_off; i0_len = it.p_len; }
    if (count == 1) { i1_hdr = off; i1_list = it.is_list; i1_len = it.p_len; }
    const bool hash = !it.is_list && it.p_len == 32, empty = !it.is_list && it.p_len == 0;  // 32 bytes: 0xa0 and the hash
    if (count < 16) {
      if (hash) mask |= 1u << count;
      else if (!empty && !branch_bad) branch_bad = it.is_list ? MP2G_MPT_NODE_EMBEDDED_CHILD : MP2G_MPT_NODE_MALFORMED;
    } else if (!empty && !branch_bad) branch_bad = MP2G_MPT_NODE_BRANCH_VALUE;
    off = it.next;
    count++;
  }
  if (count == 17) {
    if (branch_bad) return mpt_info_invalid(branch_bad);
    return MP2G_MPT_NODE_BRANCH | hl << 5 | mask << 8;
  }
  if (count != 2) return mpt_info_invalid(MP2G_MPT_NODE_ITEM_COUNT);
  // two items: item 0 is the hex-prefix path
  if (!i0_str || i0_len < 1 || i0_len > 33) return mpt_info_invalid(MP2G_MPT_NODE_MALFORMED);
  const u32 flag = (u32)node[i0_off] >> 4;
  if (flag > 3) return mpt_info_invalid(MP2G_MPT_NODE_BAD_PREFIX);
  const u32 nib = 2 * (i0_len - 1) + (flag & 1);
  if (nib > 64) return mpt_info_invalid(MP2G_MPT_NODE_MALFORMED);
  if (flag < 2) {  // an extension: at least one nibble, then the child's hash
    if (nib < 1) return mpt_info_invalid(MP2G_MPT_NODE_MALFORMED);
    if (i1_list) return mpt_info_invalid(MP2G_MPT_NODE_EMBEDDED_CHILD);
    if (i1_len != 32) return mpt_info_invalid(MP2G_MPT_NODE_MALFORMED);
    return MP2G_MPT_NODE_EXTENSION | hl << 5 | nib << 8 | i1_hdr << 16;
  }
  if (i1_list) return mpt_info_invalid(MP2G_MPT_NODE_MALFORMED);  // a leaf's item 1 is a string; the walk judges its content
  return MP2G_MPT_NODE_LEAF | hl << 5 | nib << 8 | i1_hdr << 16;
}

// 32 bytes at any alignment as four little-endian lanes, the form keccak256_lanes gives a digest in
GLHD void mpt_load32(const uint8_t* __restrict__ p, u64 out[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    u64 w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) w |= (u64)p[8 * k + j] << (8 * j);
    out[k] = w;
  }
}

// nibbles [0, n_nib) of the hex-prefix path whose first byte is path[0], against nibbles [ptr, ptr + n_nib) of key: 0 when equal
GLHD u32 mpt_path_diff(const uint8_t* __restrict__ path, u32 n_nib, const uint8_t* __restrict__ key, u32 ptr) {
  const u32 odd = n_nib & 1;
  u32 diff = 0;
  for (u32 t = 0; t < n_nib; t++) {
    const u32 pn = t + 2 - odd;  // nibble index inside the path's bytes: past the flag, and past the padding of an even path
    const u32 pb = path[pn / 2], kb = key[(ptr + t) / 2];
    diff |= ((pn & 1) ? pb & 15 : pb >> 4) ^ (((ptr + t) & 1) ? kb & 15 : kb >> 4);
  }
  return diff;
}

// what a walk leaves of one proof; word is valid (and non-zero at most) on MP2G_MPT_PATH_OK
struct MptWalk {
  u32 status, fail_level, val_off, val_len;
  u64 word[4];
};

// left_pad32 of the len <= 32 bytes at p, as four lanes whose indices are static
GLHD void mpt_left_pad32(const uint8_t* __restrict__ p, u32 len, u64 w[4]) {
  const u32 pad = 32 - len;
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = 0;
#pragma unroll
  for (int k = 0; k < 32; k++)
    if ((u32)k >= pad) w[k / 8] |= (u64)p[k - pad] << (8 * (k % 8));
}

// the value of a leaf, item 1's payload [v_off, v_off + v_len) of node, by mode: 1 when sound, the word in w
GLHD bool mpt_leaf_value(const uint8_t* __restrict__ node, u32 v_off, u32 v_len, u32 mode, u64 w[4]) {
  if (mode == MP2G_MPT_VALUE_RAW) return true;
  if (v_len < 1) return false;
  const u32 c = node[v_off], end = v_off + v_len;
  if (mode == MP2G_MPT_VALUE_WORD) {
    // the RLP of one string of at most 32 bytes that fills the item: the rules of mp2g_mpt_storage_leaves
    if (c < 0x80) { if (v_len != 1) return false; mpt_left_pad32(node + v_off, 1, w); return true; }
    if (c > 0x80 + 32 || v_len != 1 + (c - 0x80)) return false;
    mpt_left_pad32(node + v_off + 1, c - 0x80, w);
    return true;
  }
  // an account: a list of exactly four strings that fills the item, items 2 and 3 of 32 bytes (nonce, balance, storageHash, codeHash)
  u32 off;
  if (c >= 0xc0 && c <= 0xf7) { off = v_off + 1; if (off + (c - 0xc0) != end) return false; }
  else if (c == 0xf8 && v_len >= 2) { off = v_off + 2; const u32 L = node[v_off + 1]; if (L < 56 || off + L != end) return false; }
  else return false;
  u32 storage = 0;
#pragma unroll 1
  for (u32 k = 0; k < 4; k++) {
    if (off >= end) return false;
    const MptItem it = mpt_item(node, off, end);
    if (!it.ok || it.is_list) return false;
    if (k >= 2 && it.p_len != 32) return false;
    if (k == 2) storage = it.p_off;
    off = it.next;
  }
  if (off != end) return false;
  mpt_load32(node + storage, w);
  return true;
}

// The walk of one proof (include/mp2g.h gives the steps in this order). Nodes is the node table: node(idx) is the first byte of
// node idx and len(idx) its length, already clamped to the row. path [depth] are node indices, the root first; hashes [n_nodes][32]
// 8-byte aligned and info [n_nodes] are stage 1's; key [32]; root four lanes or null. consumed [max_depth] (or null) receives the
// number of nibbles consumed on entering each level, 0xff for the levels not entered.
template <class Nodes>
GLHD MptWalk mpt_walk_path(const Nodes& nodes, const u64* __restrict__ hashes, const u32* __restrict__ info, u32 n_nodes,
                           const u32* __restrict__ path, u32 depth, u32 max_depth, const uint8_t* __restrict__ key, const u64* root, u32 mode,
                           uint8_t* __restrict__ consumed) {
  MptWalk r = {MP2G_MPT_PATH_OK, 0, 0, 0, {0, 0, 0, 0}};
  u32 ptr = 0, l = 0;
  u64 expected[4] = {0, 0, 0, 0};
  bool check = root != nullptr;
  if (check) {
#pragma unroll
    for (int k = 0; k < 4; k++) expected[k] = root[k];
  }
  if (depth < 1 || depth > max_depth) { r.status = MP2G_MPT_PATH_BAD_PATH; depth = 0; }
#pragma unroll 1
  for (; l < depth; l++) {
    if (consumed) consumed[l] = (uint8_t)ptr;
    const u32 idx = path[l];
    if (idx >= n_nodes) { r.status = MP2G_MPT_PATH_BAD_PATH; break; }
    if (check) {
      const u64* h = hashes + 4 * (u64)idx;
      if ((h[0] ^ expected[0]) | (h[1] ^ expected[1]) | (h[2] ^ expected[2]) | (h[3] ^ expected[3])) {
        r.status = l ? MP2G_MPT_PATH_HASH_MISMATCH : MP2G_MPT_PATH_ROOT_MISMATCH;
        break;
      }
    }
    check = true;
    const u32 w = info[idx], kind = w & 3, hl = (w >> 5) & 3, n = nodes.len(idx);
    const uint8_t* node = nodes.node(idx);
    if (kind == MP2G_MPT_NODE_INVALID || hl < 1 || hl >= n) { r.status = MP2G_MPT_PATH_BAD_NODE; break; }
    const bool last = l + 1 == depth;
    if (kind == MP2G_MPT_NODE_LEAF && !last) { r.status = MP2G_MPT_PATH_LEAF_ABOVE; break; }
    if (kind != MP2G_MPT_NODE_LEAF && last) { r.status = MP2G_MPT_PATH_NO_LEAF; break; }
    if (kind == MP2G_MPT_NODE_BRANCH) {
      if (ptr >= 64) { r.status = MP2G_MPT_PATH_KEY_LENGTH; break; }
      const u32 mask = (w >> 8) & 0xffff, kb = key[ptr / 2], k = (ptr & 1) ? kb & 15 : kb >> 4;
      if (!(mask >> k & 1)) { r.status = MP2G_MPT_PATH_EMPTY_CHILD; break; }
      const u32 child = hl + k + 32 * (u32)__builtin_popcount(mask & ((1u << k) - 1)) + 1;
      if (child + 32 > n) { r.status = MP2G_MPT_PATH_BAD_NODE; break; }  // an info word that is not this node's
      mpt_load32(node + child, expected);
      ptr += 1;
      continue;
    }
    // an extension or a leaf: the path starts at the list's first item, item 1's header byte is where the info word says
    const u32 nib = (w >> 8) & 0x7f, i1 = w >> 16, p_off = hl + (node[hl] >= 0x80);
    if (nib > 64 || i1 >= n || p_off + (nib + 2) / 2 > i1) { r.status = MP2G_MPT_PATH_BAD_NODE; break; }
    if (kind == MP2G_MPT_NODE_EXTENSION) {
      if (i1 + 33 > n) { r.status = MP2G_MPT_PATH_BAD_NODE; break; }
      if (ptr + nib > 64) { r.status = MP2G_MPT_PATH_KEY_LENGTH; break; }
      if (mpt_path_diff(node + p_off, nib, key, ptr)) { r.status = MP2G_MPT_PATH_KEY_MISMATCH; break; }
      mpt_load32(node + i1 + 1, expected);
      ptr += nib;
      continue;
    }
    const MptItem it = mpt_item(node, i1, n);
    if (!it.ok || it.is_list || it.next != n) { r.status = MP2G_MPT_PATH_BAD_NODE; break; }
    if (ptr + nib != 64) { r.status = MP2G_MPT_PATH_KEY_LENGTH; break; }
    if (mpt_path_diff(node + p_off, nib, key, ptr)) { r.status = MP2G_MPT_PATH_KEY_MISMATCH; break; }
    if (!mpt_leaf_value(node, it.p_off, it.p_len, mode, r.word)) {
      r.status = MP2G_MPT_PATH_BAD_VALUE;
#pragma unroll
      for (int k = 0; k < 4; k++) r.word[k] = 0;
      break;
    }
    r.val_off = it.p_off;
    r.val_len = it.p_len;
  }
  if (r.status != MP2G_MPT_PATH_OK) r.fail_level = l < depth ? l : 0;
  if (consumed)
    for (u32 t = (r.status != MP2G_MPT_PATH_OK && l < depth) ? l + 1 : l; t < max_depth; t++) consumed[t] = 0xff;
  return r;
}
}  // namespace mp2g
