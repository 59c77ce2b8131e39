// MPT subtree digests (include/mp2g.h, "MPT subtree digests"): the shape of a trie as a set of proofs shows it, and the sum of one
// node over its children, one body for the kernels of mpt_digest.hip and for the host test (tools/hosttest/mpt_graph_host_test.cpp).
// Replaces, on the value (non-circuit) side, what the reference accumulates node by node up the storage trie:
//   mp2-v1/src/values_extraction/branch.rs:77-112      DV and N of a branch: the sums over the children that are proved
//   mp2-v1/src/values_extraction/extension.rs:53-61    an extension exposes its child's DV and N
//   mp2-v1/src/values_extraction/public_inputs.rs:23-36  H, K, T, DV, DM, N
//
// The shape is built from integer minima and ORs over the proofs, so launches are the only ordering and no result depends on the
// schedule: a policy type P gives min64 / min32 / or32, atomics on the device and plain code on the host. Per node the passes keep
//   ref     (proof << 8 | level) of the node's reference occurrence: the lowest level of the lowest accepted proof through it
//   child   [16] the lowest node index seen below each nibble (an extension's child is slot 0)
//   parent, les  the reference occurrence's parent and level | entered << 8 | slot << 16, written by the proof that owns ref
//   direct  an occurrence differs from the reference one, or two nodes share a (parent, slot): rules (a) and (b)
//   above   a proof through the node reaches a `direct` node further down: rule (c)
// Rule (c) walks proofs, not parent pointers. The two agree: above a node that is not `direct` every proof continues with that
// node's one parent, and where a proof leaves the parent pointers rule (a) has marked both ends.
//
// No private array is indexed by a run-time value: a proof is walked by loads of its path row and of the info words.
#pragma once
#include "gl.cuh"
#include "mp2g.h"

namespace mp2g {

constexpr u64 MPT_REF_NONE = ~0ull;

GLHD u64 mpt_ref_key(u32 proof, u32 level) { return (u64)proof << 8 | level; }
GLHD u32 mpt_key_nibble(const uint8_t* __restrict__ key, u32 ptr) {
  const u32 b = key[ptr / 2];
  return (ptr & 1) ? b & 15 : b >> 4;
}
// the nibbles a node consumes: one at a branch, the path's count at an extension or a leaf (up to 127 in a hostile word)
GLHD u32 mpt_own_nibbles(u32 info) { return (info & 3) == MP2G_MPT_NODE_BRANCH ? 1 : (info >> 8) & 0x7f; }

// Whether proof i contributes: decided before anything of it is written. No index is trusted before it is held against n_nodes.
GLHD bool mpt_graph_accept(const u32* __restrict__ info, u32 n_nodes, const u32* __restrict__ path, u32 depth, u32 max_depth,
                           const u32* __restrict__ status, u32 i) {
  if (status && status[i] != MP2G_MPT_PATH_OK) return false;
  if (depth < 1 || depth > max_depth) return false;
  u32 ptr = 0;
#pragma unroll 1
  for (u32 l = 0; l < depth; l++) {
    const u32 x = path[l];
    if (x >= n_nodes) return false;
    const u32 w = info[x], kind = w & 3;
    if (l + 1 == depth ? kind != MP2G_MPT_NODE_LEAF : (kind != MP2G_MPT_NODE_BRANCH && kind != MP2G_MPT_NODE_EXTENSION)) return false;
    ptr += mpt_own_nibbles(w);
    if (ptr > 64) return false;
  }
  return ptr == 64;
}

// one node of one accepted proof
struct MptOcc {
  u32 node, parent, level, entered, slot;
};
GLHD u32 mpt_occ_pack(const MptOcc& o) { return o.level | o.entered << 8 | o.slot << 16; }

// f(occurrence) for every level of an ACCEPTED proof, the root first
template <class F>
GLHD void mpt_graph_visit(const u32* __restrict__ info, const u32* __restrict__ path, u32 depth, const uint8_t* __restrict__ key, F&& f) {
  u32 ptr = 0, parent = MP2G_MPT_NO_NODE, slot = 0;
#pragma unroll 1
  for (u32 l = 0; l < depth; l++) {
    const u32 x = path[l], w = info[x];
    const MptOcc o = {x, parent, l, ptr, slot};
    f(o);
    slot = (w & 3) == MP2G_MPT_NODE_BRANCH ? mpt_key_nibble(key, ptr) : 0;  // an accepted proof enters a branch below 64
    ptr += mpt_own_nibbles(w);
    parent = x;
  }
}

// Pass 1, minima. Returns whether the proof is accepted.
template <class P>
GLHD bool mpt_graph_minima(const u32* __restrict__ info, u32 n_nodes, const u32* __restrict__ path, u32 depth, u32 max_depth,
                           const uint8_t* __restrict__ key, const u32* __restrict__ status, u32 i, u64* ref, u32* child) {
  if (!mpt_graph_accept(info, n_nodes, path, depth, max_depth, status, i)) return false;
  mpt_graph_visit(info, path, depth, key, [&](const MptOcc& o) {
    P::min64(ref + o.node, mpt_ref_key(i, o.level));
    if (o.parent != MP2G_MPT_NO_NODE) P::min32(child + 16 * (u64)o.parent + o.slot, o.node);
  });
  return true;
}

// Pass 2, the owner writes: the occurrence that is a node's ref leaves its tuple. One writer per node.
GLHD void mpt_graph_own(const u32* __restrict__ info, const u32* __restrict__ path, u32 depth, const uint8_t* __restrict__ key, u32 i,
                        const u64* __restrict__ ref, u32* __restrict__ parent, u32* __restrict__ les) {
  mpt_graph_visit(info, path, depth, key, [&](const MptOcc& o) {
    if (ref[o.node] != mpt_ref_key(i, o.level)) return;
    parent[o.node] = o.parent;
    les[o.node] = mpt_occ_pack(o);
  });
}

// Pass 3, compare and OR: rules (a) and (b)
template <class P>
GLHD void mpt_graph_compare(const u32* __restrict__ info, const u32* __restrict__ path, u32 depth, const uint8_t* __restrict__ key,
                            const u32* __restrict__ parent, const u32* __restrict__ les, const u32* __restrict__ child, u32* direct) {
  mpt_graph_visit(info, path, depth, key, [&](const MptOcc& o) {
    const bool top = o.parent == MP2G_MPT_NO_NODE;
    if (parent[o.node] != o.parent || les[o.node] != mpt_occ_pack(o)) {
      P::or32(direct + o.node, 1);
      if (!top) P::or32(direct + o.parent, 1);
    }
    if (!top && child[16 * (u64)o.parent + o.slot] != o.node) P::or32(direct + o.parent, 1);
  });
}

// Pass 4, rule (c): everything above the deepest `direct` node of the proof. It reads `direct` and writes `above` only.
template <class P>
GLHD void mpt_graph_above(const u32* __restrict__ path, u32 depth, const u32* __restrict__ direct, u32* above) {
  u32 deepest = 0;
#pragma unroll 1
  for (u32 l = 1; l < depth; l++)
    if (direct[path[l]]) deepest = l;
#pragma unroll 1
  for (u32 l = 0; l < deepest; l++) P::or32(above + path[l], 1);
}

// what the passes leave of one node
struct MptNodeShape {
  u32 state, via, parent, entered, level;
};
GLHD MptNodeShape mpt_graph_node(u32 x, const u64* __restrict__ ref, const u32* __restrict__ parent, const u32* __restrict__ les,
                                 const u32* __restrict__ direct, const u32* __restrict__ above) {
  const u64 r = ref[x];
  if (r == MPT_REF_NONE) return {MP2G_MPT_SUBTREE_UNREACHED, MP2G_MPT_NO_NODE, MP2G_MPT_NO_NODE, 0xff, 0};
  const u32 w = les[x];
  return {(direct[x] | above[x]) ? (u32)MP2G_MPT_SUBTREE_CONFLICT : (u32)MP2G_MPT_SUBTREE_OK, (u32)(r >> 8), parent[x], (w >> 8) & 0xff, w & 0xff};
}

// The sum of one OK node, whose children (all OK, all one level down) hold theirs: a leaf takes the point of the proof that owns
// it, an extension its child's, a branch the sum of the children the proofs showed, in nibble order. E gives the point type and
// load / add / neutral / store: the curve on the device, tokens in the host test. acc null: the leaf counts alone.
template <class E>
GLHD void mpt_graph_sum(u32 x, const u32* __restrict__ info, const u32* __restrict__ child, const u64* __restrict__ ref,
                        const u64* __restrict__ leaf_frac, u64* acc, u32* n_leaves) {
  const u32 kind = info[x] & 3;
  typename E::point p = E::neutral();
  u32 n = 0;
  if (kind == MP2G_MPT_NODE_LEAF) {
    if (acc) p = E::load(leaf_frac + 20 * (ref[x] >> 8));
    n = 1;
  } else {
    const u32* c = child + 16 * (u64)x;
    const u32 slots = kind == MP2G_MPT_NODE_BRANCH ? 16 : 1;
    bool first = true;
#pragma unroll 1
    for (u32 s = 0; s < slots; s++) {
      const u32 k = c[s];
      if (k == MP2G_MPT_NO_NODE) continue;  // a child the proofs never showed costs nothing
      n += n_leaves[k];
      if (!acc) continue;
      if (first) p = E::load(acc + 20 * (u64)k);
      else p = E::add(p, E::load(acc + 20 * (u64)k));
      first = false;
    }
  }
  if (acc) E::store(acc + 20 * (u64)x, p);
  n_leaves[x] = n;
}
}  // namespace mp2g
