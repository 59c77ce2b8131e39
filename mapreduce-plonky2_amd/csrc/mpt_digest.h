// Launchers of the MPT subtree-digest kernels (mpt_digest.hip): the shape of a trie from its proofs, then every node's digest and
// leaf count level by level (include/mp2g.h, "MPT subtree digests"; the bodies are mpt_graph.cuh's).
#pragma once
#include "mp2g.h"
#include "storage.h"

namespace mp2g {
// the words the passes share with the host, at the head of the working block
enum : u32 {
  MPT_CTL_REJECTED = 0,   // proofs that are not accepted
  MPT_CTL_CONFLICT = 1,   // CONFLICT nodes
  MPT_CTL_LEVELS = 2,     // 1 + the deepest level of a reached node
  MPT_CTL_COUNT = 4,      // [65] OK nodes per level
  MPT_CTL_HOST_WORDS = MPT_CTL_COUNT + MP2G_MPT_MAX_DEPTH,  // what the host reads after the shape passes
  MPT_CTL_OFF = MPT_CTL_HOST_WORDS,                         // [66] where each level's list starts in `order`
  MPT_CTL_WORDS = MPT_CTL_OFF + MP2G_MPT_MAX_DEPTH + 2      // 136: the block after it stays 8-byte aligned
};

// One device block of mpt_graph_work_bytes(n_nodes, count) bytes, 8-byte aligned, carved into the arrays of mpt_graph.cuh.
struct MptGraphWork {
  u32* ctl;
  u64* ref;
  u32 *child, *direct, *above, *parent, *les, *rank, *order, *n_leaves;
  uint8_t* accepted;
};
size_t mpt_graph_work_bytes(u32 n_nodes, u32 count);
MptGraphWork mpt_graph_work(void* block, u32 n_nodes, u32 count);

// Everything before the one synchronisation: the four passes over the proofs, then over the nodes the outputs (each may be null),
// the neutral point and N = 0 of every node that is not OK, and the OK nodes listed by level in w.order. n_leaves is never null
// (w.n_leaves when the caller has none). n_nodes and count are not 0.
hipError_t mpt_graph_shape(hipStream_t st, const MptGraphWork& w, const u32* info, u32 n_nodes, const u32* paths, const u32* depths, u32 max_depth,
                           const uint8_t* mpt_keys, const u32* status, u32 count, u64* acc, u32* n_leaves, u32* state, u32* via, u32* parent,
                           uint8_t* entered);
// one level: the `count` nodes order[0..count), whose children are one level down and done. acc null: the leaf counts alone.
hipError_t mpt_subtree_level(hipStream_t st, const MptGraphWork& w, const u32* order, u32 count, const u32* info, const u64* leaf_frac, u64* acc,
                             u32* n_leaves);
}  // namespace mp2g
