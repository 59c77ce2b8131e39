// Host-side launchers for the node-hash kernels of index_hash.hip: every node of every row's cells tree, and every node of a row
// tree / index tree, level by level on the device (MerkleCell::aggregate mp2-v1/src/indexing/cell.rs:120-157, RowPayload::aggregate
// row.rs:257-317, IndexNode::aggregate index.rs:61-101).
#pragma once
#include "gl.cuh"

namespace mp2g {
// the cells of ONE height of the sbbst over `cells` positions, passed by value (a height of 255 cells has at most 128 nodes): the
// kernel reads entry blockIdx.y through the scalar cache, and no device table has to outlive the call
#define MP2G_CELLS_PER_LAUNCH 128
struct CellsLevel {
  u64 id[MP2G_CELLS_PER_LAUNCH];        // the cell's column identifier
  int16_t node[MP2G_CELLS_PER_LAUNCH];  // position - 1: the cell's slot in node-major `work`, its column is node + 1
  int16_t left[MP2G_CELLS_PER_LAUNCH], right[MP2G_CELLS_PER_LAUNCH];  // children's slots, -1 = none (hashes as all zero)
};
// one launch: work[node][row][4] = H(work[left][row] || work[right][row] || id || values[row][node + 1][0..8)) for the `count` cells
// of lv and every row. nodes_out (NULL or [rows][cells][4]) receives the same digests row-major; the cell root_node also goes to
// roots_out[row][4]. values [rows][n_cols][8] u32. Digest buffers are 16-byte aligned.
hipError_t cells_level_hash(hipStream_t st, int variant, const CellsLevel& lv, u32 count, const u32* values, u32 n_cols, u32 rows,
                            u64* work, u64* nodes_out, u64* roots_out, int root_node);
// roots[row][4] = 0 for every row: hash_no_pad(&[]) of a row without cells
hipError_t cells_empty_roots(hipStream_t st, u64* roots, u32 rows);
// the same two for a list of rows (MerkleTreeKvDb::aggregate over touched(), ryhope/src/lib.rs:179-222, applied to the rows' cells
// trees): lane t handles table row row_idx[t] (device array, n_idx entries < rows, duplicates allowed: they write the same words).
// work is compact, [cell][n_idx][4]; nodes_out / roots_out are the whole table's and are written at the listed rows only.
hipError_t cells_rows_level_hash(hipStream_t st, int variant, const CellsLevel& lv, u32 count, const u32* values, u32 n_cols,
                                 const u32* row_idx, u32 n_idx, u64* work, u64* nodes_out, u64* roots_out, int root_node);
hipError_t cells_rows_empty_roots(hipStream_t st, u64* roots, const u32* row_idx, u32 n_idx);
// one launch: hashes[i] = H(hashes[left[i]] || hashes[right[i]] || value(min_idx[i]) || value(max_idx[i]) || id || value(i) || payload[i])
// for the `count` nodes i = order[0..count) (all of one height: their children were hashed by earlier launches); value(i) = the 8
// u32 words at values + i * value_stride; payload NULL = all zero. left / right / min_idx / max_idx / order are device arrays.
hipError_t row_level_hash(hipStream_t st, int variant, const u32* order, u32 count, const int32_t* left, const int32_t* right,
                          const u32* min_idx, const u32* max_idx, u64 id, const u32* values, u64 value_stride, const u64* payload,
                          u64* hashes);

// Re-hashing a few lineages of a row tree (the closure of the touched nodes, tree_shape_touched): every level has one to a few
// nodes, and a launch of row_level_hash per level costs a launch plus five one-lane permutations run one after the other whatever
// the level's size (profiles/index_hashes.md). row_update_fused is ONE launch of ONE workgroup for the whole closure: 16-lane
// groups, one closure node per group per round, the lane-cooperative permutation of poseidon_wave.cuh, a workgroup barrier between
// levels. Poseidon2 only. The caller takes it while the closure's widest level has at most MP2G_ROW_UPDATE_FUSED_WIDTH nodes
// (64 = the groups of the block, one round per level; profiles/index_hashes.md has the measurements behind the figure) and the
// closure has at most MP2G_ROW_UPDATE_FUSED_LEVELS levels (a bound on the length of one launch: 256 x 5 cooperative permutations
// per round; the reference's trees, sbbst and scapegoat, stay far below it up to 2^31 nodes); everything else goes level by level
// through row_level_hash over the same compact lists.
#define MP2G_ROW_UPDATE_FUSED_WIDTH 64
#define MP2G_ROW_UPDATE_FUSED_LEVELS 256
// order: the closure's nodes level by level (device); level_off [n_levels + 1] (device): level l is order[level_off[l] ..
// level_off[l + 1]), and every child of a node of level l that is in the closure lies in a lower level; the other arguments as
// row_level_hash takes them. Writes hashes[i] for the nodes i of order, nothing else.
hipError_t row_update_fused(hipStream_t st, const u32* order, const u32* level_off, u32 n_levels, const int32_t* left,
                            const int32_t* right, const u32* min_idx, const u32* max_idx, u64 id, const u32* values, u64 value_stride,
                            const u64* payload, u64* hashes);
}  // namespace mp2g
