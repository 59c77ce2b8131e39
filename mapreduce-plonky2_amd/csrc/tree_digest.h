// Host-side launchers for the accumulated-digest kernels of tree_digest.hip: the Ecgfp5 digest every node of a cells tree or row tree
// exposes as public inputs (SplitDigestPoint::accumulate, mp2-common/src/digest.rs:38-47; cells_tree/full_node.rs:26-28,
// row_tree/full_node.rs:78-82), level by level on the device over a tree shape (tree_shape.h), and for the touched closure only.
// A point is the 20 words pt_store writes (X, Z, U, T: a representative, not a canonical form); it stays in that form between the
// stages, so no encode / decode round trip (a GF(p^5) inversion and a square root per point) happens on the way.
#pragma once
#include "gl.cuh"
#include "index_hash.h"

namespace mp2g {
// one launch: acc[i] = own[i] (+ acc[left[i]]) (+ acc[right[i]]) for the `count` nodes i = order[0..count), all of one height: their
// children were summed by earlier launches. left / right / order are device arrays; own and acc [n][20] do not overlap.
hipError_t digest_level(hipStream_t st, const u32* order, u32 count, const int32_t* left, const int32_t* right, const u64* own, u64* acc);

// The closure of the touched nodes (tree_shape_touched) is a few lineages: every level has one to a few nodes, and a launch per level
// costs a launch plus one or two point additions whatever the level's size. digest_update_fused is ONE launch of ONE 128-lane
// workgroup for the whole closure, lane t takes node order[level_off[l] + t] of level l, a workgroup barrier between levels. The
// caller takes it while the closure's widest level has at most MP2G_TREE_DIGEST_FUSED_WIDTH nodes (the lanes of the block) and the
// closure has at most MP2G_ROW_UPDATE_FUSED_LEVELS levels; everything else goes level by level through digest_level over the same
// compact lists. Both write acc[i] for the nodes i of order and no other word (profiles/tree_digests.md has the measurements).
#define MP2G_TREE_DIGEST_FUSED_WIDTH 128
hipError_t digest_update_fused(hipStream_t st, const u32* order, const u32* level_off, u32 n_levels, const int32_t* left,
                               const int32_t* right, const u64* own, u64* acc);

// one launch: nodes[row][node] = map_to_curve(id || values[row][node + 1][0..8)) + nodes[row][left] + nodes[row][right] for the
// `count` cells of lv (one height of the sbbst over n_cols - 1 positions) and the rows row_idx[0..n) (device array; NULL = the rows
// 0..n-1). nodes [rows][n_cols-1][20] row-major, read and written in place: Cell::values_digest (verifiable-db/src/cells_tree/
// mod.rs:65-72) and its accumulation up the cells tree in one pass. Duplicates in row_idx write the same words.
hipError_t cells_digest_level(hipStream_t st, int variant, const CellsLevel& lv, u32 count, const u32* values, u32 n_cols,
                              const u32* row_idx, u32 n, u64* nodes);

// own[row] = row_id * (sum over columns of D(id_c || value_c)) as row_digest_kernel computes it (mp2-v1/src/values_extraction/
// mod.rs:499-571), for the rows row_idx[0..n) (device; NULL = 0..n-1). The row's unique columns are the 8 * n_unique words at
// unique + row * unique_stride. cells_nodes (NULL or [rows][n_cols-1][20]): the sum is D(id_0 || value_0) + cells_nodes[row][root_node]
// instead of mapping every column again. col_ids is a device array of n_cols words.
hipError_t row_own(hipStream_t st, int variant, const u64* col_ids, u32 n_cols, const u32* values, const u32* unique, u32 unique_stride,
                   u32 n_unique, const u64* cells_nodes, int root_node, const u32* row_idx, u32 n, u64* own);

// pt_emit of the points frac[idx[t]] (device idx; NULL = t) into the compact outputs w_out [count][5] / wei_out [count][11] (either NULL)
hipError_t emit_indexed(hipStream_t st, const u64* frac, const u32* idx, u32 count, u64* w_out, u64* wei_out);
}  // namespace mp2g
