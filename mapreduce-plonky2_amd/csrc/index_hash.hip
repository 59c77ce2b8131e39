// Off-circuit node hashes of a table's trees for gfx950: every node of every row's cells tree (MerkleCell::aggregate,
// mp2-v1/src/indexing/cell.rs:120-157: H(hL || hR || id || value), 17 limbs, 3 permutations) and every node of a row tree or index
// tree (RowPayload::aggregate row.rs:257-317, IndexNode::aggregate index.rs:61-101: H(hL || hR || min || max || id || value ||
// payload), 37 limbs, 5 permutations), with the sponge of hash_no_pad_batch_kernel (merkle.hip): overwrite-mode absorb at rate 8,
// the state in registers, words taken as they come.
//
// One launch per height, one lane per node; a lane never walks a tree (a runtime-indexed stack of digests would live in scratch).
// Cells: the lanes of a block run along the rows and blockIdx.y names the cell, so that the children's digests, which sit node-major
// in `work`, are read and written as contiguous 32 B per lane, and which children exist is uniform over the block (a scalar branch,
// no divergence). Rows: a lane gathers its two children's digests and the min / max values by index. A level of a few thousand nodes
// costs the latency of its 5 permutations whatever its size, so a balanced tree's upper levels set a floor under the call
// (measured in profiles/index_hashes.md).
//
// Updates re-hash a list of rows' cells trees (the same schedule with a row indirection) and the closure of the touched nodes of a
// row tree. The closure is a few lineages, 11 to 21 levels of one to a few nodes in a balanced tree, so it is all latency: while it
// is narrow it takes ONE launch of one workgroup with the lane-cooperative Poseidon2 of poseidon_wave.cuh and a barrier between
// levels (row_update_fused_kernel, the pattern of witness_exec_kernel in witness_dev.hip); otherwise one row_level_kernel launch
// per closure level.
#include "index_hash.h"
#include "poseidon.cuh"
#include "poseidon_wave.cuh"

namespace mp2g {

// the 8 big-endian u32 words of a U256, kept as 32-bit registers until they are absorbed; VEC: p is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void load_u256(const u32* __restrict__ p, u32 v[8]) {
  if (VEC) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = p[k];
  }
}
__device__ __forceinline__ void load_digest(const u64* __restrict__ p, u64& a, u64& b, u64& c, u64& d) {
  const ulonglong2 q0 = reinterpret_cast<const ulonglong2*>(p)[0], q1 = reinterpret_cast<const ulonglong2*>(p)[1];
  a = q0.x; b = q0.y; c = q1.x; d = q1.y;
}
__device__ __forceinline__ void store_digest(u64* __restrict__ p, const u64 s[12]) {
  reinterpret_cast<ulonglong2*>(p)[0] = make_ulonglong2(s[0], s[1]);
  reinterpret_cast<ulonglong2*>(p)[1] = make_ulonglong2(s[2], s[3]);
}

// one cell of one row: `row` is the row of the table (values, nodes_out, roots_out), `col` of `cols` its column in node-major `work`
template <int V, bool VEC>
__device__ __forceinline__ void cells_node(const CellsLevel& lv, const u32* __restrict__ values, u32 n_cols, u64 row, u64 col, u64 cols,
                                           u64* __restrict__ work, u64* __restrict__ nodes_out, u64* __restrict__ roots_out, int root_node) {
  const int node = lv.node[blockIdx.y], l = lv.left[blockIdx.y], rt = lv.right[blockIdx.y];  // uniform over the block
  u64 s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  if (l >= 0) load_digest(work + ((u64)l * cols + col) * 4, s[0], s[1], s[2], s[3]);
  if (rt >= 0) load_digest(work + ((u64)rt * cols + col) * 4, s[4], s[5], s[6], s[7]);
  u32 v[8];
  load_u256<VEC>(values + (row * n_cols + (u32)(node + 1)) * 8, v);
  perm<V>(s);
  s[0] = lv.id[blockIdx.y];
#pragma unroll
  for (int k = 0; k < 7; k++) s[1 + k] = v[k];
  perm<V>(s);
  s[0] = v[7];
  perm<V>(s);
  store_digest(work + ((u64)node * cols + col) * 4, s);
  if (nodes_out) store_digest(nodes_out + (row * (n_cols - 1) + (u32)node) * 4, s);
  if (node == root_node) store_digest(roots_out + row * 4, s);
}
template <int V, bool VEC>
__global__ void __launch_bounds__(256) cells_level_kernel(const CellsLevel lv, const u32* __restrict__ values, u32 n_cols, u32 rows,
                                                          u64* __restrict__ work, u64* __restrict__ nodes_out, u64* __restrict__ roots_out,
                                                          int root_node) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  cells_node<V, VEC>(lv, values, n_cols, r, r, rows, work, nodes_out, roots_out, root_node);
}
// the same for the rows row_idx[0..n_idx): lane t's column of the compact `work` is t, its row of the table row_idx[t]
template <int V, bool VEC>
__global__ void __launch_bounds__(256) cells_rows_level_kernel(const CellsLevel lv, const u32* __restrict__ values, u32 n_cols,
                                                               const u32* __restrict__ row_idx, u32 n_idx, u64* __restrict__ work,
                                                               u64* __restrict__ nodes_out, u64* __restrict__ roots_out, int root_node) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_idx) return;
  cells_node<V, VEC>(lv, values, n_cols, row_idx[t], t, n_idx, work, nodes_out, roots_out, root_node);
}

__global__ void __launch_bounds__(256) cells_empty_roots_kernel(u64* __restrict__ roots, u32 rows) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const u64 s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  store_digest(roots + r * 4, s);
}

__global__ void __launch_bounds__(256) cells_rows_empty_roots_kernel(u64* __restrict__ roots, const u32* __restrict__ row_idx, u32 n_idx) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_idx) return;
  const u64 s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  store_digest(roots + (u64)row_idx[t] * 4, s);
}

template <int V, bool VEC>
__global__ void __launch_bounds__(256) row_level_kernel(const u32* __restrict__ order, u32 count, const int32_t* __restrict__ left,
                                                        const int32_t* __restrict__ right, const u32* __restrict__ min_idx,
                                                        const u32* __restrict__ max_idx, u64 id, const u32* __restrict__ values,
                                                        u64 value_stride, const u64* __restrict__ payload, u64* __restrict__ hashes) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const u32 i = order[t];
  const int32_t l = left[i], rt = right[i];
  const u32 mn = min_idx[i], mx = max_idx[i];
  u64 s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  if (l >= 0) load_digest(hashes + (u64)l * 4, s[0], s[1], s[2], s[3]);
  if (rt >= 0) load_digest(hashes + (u64)rt * 4, s[4], s[5], s[6], s[7]);
  // each operand is requested one permutation before it is absorbed: one load in flight per permutation (v and w alternate, and
  // both are live across the second permutation) instead of all 28 words held from the start
  u32 v[8], w[8];
  load_u256<VEC>(values + (u64)mn * value_stride, v);
  perm<V>(s);
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = v[k];
  load_u256<VEC>(values + (u64)mx * value_stride, w);
  perm<V>(s);
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = w[k];
  load_u256<VEC>(values + (u64)i * value_stride, v);
  perm<V>(s);
  s[0] = id;
#pragma unroll
  for (int k = 0; k < 7; k++) s[1 + k] = v[k];
  u64 p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  if (payload) load_digest(payload + (u64)i * 4, p0, p1, p2, p3);
  perm<V>(s);
  s[0] = v[7]; s[1] = p0; s[2] = p1; s[3] = p2; s[4] = p3;
  perm<V>(s);
  store_digest(hashes + (u64)i * 4, s);
}

// The closure of the touched nodes, all of its levels in one launch of one workgroup: UPD_LANES / 16 groups of 16 lanes, one node
// per group per round, the sponge state of row_level_kernel in lanes 0..11 of the group (wp2_perm). The five absorbs of
// row_level_kernel lane by lane, overwrite mode at rate 8: [hL hR] [min] [max] [id v0..v6] [v7 p0..p3]; lane l < 8 requests its
// own word of a chunk one permutation before it is absorbed, as the one-lane kernel requests its operands.
// Every lane of the block reaches every barrier: no lane returns early, a group without a node skips the group-uniform loop, and
// the trip count of the level loop is a kernel argument.
constexpr int UPD_LANES = 1024;
__global__ void __launch_bounds__(UPD_LANES) row_update_fused_kernel(const u32* __restrict__ order, const u32* __restrict__ level_off, u32 n_levels,
                                                                    const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                                    const u32* __restrict__ min_idx, const u32* __restrict__ max_idx, u64 id,
                                                                    const u32* __restrict__ values, u64 value_stride,
                                                                    const u64* __restrict__ payload, u64* hashes) {
  const u32 tid = threadIdx.x;
  const int l = (int)(tid & 15);
  for (u32 lv = 0; lv < n_levels; lv++) {
    const u32 hi = level_off[lv + 1];
    for (u32 g = level_off[lv] + (tid >> 4); g < hi; g += UPD_LANES / 16) {
      const u32 i = order[g];
      const int32_t lc = left[i], rc = right[i];
      const u32* vmin = values + (u64)min_idx[i] * value_stride;
      const u32* vmax = values + (u64)max_idx[i] * value_stride;
      const u32* vown = values + (u64)i * value_stride;
      u64 x = 0;  // lanes 8..11 are the capacity, 12..15 carry nothing
      if (l < 4) {
        if (lc >= 0) x = hashes[(u64)lc * 4 + l];
      } else if (l < 8) {
        if (rc >= 0) x = hashes[(u64)rc * 4 + (l - 4)];
      }
      u64 nxt = l < 8 ? vmin[l] : 0;
      x = wp2_perm(x, l);
      if (l < 8) x = nxt;
      nxt = l < 8 ? vmax[l] : 0;
      x = wp2_perm(x, l);
      if (l < 8) x = nxt;
      nxt = l == 0 ? id : (l < 8 ? vown[l - 1] : 0);
      x = wp2_perm(x, l);
      if (l < 8) x = nxt;
      nxt = l == 0 ? vown[7] : (l < 5 && payload ? payload[(u64)i * 4 + (l - 1)] : 0);
      x = wp2_perm(x, l);
      if (l < 5) x = nxt;
      x = wp2_perm(x, l);
      if (l < 4) hashes[(u64)i * 4 + l] = x;
    }
    __syncthreads();  // the level's digests (global memory, written by this block) are visible to the next level's reads
  }
}

#define LAUNCH_VV(kernel, vec, grid, block, st, ...)                                                                       \
  do {                                                                                                                     \
    if (variant == MP2G_POSEIDON2 && (vec)) hipLaunchKernelGGL((kernel<MP2G_POSEIDON2, true>), grid, block, 0, st, __VA_ARGS__);       \
    else if (variant == MP2G_POSEIDON2) hipLaunchKernelGGL((kernel<MP2G_POSEIDON2, false>), grid, block, 0, st, __VA_ARGS__);          \
    else if (variant == MP2G_POSEIDON && (vec)) hipLaunchKernelGGL((kernel<MP2G_POSEIDON, true>), grid, block, 0, st, __VA_ARGS__);    \
    else if (variant == MP2G_POSEIDON) hipLaunchKernelGGL((kernel<MP2G_POSEIDON, false>), grid, block, 0, st, __VA_ARGS__);            \
    else return hipErrorInvalidValue;                                                                                      \
  } while (0)

hipError_t cells_level_hash(hipStream_t st, int variant, const CellsLevel& lv, u32 count, const u32* values, u32 n_cols, u32 rows,
                            u64* work, u64* nodes_out, u64* roots_out, int root_node) {
  if (!count || !rows) return hipSuccess;
  if (count > MP2G_CELLS_PER_LAUNCH) return hipErrorInvalidValue;
  const bool vec = ((uintptr_t)values & 15) == 0;  // a cell's value lies a multiple of 32 bytes after the table's start
  LAUNCH_VV(cells_level_kernel, vec, dim3((rows + 255) / 256, count), dim3(256), st, lv, values, n_cols, rows, work, nodes_out, roots_out,
            root_node);
  return hipGetLastError();
}
hipError_t cells_empty_roots(hipStream_t st, u64* roots, u32 rows) {
  if (!rows) return hipSuccess;
  hipLaunchKernelGGL(cells_empty_roots_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, roots, rows);
  return hipGetLastError();
}
hipError_t cells_rows_level_hash(hipStream_t st, int variant, const CellsLevel& lv, u32 count, const u32* values, u32 n_cols,
                                 const u32* row_idx, u32 n_idx, u64* work, u64* nodes_out, u64* roots_out, int root_node) {
  if (!count || !n_idx) return hipSuccess;
  if (count > MP2G_CELLS_PER_LAUNCH) return hipErrorInvalidValue;
  const bool vec = ((uintptr_t)values & 15) == 0;
  LAUNCH_VV(cells_rows_level_kernel, vec, dim3((n_idx + 255) / 256, count), dim3(256), st, lv, values, n_cols, row_idx, n_idx, work,
            nodes_out, roots_out, root_node);
  return hipGetLastError();
}
hipError_t cells_rows_empty_roots(hipStream_t st, u64* roots, const u32* row_idx, u32 n_idx) {
  if (!n_idx) return hipSuccess;
  hipLaunchKernelGGL(cells_rows_empty_roots_kernel, dim3((n_idx + 255) / 256), dim3(256), 0, st, roots, row_idx, n_idx);
  return hipGetLastError();
}
hipError_t row_update_fused(hipStream_t st, const u32* order, const u32* level_off, u32 n_levels, const int32_t* left,
                            const int32_t* right, const u32* min_idx, const u32* max_idx, u64 id, const u32* values, u64 value_stride,
                            const u64* payload, u64* hashes) {
  if (!n_levels) return hipSuccess;
  hipLaunchKernelGGL(row_update_fused_kernel, dim3(1), dim3(UPD_LANES), 0, st, order, level_off, n_levels, left, right, min_idx, max_idx, id,
                     values, value_stride, payload, hashes);
  return hipGetLastError();
}
hipError_t row_level_hash(hipStream_t st, int variant, const u32* order, u32 count, const int32_t* left, const int32_t* right,
                          const u32* min_idx, const u32* max_idx, u64 id, const u32* values, u64 value_stride, const u64* payload,
                          u64* hashes) {
  if (!count) return hipSuccess;
  const bool vec = ((uintptr_t)values & 15) == 0 && (value_stride & 3) == 0;
  LAUNCH_VV(row_level_kernel, vec, dim3((count + 255) / 256), dim3(256), st, order, count, left, right, min_idx, max_idx, id, values,
            value_stride, payload, hashes);
  return hipGetLastError();
}
}  // namespace mp2g
