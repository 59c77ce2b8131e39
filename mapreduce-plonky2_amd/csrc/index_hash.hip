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
// (measured in profiles/index_hashes.md); there is no lane-cooperative variant for them.
#include "index_hash.h"
#include "poseidon.cuh"

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

template <int V, bool VEC>
__global__ void __launch_bounds__(256) cells_level_kernel(const CellsLevel lv, const u32* __restrict__ values, u32 n_cols, u32 rows,
                                                          u64* __restrict__ work, u64* __restrict__ nodes_out, u64* __restrict__ roots_out,
                                                          int root_node) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int node = lv.node[blockIdx.y], l = lv.left[blockIdx.y], rt = lv.right[blockIdx.y];  // uniform over the block
  u64 s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  if (l >= 0) load_digest(work + ((u64)l * rows + r) * 4, s[0], s[1], s[2], s[3]);
  if (rt >= 0) load_digest(work + ((u64)rt * rows + r) * 4, s[4], s[5], s[6], s[7]);
  u32 v[8];
  load_u256<VEC>(values + (r * n_cols + (u32)(node + 1)) * 8, v);
  perm<V>(s);
  s[0] = lv.id[blockIdx.y];
#pragma unroll
  for (int k = 0; k < 7; k++) s[1 + k] = v[k];
  perm<V>(s);
  s[0] = v[7];
  perm<V>(s);
  store_digest(work + ((u64)node * rows + r) * 4, s);
  if (nodes_out) store_digest(nodes_out + (r * (n_cols - 1) + (u32)node) * 4, s);
  if (node == root_node) store_digest(roots_out + r * 4, s);
}

__global__ void __launch_bounds__(256) cells_empty_roots_kernel(u64* __restrict__ roots, u32 rows) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const u64 s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  store_digest(roots + r * 4, s);
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
