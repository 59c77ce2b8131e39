// Accumulated Ecgfp5 digests of a table's trees for gfx950: what SplitDigestPoint::accumulate (mp2-common/src/digest.rs:38-47)
// builds node by node up a cells tree (verifiable-db/src/cells_tree/full_node.rs:26-28, partial_node.rs) and up the row tree
// (row_tree/full_node.rs:78-82), for every node at once: acc[i] = own[i] + acc[left[i]] + acc[right[i]].
//
// The schedule is that of index_hash.hip: one launch per height of a tree shape (tree_shape.h), one lane per node, children read by
// index from what earlier launches wrote. A balanced tree of n nodes costs n - 1 additions (every node is added to its parent once)
// where summing every subtree's range on its own costs n log2 n. Points stay in fractional coordinates (X:Z:U:T, 20 words, the
// representative pt_store writes) between the stages: the cells trees' roots feed the rows' own digests, those feed the row tree,
// and only what a caller downloads is encoded (emit_indexed_kernel).
//
// ALU-bound like sum_kernel: a lane's point is 160 bytes, so a wave's loads are strided; the 10 GF(p^5) products of the complete
// addition dwarf them. Every kernel declares the 128 lanes it is launched with, as the kernels of ecgfp5.hip do: the bound reaches
// the out-of-line EC bodies (ec_curve.cuh).
//
// The update of a touched closure is a few lineages and all latency: while it is narrow it takes ONE launch of one workgroup with a
// barrier between levels (digest_update_fused_kernel, the pattern of row_update_fused_kernel), otherwise one digest_level_kernel
// launch per closure level.
#include "tree_digest.h"
#include "poseidon.cuh"
#include "gl5.cuh"
#include "ec_curve.cuh"

namespace mp2g {

// own[i] plus the accumulated digests of the children that exist: a missing child costs no addition
__device__ __forceinline__ pt digest_node(u32 i, const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                          const u64* __restrict__ own, const u64* acc) {
  const int32_t l = left[i], r = right[i];
  pt p = pt_load(own + 20 * (u64)i);
  if (l >= 0) p = pt_add(p, pt_load(acc + 20 * (u64)l));
  if (r >= 0) p = pt_add(p, pt_load(acc + 20 * (u64)r));
  return p;
}

__global__ void __launch_bounds__(128) digest_level_kernel(const u32* __restrict__ order, u32 count, const int32_t* __restrict__ left,
                                                           const int32_t* __restrict__ right, const u64* __restrict__ own, u64* acc) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const u32 i = order[t];
  pt_store(acc + 20 * (u64)i, digest_node(i, left, right, own, acc));
}

// The closure of the touched nodes, all of its levels in one launch of one 128-lane workgroup: lane t takes node
// order[level_off[lv] + t] of level lv (the caller guarantees that no level is wider than the block). Every lane reaches every
// barrier: no lane returns early, and the trip count of the level loop is a kernel argument. level_off is uniform (scalar loads);
// the children's digests are read per lane (vector loads) after the barrier that follows the level that wrote them.
__global__ void __launch_bounds__(128) digest_update_fused_kernel(const u32* __restrict__ order, const u32* __restrict__ level_off, u32 n_levels,
                                                                  const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                                  const u64* __restrict__ own, u64* acc) {
  const u32 tid = threadIdx.x;
  for (u32 lv = 0; lv < n_levels; lv++) {
    const u32 g = level_off[lv] + tid;
    if (g < level_off[lv + 1]) {
      const u32 i = order[g];
      pt_store(acc + 20 * (u64)i, digest_node(i, left, right, own, acc));
    }
    __syncthreads();  // the level's digests (global memory, written by this block) are visible to the next level's reads
  }
}

// lane = row (or row_idx[lane]), blockIdx.y = cell of this height: which children exist is uniform over the block
template <int V>
__global__ void __launch_bounds__(128) cells_digest_level_kernel(const CellsLevel lv, const u32* __restrict__ values, u32 n_cols,
                                                                 const u32* __restrict__ row_idx, u32 n, u64* nodes) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u64 row = row_idx ? row_idx[t] : t;
  const int node = lv.node[blockIdx.y], l = lv.left[blockIdx.y], rt = lv.right[blockIdx.y];
  u64 in[9];
  in[0] = lv.id[blockIdx.y];
  const u32* v = values + (row * n_cols + (u32)(node + 1)) * 8;
#pragma unroll
  for (int j = 0; j < 8; j++) in[1 + j] = v[j];
  pt p = map_to_curve<V>(in, 9);
  u64* base = nodes + row * (u64)(n_cols - 1) * 20;
  if (l >= 0) p = pt_add(p, pt_load(base + 20 * l));
  if (rt >= 0) p = pt_add(p, pt_load(base + 20 * rt));
  pt_store(base + 20 * node, p);
}

// one lane per row: sum_c D(id_c || value_c) (or D(id_0 || value_0) + the cells tree's root), row id, row_id * sum
template <int V>
__global__ void __launch_bounds__(128) row_own_kernel(const u64* __restrict__ col_ids, u32 n_cols, const u32* __restrict__ values,
                                                      const u32* __restrict__ unique, u32 unique_stride, u32 n_unique,
                                                      const u64* __restrict__ cells_nodes, int root_node, const u32* __restrict__ row_idx,
                                                      u32 n, u64* __restrict__ own) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u64 r = row_idx ? row_idx[t] : t;
  pt rd = pt_neutral();
  const u32 mapped = cells_nodes ? 1 : n_cols;
  for (u32 c = 0; c < mapped; c++) {
    u64 in[9];
    in[0] = col_ids[c];
    const u32* v = values + (r * n_cols + c) * 8;
#pragma unroll
    for (int j = 0; j < 8; j++) in[1 + j] = v[j];
    rd = pt_add(rd, map_to_curve<V>(in, 9));
  }
  if (cells_nodes) rd = pt_add(rd, pt_load(cells_nodes + (r * (u64)(n_cols - 1) + (u32)root_node) * 20));
  // row_unique_data = H(unique columns as 8 big-endian u32 limbs each)   (mod.rs:499-510)
  u64 s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  const u32* uq = unique + r * unique_stride;
  for (u32 c = 0; c < n_unique; c++) {
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = uq[c * 8 + k];
    perm<V>(s);
  }
  // compute_row_id: H(row_unique_data(4) || num_actual_columns)[0..2] -> 128-bit scalar (mod.rs:512-523)
  u64 h[4] = {s[0], s[1], s[2], s[3]};
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  s[0] = h[0]; s[1] = h[1]; s[2] = h[2]; s[3] = h[3]; s[4] = n_cols;
  perm<V>(s);
  u32 k128[4] = {(u32)s[0], (u32)(s[0] >> 32), (u32)s[1], (u32)(s[1] >> 32)};
  pt_store(own + 20 * r, pt_mul128(rd, k128));
}

__global__ void __launch_bounds__(128) emit_indexed_kernel(const u64* __restrict__ frac, const u32* __restrict__ idx, u32 count,
                                                           u64* __restrict__ w_out, u64* __restrict__ wei_out) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const u64 i = idx ? idx[t] : t;
  pt p = pt_load(frac + 20 * i);
  pt_emit(p, w_out ? w_out + 5 * t : nullptr, wei_out ? wei_out + 11 * t : nullptr);
}

// ---- launchers --------------------------------------------------------------------------------
static inline dim3 g128(u32 n) { return dim3((n + 127) / 128); }

hipError_t digest_level(hipStream_t st, const u32* order, u32 count, const int32_t* left, const int32_t* right, const u64* own, u64* acc) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(digest_level_kernel, g128(count), dim3(128), 0, st, order, count, left, right, own, acc);
  return hipGetLastError();
}
hipError_t digest_update_fused(hipStream_t st, const u32* order, const u32* level_off, u32 n_levels, const int32_t* left,
                               const int32_t* right, const u64* own, u64* acc) {
  if (!n_levels) return hipSuccess;
  hipLaunchKernelGGL(digest_update_fused_kernel, dim3(1), dim3(128), 0, st, order, level_off, n_levels, left, right, own, acc);
  return hipGetLastError();
}
hipError_t cells_digest_level(hipStream_t st, int variant, const CellsLevel& lv, u32 count, const u32* values, u32 n_cols,
                              const u32* row_idx, u32 n, u64* nodes) {
  if (!count || !n) return hipSuccess;
  if (count > MP2G_CELLS_PER_LAUNCH) return hipErrorInvalidValue;
  const dim3 grid((n + 127) / 128, count);
  if (variant == MP2G_POSEIDON2) hipLaunchKernelGGL((cells_digest_level_kernel<MP2G_POSEIDON2>), grid, dim3(128), 0, st, lv, values, n_cols, row_idx, n, nodes);
  else if (variant == MP2G_POSEIDON) hipLaunchKernelGGL((cells_digest_level_kernel<MP2G_POSEIDON>), grid, dim3(128), 0, st, lv, values, n_cols, row_idx, n, nodes);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t row_own(hipStream_t st, int variant, const u64* col_ids, u32 n_cols, const u32* values, const u32* unique, u32 unique_stride,
                   u32 n_unique, const u64* cells_nodes, int root_node, const u32* row_idx, u32 n, u64* own) {
  if (!n) return hipSuccess;
  if (variant == MP2G_POSEIDON2)
    hipLaunchKernelGGL((row_own_kernel<MP2G_POSEIDON2>), g128(n), dim3(128), 0, st, col_ids, n_cols, values, unique, unique_stride, n_unique,
                       cells_nodes, root_node, row_idx, n, own);
  else if (variant == MP2G_POSEIDON)
    hipLaunchKernelGGL((row_own_kernel<MP2G_POSEIDON>), g128(n), dim3(128), 0, st, col_ids, n_cols, values, unique, unique_stride, n_unique,
                       cells_nodes, root_node, row_idx, n, own);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t emit_indexed(hipStream_t st, const u64* frac, const u32* idx, u32 count, u64* w_out, u64* wei_out) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(emit_indexed_kernel, g128(count), dim3(128), 0, st, frac, idx, count, w_out, wei_out);
  return hipGetLastError();
}
}  // namespace mp2g
