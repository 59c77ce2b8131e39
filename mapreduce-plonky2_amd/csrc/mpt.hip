// MPT inclusion proofs on the device, for gfx950: what ties the leaf of an eth_getProof answer to its storage root, and a storage
// root to a state root (mpt.cuh names what of the reference this replaces).
//
// Two kernels, split the way the data is shared: the leaves of a table share their upper nodes, so a node is hashed and opened once
// (stage 1, one lane per distinct node: the sponge of keccak.cuh, ALU-bound, then the item scan over bytes the sponge has just
// read), and the proofs are walked over a table of node indices (stage 2, one lane per proof: no Keccak, a chain of dependent
// loads: the index, the node's hash and info word, one key byte, the child's 32 bytes). Neither indexes a private array by a
// run-time value.
#include "mpt.h"
#include "mpt.cuh"

namespace mp2g {

__global__ void __launch_bounds__(128) mpt_open_nodes_kernel(const uint8_t* __restrict__ nodes, u32 stride, const u32* __restrict__ lens,
                                                             u32 n_nodes, uint8_t* __restrict__ hashes, u32* __restrict__ info) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const uint8_t* node = nodes + (u64)stride * i;
  u32 n = lens[i];
  if (n > stride) n = stride;  // the host cannot see device lengths: a lane never reads past its row
  if (hashes) {
    u64 h[4];
    keccak256_lanes((const u64*)node, n, h);
    u64* o = (u64*)(hashes + 32 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = h[k];
  }
  if (info) info[i] = mpt_open_node(node, n);
}

struct DeviceNodes {
  const uint8_t* base;
  const u32* lens;
  u32 stride;
  GLD const uint8_t* node(u32 idx) const { return base + (u64)stride * idx; }
  GLD u32 len(u32 idx) const { const u32 n = lens[idx]; return n > stride ? stride : n; }
};

__global__ void __launch_bounds__(128) mpt_verify_paths_kernel(DeviceNodes nodes, const u64* __restrict__ hashes, const u32* __restrict__ info,
                                                               u32 n_nodes, const u32* __restrict__ paths, const u32* __restrict__ depths,
                                                               u32 max_depth, const uint8_t* __restrict__ mpt_keys, u32 count,
                                                               const uint8_t* __restrict__ roots, u32 root_stride, u32 mode,
                                                               u32* __restrict__ status, u32* __restrict__ fail_level, uint8_t* __restrict__ words,
                                                               u32* __restrict__ val_off, u32* __restrict__ val_len, uint8_t* __restrict__ consumed) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const MptWalk r = mpt_walk_path(nodes, hashes, info, n_nodes, paths + i * max_depth, depths[i], max_depth, mpt_keys + 32 * i,
                                  roots ? (const u64*)(roots + (u64)root_stride * i) : nullptr, mode,
                                  consumed ? consumed + i * max_depth : nullptr);
  if (status) status[i] = r.status;
  if (fail_level) fail_level[i] = r.fail_level;
  if (words && mode != MP2G_MPT_VALUE_RAW) {
    u64* o = (u64*)(words + 32 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = r.word[k];
  }
  if (val_off) val_off[i] = r.val_off;
  if (val_len) val_len[i] = r.val_len;
}

// ---- launchers --------------------------------------------------------------------------------
hipError_t mpt_open_nodes(hipStream_t st, const uint8_t* nodes, u32 stride, const u32* lens, u32 n_nodes, uint8_t* hashes, u32* info) {
  if (!n_nodes) return hipSuccess;
  if (!stride || stride % 8 || stride > MP2G_KECCAK_MAX_STRIDE) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mpt_open_nodes_kernel, dim3((n_nodes + 127) / 128), dim3(128), 0, st, nodes, stride, lens, n_nodes, hashes, info);
  return hipGetLastError();
}
hipError_t mpt_verify_paths(hipStream_t st, const uint8_t* nodes, u32 stride, const u32* lens, const uint8_t* hashes, const u32* info,
                            u32 n_nodes, const u32* paths, const u32* depths, u32 max_depth, const uint8_t* mpt_keys, u32 count,
                            const uint8_t* roots, u32 root_stride, u32 mode, u32* status, u32* fail_level, uint8_t* words, u32* val_off,
                            u32* val_len, uint8_t* consumed) {
  if (!count) return hipSuccess;
  if (!stride || stride % 8 || stride > MP2G_KECCAK_MAX_STRIDE || !max_depth || max_depth > MP2G_MPT_MAX_DEPTH ||
      (root_stride != 0 && root_stride != 32) || mode > MP2G_MPT_VALUE_RAW)
    return hipErrorInvalidValue;
  const DeviceNodes table = {nodes, lens, stride};
  hipLaunchKernelGGL(mpt_verify_paths_kernel, dim3((count + 127) / 128), dim3(128), 0, st, table, (const u64*)hashes, info, n_nodes, paths,
                     depths, max_depth, mpt_keys, count, roots, root_stride, mode, status, fail_level, words, val_off, val_len, consumed);
  return hipGetLastError();
}
}  // namespace mp2g
