// Launchers of the MPT inclusion-proof kernels (mpt.hip): every distinct node of a proof set hashed and opened once, then every
// proof walked from its root to its leaf over a table of node indices. One lane per node / per proof; the bodies are mpt.cuh's.
#pragma once
#include "storage.h"

namespace mp2g {
// hashes[i] = keccak256(node i), info[i] = its info word (include/mp2g.h). nodes and hashes 8-byte aligned, stride a multiple of 8;
// a lane clamps lens[i] to stride; each output may be null.
hipError_t mpt_open_nodes(hipStream_t st, const uint8_t* nodes, u32 stride, const u32* lens, u32 n_nodes, uint8_t* hashes, u32* info);
// The walk of `count` proofs: paths [count][max_depth] node indices (the root first), depths [count], mpt_keys [count][32] (any
// alignment), roots (or null) at root_stride 0 or 32. nodes, hashes, roots and words 8-byte aligned; each output may be null.
hipError_t mpt_verify_paths(hipStream_t st, const uint8_t* nodes, u32 stride, const u32* lens, const uint8_t* hashes, const u32* info,
                            u32 n_nodes, const u32* paths, const u32* depths, u32 max_depth, const uint8_t* mpt_keys, u32 count,
                            const uint8_t* roots, u32 root_stride, u32 mode, u32* status, u32* fail_level, uint8_t* words, u32* val_off,
                            u32* val_len, uint8_t* consumed);
}  // namespace mp2g
