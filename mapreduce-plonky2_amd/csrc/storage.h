// Launchers of the Keccak-256 kernels (storage.hip): batched hashes, the storage locations and MPT keys of a table's leaves
// (mp2-common/src/eth.rs:233-276) and the opening of MPT storage leaf nodes. One lane per message / leaf; all share keccak.cuh.
#pragma once
#include "extraction.h"

namespace mp2g {
#define MP2G_KECCAK_MAX_STRIDE 65536
// out[i] = keccak256(msgs + i * stride, lens ? min(lens[i], stride) : len). msgs and out 8-byte aligned, stride a multiple of 8.
hipError_t keccak256_batch(hipStream_t st, const uint8_t* msgs, u32 stride, const u32* lens, u32 len, u32 count, uint8_t* out);
// StorageSlot::location / mpt_key / mpt_nibbles of `count` leaves under one slot or under parents[i]; n_keys <= MP2G_LEAF_MAX_KEYS.
// A leaf whose location + evm_offset leaves 256 bits gets zero outputs and bumps *n_overflow (when given). Every pointer 8-byte
// aligned; each output may be null.
hipError_t storage_slot_keys(hipStream_t st, u64 slot, const uint8_t* parents, const uint8_t* keys, u32 n_keys, u32 evm_offset, u32 count,
                             uint8_t* locations, uint8_t* mpt_keys, uint8_t* nibbles, u32* n_overflow);
// hashes[i] = keccak256(node i); words / n_nibbles / status of the leaf opened as RLP (include/mp2g.h). nodes, hashes and words
// 8-byte aligned, stride a multiple of 8; mpt_keys (or null) any alignment; each output may be null.
hipError_t mpt_storage_leaves(hipStream_t st, const uint8_t* nodes, u32 stride, const u32* lens, const uint8_t* mpt_keys, u32 count,
                              uint8_t* hashes, uint8_t* words, u32* n_nibbles, u32* status);
}  // namespace mp2g
