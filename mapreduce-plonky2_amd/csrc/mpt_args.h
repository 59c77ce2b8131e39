// What the MPT entry points (mpt_api.hip, mpt_digest_api.hip) refuse alike: the node table and the arguments of a walk.
#pragma once
#include "keccak_args.h"

namespace mp2g {
// stride, nodes and lens, as mp2g_keccak256_batch judges its messages; lens on the host only in the host forms
inline int table_args(const uint8_t* nodes, uint32_t stride, const uint32_t* lens, uint32_t n_nodes, bool host) {
  int rc = stride_arg(stride);
  if (rc || !n_nodes) return rc;
  NEED(nodes, "nodes");
  NEED(lens, "lens");
  return host ? lens_arg(lens, n_nodes, stride) : 0;
}
inline int max_depth_arg(uint32_t max_depth) {
  if (max_depth == 0 || max_depth > MP2G_MPT_MAX_DEPTH) return fail("invalid argument: max_depth %u is not in 1..%d", max_depth, MP2G_MPT_MAX_DEPTH);
  return 0;
}
// everything mp2g_mpt_verify_paths[_dev] refuses but its node table and the alignment of device pointers
inline int walk_args(const uint32_t* paths, const uint32_t* depths, uint32_t max_depth, const uint8_t* mpt_keys, uint32_t root_stride,
                     uint32_t mode) {
  int rc = max_depth_arg(max_depth);
  if (rc) return rc;
  if (root_stride != 0 && root_stride != 32) return fail("invalid argument: root_stride %u is neither 0 nor 32", root_stride);
  if (mode > MP2G_MPT_VALUE_RAW) return fail("invalid argument: mode %u is not an MP2G_MPT_VALUE_*", mode);
  NEED(paths, "paths");
  NEED(depths, "depths");
  NEED(mpt_keys, "mpt_keys");
  return 0;
}
// the host's depths against max_depth: the first one above it is named
inline int depths_arg(const uint32_t* depths, uint32_t count, uint32_t max_depth) {
  for (uint32_t i = 0; i < count; i++)
    if (depths[i] > max_depth) return fail("invalid argument: depths: entry %u is %u, above max_depth %u", i, depths[i], max_depth);
  return 0;
}
}  // namespace mp2g
