// What the C ABI of the Keccak-256 and MPT entry points (storage_api.hip, mpt_api.hip) judges alike: a table of rows at a stride,
// the alignment of a device pointer, and the upload of a host array. Each refusal names its argument.
#pragma once
#include "ctx.h"
#include "storage.h"

namespace mp2g {
inline int aligned_arg(const void* p, uintptr_t a, const char* name) {
  if ((uintptr_t)p & (a - 1)) return fail("invalid argument: %s is not %u-byte aligned", name, (unsigned)a);
  return 0;
}
inline int aligned8(const void* p, const char* name) { return aligned_arg(p, 8, name); }
inline int stride_arg(uint32_t stride) {
  if (stride == 0 || stride % 8 || stride > MP2G_KECCAK_MAX_STRIDE)
    return fail("invalid argument: stride %u is not a multiple of 8 in 8..%d", stride, MP2G_KECCAK_MAX_STRIDE);
  return 0;
}
// the host's lengths against the row
inline int lens_arg(const uint32_t* lens, uint32_t count, uint32_t stride) {
  for (uint32_t i = 0; i < count; i++)
    if (lens[i] > stride) return fail("invalid argument: lens: entry %u is %u, above the stride %u", i, lens[i], stride);
  return 0;
}
inline hipError_t upload(DevBuf& d, const void* src, size_t bytes, hipStream_t st) {
  hipError_t e = d.alloc(bytes);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, st);
}
}  // namespace mp2g
