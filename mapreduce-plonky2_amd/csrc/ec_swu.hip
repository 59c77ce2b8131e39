// simple_swu on its own, for gfx950: mp2-common/src/group_hashing/sswu_value.rs:31-77 of GF(p^5) elements given directly, without
// the sponge of map_to_curve_point -- what map_to_curve_kernel (ecgfp5.hip) does after its hash, with the same outputs. A unit of
// its own, so that the digest kernels' code object stays as it was.
#include "ecgfp5.h"
#include "ec_curve.cuh"

namespace mp2g {

// one lane per element; limbs are any u64 and are read mod p (GoldilocksField(x) of sswu_value.rs:135-137): reduced once at the load
__global__ void __launch_bounds__(128) swu_kernel(const u64* u_in, u32 count, u64* w_out, u64* wei_out) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  gl5 u;
  for (int k = 0; k < 5; k++) u.c[k] = gl_canon(u_in[5 * (u64)i + k]);
  pt p = simple_swu(u);
  pt_emit(p, w_out ? w_out + 5 * (u64)i : nullptr, wei_out ? wei_out + 11 * (u64)i : nullptr);
}

hipError_t ec_swu(hipStream_t s, const u64* u_in, u32 count, u64* w_out, u64* wei_out) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(swu_kernel, dim3((count + 127) / 128), dim3(128), 0, s, u_in, count, w_out, wei_out);
  return hipGetLastError();
}
}  // namespace mp2g
