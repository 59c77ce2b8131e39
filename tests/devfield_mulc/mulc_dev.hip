// Device harness for the constant-operand multiply-add of csrc/gl.cuh (gl_mulc_addw) over the twelve entries of Poseidon2's internal
// diagonal: out[i] = p2_diag_mul_addw(k, a[i], c[i]), the product exactly as p2_internal forms it for limb k -- gl_mulc_addw<true> where
// the pair (d_k, d_k 2^32 mod p) is narrow, gl_mulc_addw<false> where it is not. One kernel per k, so that the constants are read with a
// constant index as in the permutation. Test infrastructure only (tests/test_gpu_p2_diag.py): libmp2g_devfield_mulc.so, a library of
// its own beside tests/devfield, not part of libmp2gpu.so.
//
// No checking happens here. The host entry point takes host arrays, allocates, copies, launches on the default stream, synchronises,
// copies back, frees, and returns the HIP status. One lane per case in 256-thread blocks with a bounds guard; an empty case list is an
// error (no empty grid is ever launched).
#include "poseidon.cuh"

namespace {

constexpr int BLOCK = 256;

template <int K>
__global__ void __launch_bounds__(BLOCK) mulc_kernel(size_t n, const u64* pa, const u64* pc, u64* out) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = p2_diag_mul_addw(K, pa[i], pc[i]);
}

struct DevBuf {
  u64* p = nullptr;
  hipError_t alloc(size_t words) { return hipMalloc(&p, words * sizeof(u64)); }
  hipError_t up(const u64* h, size_t words) {
    hipError_t e = alloc(words);
    return e != hipSuccess ? e : hipMemcpy(p, h, words * sizeof(u64), hipMemcpyHostToDevice);
  }
  ~DevBuf() { if (p) (void)hipFree(p); }
};
#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) return (int)e_; } while (0)

template <int K>
void launch(int k, size_t n, const u64* a, const u64* c, u64* out) {
  if constexpr (K < 12) {
    if (k == K) mulc_kernel<K><<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK>>>(n, a, c, out);
    else launch<K + 1>(k, n, a, c, out);
  }
}

}  // namespace

extern "C" {

// bit k set: limb k takes gl_mulc_addw<true> (the narrow form)
unsigned mp2gt_mulc_narrow_mask(void) { return POSEIDON2_DIAG_NARROW; }

// out[i] = some u64 congruent to a[i] d_k + c[i] (mod p), i < n, for the diagonal entry k < 12
int mp2gt_mulc_addw(size_t n, const u64* a, const u64* c, int k, u64* out) {
  if (k < 0 || k >= 12 || n == 0 || n > ((size_t)1 << 24)) return (int)hipErrorInvalidValue;
  DevBuf da, dc, d0;
  CK(da.up(a, n)); CK(dc.up(c, n)); CK(d0.alloc(n));
  launch<0>(k, n, da.p, dc.p, d0.p);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out, d0.p, n * sizeof(u64), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
