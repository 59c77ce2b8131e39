// Device harness for gl_mulw_k of csrc/gl.cuh, the product of the permutations' S-boxes (one middle accumulator, its carry taken from the
// multiply-add): out[i] = gl_mulw_k(a[i], b[i]) as the routine returns it, canon[i] = gl_canon(out[i]). tests/devfield exposes gl_mulw,
// gl_mul, gl_mul_wide and gl_mul_addw, which keep the product that hipcc schedules; this routine is reachable there only through p2_sbox0,
// that is for the operand pairs of a seventh power. Test infrastructure only (tests/test_gpu_mul_carry.py): libmp2g_devfield_mulk.so, a
// library of its own beside tests/devfield, not part of libmp2gpu.so.
//
// No checking happens here. The host entry point takes host arrays, allocates, copies, launches on the default stream, synchronises,
// copies back, frees, and returns the HIP status. One lane per case in 256-thread blocks with a bounds guard; an empty case list is an
// error (no empty grid is ever launched).
#include "gl.cuh"

namespace {

constexpr int BLOCK = 256;

__global__ void __launch_bounds__(BLOCK) mulk_kernel(size_t n, const u64* pa, const u64* pb, u64* out, u64* canon) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const u64 r = gl_mulw_k(pa[i], pb[i]);
  out[i] = r;
  canon[i] = gl_canon(r);
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

}  // namespace

extern "C" {

// out[i] = gl_mulw_k(a[i], b[i]), some u64 congruent to a[i] b[i] (mod p); canon[i] = gl_canon(out[i]); i < n
int mp2gt_mulw_k(size_t n, const u64* a, const u64* b, u64* out, u64* canon) {
  if (n == 0 || n > ((size_t)1 << 24)) return (int)hipErrorInvalidValue;
  DevBuf da, db, d0, d1;
  CK(da.up(a, n)); CK(db.up(b, n)); CK(d0.alloc(n)); CK(d1.alloc(n));
  mulk_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK>>>(n, da.p, db.p, d0.p, d1.p);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out, d0.p, n * sizeof(u64), hipMemcpyDeviceToHost));
  CK(hipMemcpy(canon, d1.p, n * sizeof(u64), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
