// Device harness for the arithmetic headers of csrc: every routine of gl.cuh, gl5.cuh, poseidon.cuh, poseidon_wave.cuh and
// ntt_arith.cuh behind an element-wise kernel, so that tests/test_gpu_field_device.py can run the DEVICE bodies (the
// __HIP_DEVICE_COMPILE__ branches) on chosen operands. Test infrastructure only: libmp2g_devfield.so, not part of libmp2gpu.so.
//
// No checking happens here. A host entry point (mp2gt_*) takes host arrays, allocates, copies, launches on the default stream,
// synchronises, copies back, frees, and returns the HIP status. Kernels run one lane per case in 256-thread blocks with a bounds
// guard; an empty case list is an error (no empty grid is ever launched).
#include "gl5.cuh"
#include "ntt_arith.cuh"
#include "poseidon_wave.cuh"
#include "field_ops.h"

using namespace mp2g;

namespace {

constexpr int BLOCK = 256;

// ---- scalar operations: (a, b, c) -> (o0, o1), listed in field_ops.h ------------------------------------------------------------
#define SCALAR_OPS(X) SCALAR_OPS_HD(X) SCALAR_OPS_DEV(X)

// gl_mul_2pow<S> for a run-time S < 192: a switch over the 192 instantiations
template <int S0, int N> __device__ __forceinline__ u64 mul_2pow_range(u64 x, u32 s) {
  if constexpr (N == 1) return gl_mul_2pow<S0>(x);
  else return s < S0 + N / 2 ? mul_2pow_range<S0, N / 2>(x, s) : mul_2pow_range<S0 + N / 2, N - N / 2>(x, s);
}
__device__ u64 mul_2pow_any(u64 x, u32 s) { return mul_2pow_range<0, 192>(x, s < 192 ? s : 0); }

enum ScalarOp {
#define X(name, body) OP_##name,
  SCALAR_OPS(X)
#undef X
  N_SCALAR_OPS
};
const char* const scalar_names[] = {
#define X(name, body) #name,
  SCALAR_OPS(X)
#undef X
};

template <int OP>
__global__ void __launch_bounds__(BLOCK) scalar_kernel(size_t n, const u64* pa, const u64* pb, const u64* pc, u64* p0, u64* p1) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const u64 a = pa[i], b = pb[i], c = pc[i];
  u64 o0 = 0, o1 = 0;
  (void)a; (void)b; (void)c;
#define X(name, body) if constexpr (OP == OP_##name) { body; }
  SCALAR_OPS(X)
#undef X
  p0[i] = o0;
  p1[i] = o1;
}

// ---- gl_cols: T products per case, add (f = 0) or add_scaled by f, then value() ---------------------------------------------------
template <int T, int F>
__global__ void __launch_bounds__(BLOCK) cols_kernel(size_t n, const u64* pa, const u64* pb, u64* out) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  gl_cols acc;
#pragma unroll
  for (int k = 0; k < T; k++) {
    if (F == 0) acc.add(pa[i * T + k], pb[i * T + k]); else acc.add_scaled(pa[i * T + k], pb[i * T + k], F);
  }
  out[i] = acc.value();
}

// ---- vector operations: x[n][W], y[n][W] (or a shared table), a small scalar k -> out[n][W], flag[n] -------------------------------
#define VEC_OPS(X)                                                                                 \
  X(gl2_mul, 2)                                                                                    \
  X(gl2_inv, 2)                                                                                    \
  X(gl2_scale, 2)                                                                                  \
  X(gl5_mul, 5)                                                                                    \
  X(gl5_sqr, 5)                                                                                    \
  X(gl5_small, 5)                                                                                  \
  X(gl5_mul_kz, 5)                                                                                 \
  X(gl5_frob1, 5)                                                                                  \
  X(gl5_frob2, 5)                                                                                  \
  X(gl5_inv, 5)                                                                                    \
  X(gl5_norm, 5)                                                                                   \
  X(gl5_sqrt, 5)                                                                                   \
  X(gl5_is_square, 5)                                                                              \
  X(gl5_sgn0, 5)                                                                                   \
  X(p2_external, 12)                                                                               \
  X(p2_external_rc, 12)                                                                            \
  X(p2_internal, 12)                                                                               \
  X(poseidon_mds, 12)                                                                              \
  X(poseidon_mds_rc, 12)                                                                           \
  X(poseidon2_perm, 12)                                                                            \
  X(poseidon_perm, 12)                                                                             \
  X(two_to_one_p2, 12)                                                                             \
  X(two_to_one_p, 12)                                                                              \
  X(wp2_external, 12)                                                                              \
  X(wp2_internal, 12)                                                                              \
  X(wp2_perm, 12)

enum VecOp {
#define X(name, w) VOP_##name,
  VEC_OPS(X)
#undef X
  N_VEC_OPS
};
const char* const vec_names[] = {
#define X(name, w) #name,
  VEC_OPS(X)
#undef X
};
constexpr int vec_width[] = {
#define X(name, w) w,
  VEC_OPS(X)
#undef X
};

__device__ __forceinline__ gl5 load5(const u64* p) { return gl5_make(p[0], p[1], p[2], p[3], p[4]); }
__device__ __forceinline__ void store5(u64* p, const gl5& v) {
#pragma unroll
  for (int j = 0; j < 5; j++) p[j] = v.c[j];
}

// One lane per case. y: per-case second operand for the binary operations; for the *_rc layers a table of 12 round constants shared
// by all cases, or null for the production table at round k.
template <int OP>
__global__ void __launch_bounds__(BLOCK) vec_kernel(size_t n, const u64* px, const u64* py, u32 k, u64* pout, u64* pflag) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  u64 flag = 0;
  if constexpr (OP == VOP_gl2_mul || OP == VOP_gl2_inv || OP == VOP_gl2_scale) {
    const gl2 x = gl2_make(px[2 * i], px[2 * i + 1]);
    gl2 r;
    if constexpr (OP == VOP_gl2_mul) r = gl2_mul(x, gl2_make(py[2 * i], py[2 * i + 1]));
    else if constexpr (OP == VOP_gl2_inv) r = gl2_inv(x);
    else r = gl2_scale(x, py[2 * i]);
    pout[2 * i] = r.a;
    pout[2 * i + 1] = r.b;
  } else if constexpr (vec_width[OP] == 5) {
    const gl5 x = load5(px + 5 * i);
    gl5 r = gl5_zero();
    if constexpr (OP == VOP_gl5_mul) r = gl5_mul(x, load5(py + 5 * i));
    else if constexpr (OP == VOP_gl5_sqr) r = gl5_sqr(x);
    else if constexpr (OP == VOP_gl5_small) r = gl5_small(x, k);
    else if constexpr (OP == VOP_gl5_mul_kz) r = gl5_mul_kz(x, k);
    else if constexpr (OP == VOP_gl5_frob1) r = gl5_frob1(x);
    else if constexpr (OP == VOP_gl5_frob2) r = gl5_frob2(x);
    else if constexpr (OP == VOP_gl5_inv) r = gl5_inv(x);
    else if constexpr (OP == VOP_gl5_norm) r.c[0] = gl5_norm(x);
    else if constexpr (OP == VOP_gl5_sqrt) flag = gl5_sqrt(x, r) ? 1 : 0;
    else if constexpr (OP == VOP_gl5_is_square) flag = gl5_is_square(x) ? 1 : 0;
    else flag = gl5_sgn0(x) ? 1 : 0;
    store5(pout + 5 * i, r);
  } else {
    u64 s[12];
#pragma unroll
    for (int j = 0; j < 12; j++) s[j] = px[12 * i + j];
    if constexpr (OP == VOP_p2_external) p2_external_rc<false>(s, nullptr);
    else if constexpr (OP == VOP_p2_external_rc) p2_external_rc<true>(s, py ? py : c_p2_ext + 12 * k);
    else if constexpr (OP == VOP_p2_internal) p2_internal(s);
    else if constexpr (OP == VOP_poseidon_mds) poseidon_mds_rc<false>(s, nullptr);
    else if constexpr (OP == VOP_poseidon_mds_rc) poseidon_mds_rc<true>(s, py ? py : c_p_rc + 12 * k);
    else if constexpr (OP == VOP_poseidon2_perm) poseidon2_perm(s);
    else if constexpr (OP == VOP_poseidon_perm) poseidon_perm(s);
    else {
      u64 o[4];
      if constexpr (OP == VOP_two_to_one_p2) two_to_one<MP2G_POSEIDON2>(s, s + 4, o); else two_to_one<MP2G_POSEIDON>(s, s + 4, o);
#pragma unroll
      for (int j = 0; j < 12; j++) s[j] = j < 4 ? o[j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 12; j++) pout[12 * i + j] = s[j];
  }
  pflag[i] = flag;
}

// Lane-cooperative forms: state g in lanes 0..11 of 16-lane group g. All 16 lanes of every group of the block call (groups past n
// carry zeros and store nothing), as poseidon_wave.cuh requires.
template <int OP>
__global__ void __launch_bounds__(BLOCK) wave_kernel(size_t n, const u64* px, u64* pout) {
  const size_t g = ((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 4;
  const int l = threadIdx.x & 15;
  const bool live = g < n && l < 12;
  u64 x = live ? px[12 * g + l] : 0;
  if constexpr (OP == VOP_wp2_external) x = wp2_external(x, l);
  else if constexpr (OP == VOP_wp2_internal) x = wp2_internal(x, l, c_p2_diag[l < 12 ? l : 0]);
  else x = wp2_perm(x, l);
  if (live) pout[12 * g + l] = x;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct DevBuf {
  u64* p = nullptr;
  hipError_t alloc(size_t words) { return hipMalloc(&p, words * sizeof(u64)); }
  hipError_t up(const u64* h, size_t words) {
    hipError_t e = alloc(words);
    return e != hipSuccess ? e : hipMemcpy(p, h, words * sizeof(u64), hipMemcpyHostToDevice);
  }
  hipError_t down(u64* h, size_t words) { return hipMemcpy(h, p, words * sizeof(u64), hipMemcpyDeviceToHost); }
  ~DevBuf() { if (p) (void)hipFree(p); }
};
#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) return (int)e_; } while (0)
hipError_t finish() {
  hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : hipDeviceSynchronize();
}
unsigned blocks_for(size_t lanes) { return (unsigned)((lanes + BLOCK - 1) / BLOCK); }
bool bad_count(size_t n) { return n == 0 || n > ((size_t)1 << 24); }
// the lane-cooperative forms take 16 lanes per case, every other operation one
template <int OP> void launch_vec(size_t n, const u64* x, const u64* y, u32 k, u64* out, u64* flag) {
  if constexpr (OP == VOP_wp2_external || OP == VOP_wp2_internal || OP == VOP_wp2_perm)
    wave_kernel<OP><<<blocks_for(n * 16), BLOCK>>>(n, x, out);
  else
    vec_kernel<OP><<<blocks_for(n), BLOCK>>>(n, x, y, k, out, flag);
}

}  // namespace

extern "C" {

const char* mp2gt_scalar_op_name(int op) { return op >= 0 && op < N_SCALAR_OPS ? scalar_names[op] : nullptr; }
const char* mp2gt_vec_op_name(int op) { return op >= 0 && op < N_VEC_OPS ? vec_names[op] : nullptr; }
int mp2gt_vec_op_width(int op) { return op >= 0 && op < N_VEC_OPS ? vec_width[op] : 0; }

// out0[i], out1[i] = op(a[i], b[i], c[i]), i < n
int mp2gt_scalar(int op, size_t n, const u64* a, const u64* b, const u64* c, u64* out0, u64* out1) {
  if (op < 0 || op >= N_SCALAR_OPS || bad_count(n)) return (int)hipErrorInvalidValue;
  DevBuf da, db, dc, d0, d1;
  CK(da.up(a, n)); CK(db.up(b, n)); CK(dc.up(c, n)); CK(d0.alloc(n)); CK(d1.alloc(n));
  switch (op) {
#define X(name, body) case OP_##name: scalar_kernel<OP_##name><<<blocks_for(n), BLOCK>>>(n, da.p, db.p, dc.p, d0.p, d1.p); break;
    SCALAR_OPS(X)
#undef X
  }
  CK(finish());
  CK(d0.down(out0, n)); CK(d1.down(out1, n));
  return 0;
}

// out[i] = value() of a gl_cols fed a[i][0..terms) * b[i][0..terms) with add (f = 0) or add_scaled(.., f)
int mp2gt_cols(int terms, int f, size_t n, const u64* a, const u64* b, u64* out) {
  const bool known = (f == 0 && (terms == 1 || terms == 5 || terms == 25)) || (terms == 1 && f == 2) || (terms == 3 && (f == 3 || f == 6));
  if (!known || bad_count(n)) return (int)hipErrorInvalidValue;
  DevBuf da, db, d0;
  CK(da.up(a, n * terms)); CK(db.up(b, n * terms)); CK(d0.alloc(n));
  const unsigned nb = blocks_for(n);
  if (terms == 1 && f == 0) cols_kernel<1, 0><<<nb, BLOCK>>>(n, da.p, db.p, d0.p);
  else if (terms == 5 && f == 0) cols_kernel<5, 0><<<nb, BLOCK>>>(n, da.p, db.p, d0.p);
  else if (terms == 25 && f == 0) cols_kernel<25, 0><<<nb, BLOCK>>>(n, da.p, db.p, d0.p);
  else if (terms == 1 && f == 2) cols_kernel<1, 2><<<nb, BLOCK>>>(n, da.p, db.p, d0.p);
  else if (terms == 3 && f == 3) cols_kernel<3, 3><<<nb, BLOCK>>>(n, da.p, db.p, d0.p);
  else cols_kernel<3, 6><<<nb, BLOCK>>>(n, da.p, db.p, d0.p);
  CK(finish());
  CK(d0.down(out, n));
  return 0;
}

// x, out: [n][width]; y: [n][width], or 12 shared round constants when y_shared, or null; flag: [n]
int mp2gt_vec(int op, size_t n, const u64* x, const u64* y, int y_shared, u32 k, u64* out, u64* flag) {
  if (op < 0 || op >= N_VEC_OPS || bad_count(n)) return (int)hipErrorInvalidValue;
  const size_t w = vec_width[op];
  if (k >= 8 && (op == VOP_p2_external_rc)) return (int)hipErrorInvalidValue;
  if (k >= 30 && (op == VOP_poseidon_mds_rc)) return (int)hipErrorInvalidValue;
  const bool binary = op == VOP_gl2_mul || op == VOP_gl2_scale || op == VOP_gl5_mul;
  if (binary && (!y || y_shared)) return (int)hipErrorInvalidValue;
  DevBuf dx, dy, d0, df;
  CK(dx.up(x, n * w)); CK(d0.alloc(n * w)); CK(df.alloc(n));
  if (y) CK(dy.up(y, y_shared ? 12 : n * w));
  CK(hipMemset(d0.p, 0, n * w * sizeof(u64)));
  CK(hipMemset(df.p, 0, n * sizeof(u64)));
  switch (op) {
#define X(name, width) case VOP_##name: launch_vec<VOP_##name>(n, dx.p, dy.p, k, d0.p, df.p); break;
    VEC_OPS(X)
#undef X
  }
  CK(finish());
  CK(d0.down(out, n * w)); CK(df.down(flag, n));
  return 0;
}

}  // extern "C"
