// Shift arithmetic of the NTT butterflies: multiplications by powers of two (w_8 = 2^24, w_64 = 2^3) as shifts plus a short
// reduction. Device code only: used by the kernels of ntt.hip, and included by the device test harness
// (tests/devfield/field_dev.hip), which runs each routine on its own.
#pragma once
#include "gl.cuh"

namespace mp2g {

// x * 2^24, 2^48, 2^72 (= w_8, w_8^2, w_8^3), canonical in and out
__device__ __forceinline__ u64 gl_mul_2p24(u64 x) { return gl_canon(gl_reduce96w(x << 24, x >> 40)); }
__device__ __forceinline__ u64 gl_mul_2p48(u64 x) { return gl_reduce128(x << 48, x >> 16); }
__device__ __forceinline__ u64 gl_mul_2p72(u64 x) {
  // x 2^72 = (x << 8) 2^64 with x << 8 = t_hi 2^64 + t_lo, and 2^128 = -2^32 (mod p)
  return gl_sub(gl_reduce128(0, x << 8), (x >> 56) << 32);
}
template <int K> __device__ __forceinline__ u64 gl_mul_w8(u64 x) {  // x * w_8^K, K = 1..3
  return K == 1 ? gl_mul_2p24(x) : (K == 2 ? gl_mul_2p48(x) : gl_mul_2p72(x));
}
// (u - v) * 2^48 and (u - v) * 2^72 without canonicalising the difference first: with s = u - v mod 2^64 and the borrow b, the
// difference is s - b 2^64, and -2^64 2^48 = -2^112 = +2^16, -2^64 2^72 = -2^136 = +2^40 (mod p, 2^96 = -1): the borrow becomes one
// bit of the low word that the shift leaves empty (saves the second subtract chain of gl_sub)
__device__ __forceinline__ u64 gl_sub_mul_2p48(u64 u, u64 v) {
  u32 c0, c1;
  const u32 s0 = __builtin_subc((u32)u, (u32)v, 0u, &c0);
  const u32 s1 = __builtin_subc((u32)(u >> 32), (u32)(v >> 32), c0, &c1);
  const u64 s = gl_mk(s0, s1);
  return gl_reduce128(gl_mk(c1 ? 0x10000u : 0u, s0 << 16), s >> 16);
}
__device__ __forceinline__ u64 gl_sub_mul_2p72(u64 u, u64 v) {
  u32 c0, c1;
  const u32 s0 = __builtin_subc((u32)u, (u32)v, 0u, &c0);
  const u32 s1 = __builtin_subc((u32)(u >> 32), (u32)(v >> 32), c0, &c1);
  const u64 s = gl_mk(s0, s1);
  return gl_sub(gl_reduce128(gl_mk(0u, c1 ? 0x100u : 0u), s << 8), (s >> 56) << 32);
}
template <int K> __device__ __forceinline__ u64 gl_sub_mul_w8(u64 u, u64 v) {  // (u - v) * w_8^K
  return K == 1 ? gl_mul_2p24(gl_sub(u, v)) : (K == 2 ? gl_sub_mul_2p48(u, v) : gl_sub_mul_2p72(u, v));
}
// (u - v) * w_8^K for the forward transform, (u - v) * w_8^-K = (v - u) * w_8^(4-K) for the inverse (w_8^4 = -1)
template <int K> __device__ __forceinline__ u64 bfly_lo(u64 u, u64 v, bool inverse) {
  return inverse ? gl_sub_mul_w8<4 - K>(v, u) : gl_sub_mul_w8<K>(u, v);
}
// x * 2^S (mod p) for a compile-time S in [0, 192), canonical in and out: 2^96 = -1, 2^64 = 2^32 - 1. POWER_OF_TWO_GENERATOR gives
// w_64 = 2^3, so every twiddle of a sub-transform of at most 64 points is such a shift (12-18 issue slots against 29 for a general
// multiplication with a table load in front of it)
template <int S> __device__ __forceinline__ u64 gl_mul_2pow(u64 x) {
  static_assert(S >= 0 && S < 192, "exponent mod 192");
  if constexpr (S == 0) return x;
  else if constexpr (S >= 96) return gl_neg(gl_mul_2pow<S - 96>(x));
  else if constexpr (S <= 32) return gl_canon(gl_reduce96w(x << S, x >> (64 - S)));
  else if constexpr (S < 64) return gl_reduce128(x << S, x >> (64 - S));
  else if constexpr (S == 64) return gl_reduce128(0, x);
  else {  // x 2^S = (x << K) 2^64 with x << K = h 2^64 + t, and 2^128 = -2^32: h < 2^31, so h 2^32 is canonical
    constexpr int K = S - 64;
    return gl_sub(gl_reduce128(0, x << K), (x >> (64 - K)) << 32);
  }
}

}  // namespace mp2g
