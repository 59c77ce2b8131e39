// GF(p^5) = GF(p)[z] / (z^5 - 3), the Ecgfp5 base field, for host and device code: the field arithmetic of ecgfp5.hip (the
// multiset digest's kernels) and of the witness tape's GF(p^5) opcodes (witness_gf5.h: one definition for the host replay,
// witness.hip, and the device replay, witness_dev.hip). Replaces [dep] plonky2_ecgfp5 curve/base_field.rs (sqrt / inverse /
// sgn0 / legendre) and the base-field square root of plonky2_field.
//
// An element is five canonical coefficients, c[i] of z^i. Every routine takes and returns canonical values.
#pragma once
#include "gl.cuh"
#include "perm_constants.h"

namespace mp2g {

// Small bodies are inlined. The large ones are real functions on the device, which the SWU / scalar-mul kernels call hundreds
// of times; on the host they are `inline` so that every unit that includes this header may define them.
// The device pass compiles them as __device__ functions, exactly as ecgfp5.hip declared them before they moved here: a
// __host__ __device__ function is emitted on first use instead of in source order, and a constant table it names counts as used
// by the host (clang then exports the table and loads its address through the GOT). Either would change the code objects of
// the digest kernels. __host__ __device__ callers (witness_gf5.h) reach them in both passes.
#if defined(__HIP_DEVICE_COMPILE__)
#define GL5D __device__ __forceinline__
#define GL5N __device__ __noinline__
#else
#define GL5D __host__ __device__ __forceinline__
#define GL5N __host__ __device__ inline
#endif
struct gl5 { u64 c[5]; };

GL5D gl5 gl5_zero() { gl5 r; for (int i = 0; i < 5; i++) r.c[i] = 0; return r; }
GL5D gl5 gl5_from(u64 a) { gl5 r = gl5_zero(); r.c[0] = a; return r; }
GL5D gl5 gl5_make(u64 a, u64 b, u64 c, u64 d, u64 e) { gl5 r; r.c[0] = a; r.c[1] = b; r.c[2] = c; r.c[3] = d; r.c[4] = e; return r; }
GL5D bool gl5_is_zero(const gl5& a) { return (a.c[0] | a.c[1] | a.c[2] | a.c[3] | a.c[4]) == 0; }
GL5D bool gl5_eq(const gl5& a, const gl5& b) {
  bool e = true;
#pragma unroll
  for (int i = 0; i < 5; i++) e = e && a.c[i] == b.c[i];
  return e;
}
GL5D gl5 gl5_add(const gl5& a, const gl5& b) { gl5 r;
#pragma unroll
  for (int i = 0; i < 5; i++) r.c[i] = gl_add(a.c[i], b.c[i]);
  return r; }
GL5D gl5 gl5_sub(const gl5& a, const gl5& b) { gl5 r;
#pragma unroll
  for (int i = 0; i < 5; i++) r.c[i] = gl_sub(a.c[i], b.c[i]);
  return r; }
GL5D gl5 gl5_neg(const gl5& a) { gl5 r;
#pragma unroll
  for (int i = 0; i < 5; i++) r.c[i] = gl_neg(a.c[i]);
  return r; }
GL5D gl5 gl5_dbl(const gl5& a) { return gl5_add(a, a); }
GL5D gl5 gl5_scale(const gl5& a, u64 s) { gl5 r;
#pragma unroll
  for (int i = 0; i < 5; i++) r.c[i] = gl_mul(a.c[i], s);
  return r; }
GL5D gl5 gl5_small(const gl5& a, u32 s) { gl5 r;
#pragma unroll
  for (int i = 0; i < 5; i++) r.c[i] = gl_mul_small(a.c[i], s);
  return r; }
// a * (k z): coefficients rotate, the wrapped one picks up z^5 = 3
GL5D gl5 gl5_mul_kz(const gl5& a, u32 k) {
  gl5 r;
  r.c[0] = gl_mul_small(a.c[4], 3 * k);
#pragma unroll
  for (int i = 1; i < 5; i++) r.c[i] = gl_mul_small(a.c[i - 1], k);
  return r;
}
// The one out-of-line body of a GF(p^5) product takes its ten limbs as scalars: clang's AMDGPU ABI keeps at most 16 dwords of
// aggregate arguments in registers and sends the rest through the stack, scalars all travel in VGPRs. (With both operands by
// reference every 600-instruction multiplication began with six flat loads from the stack, and row_digest_kernel sat parked for
// 43 % of its cycles -- tools/dbg/step_pmc.sh.)
GL5N gl5 gl5_mul_limbs(u64 x0, u64 x1, u64 x2, u64 x3, u64 x4, u64 y0, u64 y1, u64 y2, u64 y3, u64 y4) {
  const u64 a[5] = {x0, x1, x2, x3, x4}, b[5] = {y0, y1, y2, y3, y4};
  u64 a3[5];
#pragma unroll
  for (int j = 1; j < 5; j++) a3[j] = gl_mul_small_w(a[j], 3);  // only ever a multiplicand: a weak representative will do
  a3[0] = 0;
  gl5 r;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    gl_cols acc;  // five partial products per output limb in carry-free columns, one reduction
#pragma unroll
    for (int j = 0; j < 5; j++) {
      if (j <= i) acc.add(a[j], b[i - j]); else acc.add(a3[j], b[i + 5 - j]);
    }
    r.c[i] = acc.value();
  }
  return r;
}
GL5D gl5 gl5_mul(const gl5& a, const gl5& b) {
  return gl5_mul_limbs(a.c[0], a.c[1], a.c[2], a.c[3], a.c[4], b.c[0], b.c[1], b.c[2], b.c[3], b.c[4]);
}
// a^2 with the symmetry used: 15 products a_j a_k (j <= k) instead of 25 -- each enters output limb (j + k) mod 5 with the factor
// (2 if j < k) * (3 if j + k >= 5, z^5 = 3) folded into the column accumulation. Squarings are over half of the multiset digest's
// GF(p^5) operations (63 per square root, 5 of the 9 products of a point doubling).
GL5N gl5 gl5_sqr_limbs(u64 x0, u64 x1, u64 x2, u64 x3, u64 x4) {
  const u64 a[5] = {x0, x1, x2, x3, x4};
  gl5 r;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    gl_cols acc;
#pragma unroll
    for (int j = 0; j < 5; j++) {
#pragma unroll
      for (int k = j; k < 5; k++) {
        if ((j + k) % 5 != i) continue;
        const u32 f = (j < k ? 2u : 1u) * (j + k >= 5 ? 3u : 1u);
        if (f == 1) acc.add(a[j], a[k]); else acc.add_scaled(a[j], a[k], f);
      }
    }
    r.c[i] = acc.value();
  }
  return r;
}
GL5D gl5 gl5_sqr(const gl5& a) { return gl5_sqr_limbs(a.c[0], a.c[1], a.c[2], a.c[3], a.c[4]); }
// Frobenius powers: coefficient i times (3^((p-1)/5))^(i*e)
GL5D gl5 gl5_frob1(const gl5& a) {
  return gl5_make(a.c[0], gl_mul(a.c[1], 1041288259238279555ULL), gl_mul(a.c[2], 15820824984080659046ULL),
                  gl_mul(a.c[3], 211587555138949697ULL), gl_mul(a.c[4], 1373043270956696022ULL));
}
GL5D gl5 gl5_frob2(const gl5& a) {
  return gl5_make(a.c[0], gl_mul(a.c[1], 15820824984080659046ULL), gl_mul(a.c[2], 1373043270956696022ULL),
                  gl_mul(a.c[3], 1041288259238279555ULL), gl_mul(a.c[4], 211587555138949697ULL));
}
GL5D u64 gl_sqn(u64 x, int k) {
#pragma unroll 1
  for (int i = 0; i < k; i++) x = gl_sqr(x);
  return x;
}
// o31 = a^(2^31-1), o32 = a^(2^32-1) by an addition chain on runs of ones
GL5D void gl_ones(u64 a, u64& o31, u64& o32) {
  u64 x2 = gl_mul(gl_sqr(a), a), x4 = gl_mul(gl_sqn(x2, 2), x2), x8 = gl_mul(gl_sqn(x4, 4), x4);
  u64 x16 = gl_mul(gl_sqn(x8, 8), x8), x24 = gl_mul(gl_sqn(x16, 8), x8), x28 = gl_mul(gl_sqn(x24, 4), x4);
  u64 x30 = gl_mul(gl_sqn(x28, 2), x2);
  o31 = gl_mul(gl_sqr(x30), a);
  o32 = gl_mul(gl_sqr(o31), a);
}
GL5D u64 gl_pow_2_32_m1(u64 a) { u64 o31, o32; gl_ones(a, o31, o32); return o32; }
// a^(p-2), p-2 = (2^32-2)*2^32 + (2^32-1); 0 -> 0
GL5D u64 gl_inv_chain(u64 a) {
  u64 o31, o32;
  gl_ones(a, o31, o32);
  return gl_mul(gl_sqn(gl_sqr(o31), 32), o32);
}
GL5N gl5 gl5_inv(gl5 a) {  // inverse_or_zero
  gl5 f1 = gl5_frob1(a), f2 = gl5_frob2(a);
  gl5 f12 = gl5_mul(f1, f2);           // a^(p+p^2)
  gl5 f34 = gl5_frob2(f12);            // a^(p^3+p^4)
  gl5 q = gl5_mul(f12, f34);           // a^(r-1)
  u64 n = 0;                           // norm = (a*q)[0]
  {
    gl_cols acc;
    acc.add(a.c[0], q.c[0]);
#pragma unroll
    for (int j = 1; j < 5; j++) acc.add(gl_mul_small_w(a.c[j], 3), q.c[5 - j]);
    n = acc.value();
  }
  return gl5_scale(q, gl_inv_chain(n));
}
GL5D u64 gl5_norm(const gl5& a) {
  gl5 f12 = gl5_mul(gl5_frob1(a), gl5_frob2(a));
  gl5 q = gl5_mul(f12, gl5_frob2(f12));
  return gl5_mul(a, q).c[0];
}
// Legendre symbol of a base-field element as a bool "is a non-zero square or zero"
GL5D bool gl_is_square(u64 a) {
  if (a == 0) return true;
  u64 t = gl_pow_2_32_m1(a);  // a^(2^32-1); a^((p-1)/2) = t^(2^31)
#pragma unroll 1
  for (int i = 0; i < 31; i++) t = gl_sqr(t);
  return t == 1;
}
// g2^(2^k) for the power-of-two generator g2: the device reads the table GL_TWO_GEN_POW2 (perm_constants.h) from constant memory,
// named in gl_sqrt's own body (through an inline function the table would be laid out elsewhere in the code object); host code
// squares, since a unit's host pass may hold only the device table
#if defined(__HIP_DEVICE_COMPILE__)
#define GL_TWO_GEN_POW2_AT(k) GL_TWO_GEN_POW2[k]
#else
inline u64 gl_two_gen_pow2_host(u32 k) {
  u64 g = GL_TWO_GEN;
  for (u32 i = 0; i < k; i++) g = gl_sqr(g);
  return g;
}
#define GL_TWO_GEN_POW2_AT(k) gl_two_gen_pow2_host(k)
#endif
// Tonelli-Shanks, p - 1 = 2^32 (2^32 - 1); c-table GL_TWO_GEN_POW2_AT(k) = g2^(2^k)
GL5N bool gl_sqrt(u64 a, u64& out) {
  if (a == 0) { out = 0; return true; }
  u64 t = gl_pow_2_32_m1(a);  // a^q
  u64 chk = t;
#pragma unroll 1
  for (int i = 0; i < 31; i++) chk = gl_sqr(chk);
  if (chk != 1) { out = 0; return false; }
  u64 R = a;  // a^((q+1)/2) = a^(2^31)
#pragma unroll 1
  for (int i = 0; i < 31; i++) R = gl_sqr(R);
#pragma unroll 1
  while (t != 1) {
    u32 i = 0;
    u64 t2 = t;
    while (t2 != 1) { t2 = gl_sqr(t2); i++; }
    // c has order 2^M; b = c^(2^(M-i-1)) = g2^(2^(31-i)); new c = b^2
    u64 b = GL_TWO_GEN_POW2_AT(31 - i);
    t = gl_mul(t, GL_TWO_GEN_POW2_AT(32 - i));
    R = gl_mul(R, b);
  }
  out = R;
  return true;
}
GL5N bool gl5_sqrt(gl5 x, gl5& out) {
  gl5 v = x;
#pragma unroll 1
  for (int i = 0; i < 31; i++) v = gl5_sqr(v);
  gl5 v32 = v;
#pragma unroll 1
  for (int i = 0; i < 32; i++) v32 = gl5_sqr(v32);
  gl5 d = gl5_mul(gl5_mul(x, v32), gl5_inv(v));       // x^((p+1)/2)
  gl5 e = gl5_frob1(gl5_mul(d, gl5_frob2(d)));        // x^((r-1)/2)
  gl5 f = gl5_sqr(e);
  u64 g = gl5_mul(x, f).c[0];                         // x^r
  u64 s;
  if (!gl_sqrt(g, s)) { out = gl5_zero(); return false; }
  out = gl5_scale(gl5_inv(e), s);
  return true;
}
GL5N bool gl5_is_square(const gl5& x) { return gl_is_square(gl5_norm(x)); }
GL5D bool gl5_sgn0(const gl5& x) {
  bool sign = false, zero = true;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    bool sign_i = (x.c[i] & 1) != 0, zero_i = x.c[i] == 0;
    sign = sign || (zero && sign_i);
    zero = zero && zero_i;
  }
  return sign;
}
}  // namespace mp2g
