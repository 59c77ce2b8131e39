// Goldilocks field arithmetic for gfx950 device code: p = 2^64 - 2^32 + 1, quadratic extension
// X^2 = 7 (FRI challenges / openings), quintic extension z^5 = 3 (Ecgfp5 base field).
// Replaces [dep] plonky2_field (goldilocks_field.rs, extension/{quadratic,quintic}.rs) on the path
// entered at recursion-framework/src/circuit_builder.rs:308.
// Every value is canonical (< p) on entry and exit, so results compare bit-for-bit with the
// CPU side of the reference.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;

#define GL_P 0xFFFFFFFF00000001ULL
#define GL_EPS 0xFFFFFFFFULL
// plonky2 goldilocks_field.rs MULTIPLICATIVE_GROUP_GENERATOR / POWER_OF_TWO_GENERATOR
#define GL_MULT_GEN 14293326489335486720ULL
#define GL_TWO_GEN 7277203076849721926ULL

#define GLD __device__ __forceinline__
#define GLHD __host__ __device__ __forceinline__

// What the operations cost on gfx950, in issue slots of a plain 32-bit add (tools/ubench; single-instruction streams measured in
// round 6, profiles/r06/ubench.txt): register move 0.79 (rounds 2-5 had inferred ~0.4 from A/B residuals), any 32-bit VALU operation
// 0.85, v_cndmask with an SGPR condition 1.5, 64-bit add WITHOUT carry-out (v_lshl_add_u64) 1.5-1.6, v_mad_u64_u32 1.7, a carry-chain
// instruction inside an asm chain 1.2, an add_co / addc pair with the hazard nop hipcc puts between them 4.4, a compare ~2.5, a 64-bit
// compare + select + add 6.2. A move is not free in context either: a word that has to enter a 64-bit addend slot costs two moves and
// the 64-bit add, and where it can enter as the multiplicand of a v_mad_u64_u32 by one instead (read in place from any register, odd or
// even) the permutation gains -- 55 moves and 28 adds a round of Poseidon2's internal layer for 31 such multiply-adds, +2.7 %
// (profiles/p2_carry; alone in a stream the two forms cost the same, 1.54 against 1.59 slots). Hence the rules below: a carry (or borrow)
// is taken from an add_co / addc pair or from the multiply-add's own carry-out only where the value really can wrap; every
// correction that provably cannot wrap is a carry-less 64-bit add of a mask; sums of products go through carry-free columns
// (gl_cols) or ride in the addend slots of the multiply-adds (gl_mul_add_wide); compares are avoided altogether.
GLHD u64 gl_mk(u32 lo, u32 hi) { return ((u64)hi << 32) | lo; }
// a in [0, 2^64) -> canonical: a >= p  <=>  a + EPS carries out of 64 bits
GLHD u64 gl_canon(u64 a) {
  u32 c0, c1;
  u32 t0 = __builtin_addc((u32)a, 0xFFFFFFFFu, 0u, &c0);
  u32 t1 = __builtin_addc((u32)(a >> 32), 0u, c0, &c1);
  return c1 ? gl_mk(t0, t1) : a;
}
GLHD u64 gl_add(u64 a, u64 b) {  // canonical in, canonical out
  u32 c0, c1, d0, d1;
  u32 s0 = __builtin_addc((u32)a, (u32)b, 0u, &c0);
  u32 s1 = __builtin_addc((u32)(a >> 32), (u32)(b >> 32), c0, &c1);
  u32 t0 = __builtin_addc(s0, 0xFFFFFFFFu, 0u, &d0);  // s + EPS = s - p (mod 2^64)
  u32 t1 = __builtin_addc(s1, 0u, d0, &d1);
  return (c1 | d1) ? gl_mk(t0, t1) : gl_mk(s0, s1);
}
GLHD u64 gl_sub(u64 a, u64 b) {  // canonical in, canonical out
  u32 c0, c1, d0, d1;
  u32 s0 = __builtin_subc((u32)a, (u32)b, 0u, &c0);
  u32 s1 = __builtin_subc((u32)(a >> 32), (u32)(b >> 32), c0, &c1);
  u32 m = c1 ? 0xFFFFFFFFu : 0u;  // borrow: + p = - EPS (mod 2^64)
  u32 t0 = __builtin_subc(s0, m, 0u, &d0);
  u32 t1 = __builtin_subc(s1, 0u, d0, &d1);
  return gl_mk(t0, t1);
}
GLHD u64 gl_neg(u64 a) { return a ? GL_P - a : 0; }
GLHD u64 gl_dbl(u64 a) { return gl_add(a, a); }

// ---- weak representatives ---------------------------------------------------------------------
// Inside the hot loops a field element may be ANY u64 congruent to it (not necessarily < p);
// canonicalisation is paid once where a value leaves the kernel. Each routine states its needs.
// a: any u64, b: canonical. (a + b wraps to < p - 1, so the +EPS fix-up cannot wrap again.)
GLHD u64 gl_addw(u64 a, u64 b) {
  u32 c0, c1;
  u32 s0 = __builtin_addc((u32)a, (u32)b, 0u, &c0);
  u32 s1 = __builtin_addc((u32)(a >> 32), (u32)(b >> 32), c0, &c1);
#if defined(__HIP_DEVICE_COMPILE__)
  return gl_mk(s0, s1) + (u64)(c1 ? 0xFFFFFFFFu : 0u);
#else
  u32 m = c1 ? 0xFFFFFFFFu : 0u, d0, d1;
  u32 t0 = __builtin_addc(s0, m, 0u, &d0);
  u32 t1 = __builtin_addc(s1, 0u, d0, &d1);
  return gl_mk(t0, t1);
#endif
}
// hi*2^64 + lo -> some u64 congruent to it (2^64 = EPS, 2^96 = -1 mod p); any lo, hi.
// With hi = hh 2^32 + hl: x = lo + hl EPS - hh. Device code spells the sequence out: one
// v_mad_u64_u32 forms t = hl EPS + lo and hands its carry c over in an SGPR pair, the subtract chain
// leaves the borrow b of t - hh in vcc, and r = t - hh + (c - b) EPS (mod 2^64) is exact:
//   c = 1, b = 0: t <= 2^64 - 2^33, so + EPS cannot wrap;  c = 0, b = 1: t - hh + 2^64 >= 2^64 - 2^32 + 1, so
//   - EPS cannot wrap;  c = b: the two corrections cancel mod 2^64.
// What the compiler makes of the portable form below re-derives carry and borrow with two v_cmp_*_u64
// (~4 issue slots each): 23 % slower per reduction, 12 % per multiply (tools/ubench, profiles/r01/ubench_alu.txt).
GLHD u64 gl_reduce128w(u64 lo, u64 hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  u32 hl = (u32)hi, hh = (u32)(hi >> 32);
  u64 t, c;
  asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=&v"(t), "=s"(c) : "v"(hl), "v"(lo));
  u32 t0 = (u32)t, t1 = (u32)(t >> 32), r0, r1, mb, mc;
  // both corrections as ONE signed 64-bit addend K = (c - b) EPS, added with a carry-less 64-bit add (v_lshl_add_u64): three
  // carry-chain instructions instead of seven. K = [mc - mb, mb & ~mc] for the masks mc = -c, mb = -b.
  // Hazard discipline (gfx90a+: a VALU-written SGPR / VCC needs 2 wait states before another VALU reads it
  // as an explicit operand; the compiler cannot see inside asm): VCC is only consumed through the implicit
  // carry-in of VOP2 forms, the borrow mask is made by u0 - u0 - borrow, and the mad's carry pair %7 is
  // first read three VALU instructions into this block.
  asm("v_sub_co_u32 %0, vcc, %4, %6\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %5, vcc\n\t"
      "v_subb_co_u32 %2, vcc, %0, %0, vcc\n\t"
      "v_cndmask_b32 %3, 0, -1, %7"
      : "=&v"(r0), "=&v"(r1), "=&v"(mb), "=&v"(mc)
      : "v"(t0), "v"(t1), "v"(hh), "s"(c)
      : "vcc");
  return gl_mk(r0, r1) + gl_mk(mc - mb, mb & ~mc);
#else
  u64 hi_hi = hi >> 32, hi_lo = hi & GL_EPS;
  u64 t0;
  bool b = __builtin_sub_overflow(lo, hi_hi, &t0);  // borrow => t0 >= 2^64 - 2^32 + 1, so -EPS cannot borrow again
  t0 -= b ? GL_EPS : 0;
  u64 t1 = (hi_lo << 32) - hi_lo;                   // hi_lo * EPS <= 2^64 - 2^33 + 1
  u64 r;
  bool c = __builtin_add_overflow(t0, t1, &r);      // carry => r <= 2^64 - 2^33, so +EPS cannot carry again
  return r + (c ? GL_EPS : 0);
#endif
}
// hi*2^64 + lo with hi < 2^32
GLHD u64 gl_reduce96w(u64 lo, u64 hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  u64 t, c;
  asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=&v"(t), "=s"(c) : "v"((u32)hi), "v"(lo));
  u32 m;
  asm("s_nop 1\n\t"  // 2 wait states between the mad's SGPR carry and its first VALU reader
      "v_cndmask_b32 %0, 0, -1, %1" : "=v"(m) : "s"(c));
  return t + (u64)m;  // + c EPS cannot wrap (see gl_reduce128w): a carry-less 64-bit add
#else
  u64 t1 = (hi << 32) - hi;
  u64 r;
  bool c = __builtin_add_overflow(lo, t1, &r);
  return r + (c ? GL_EPS : 0);
#endif
}
GLHD u64 gl_reduce128(u64 lo, u64 hi) { return gl_canon(gl_reduce128w(lo, hi)); }
GLHD void gl_mul_wide(u64 a, u64 b, u64& lo, u64& hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  // four 32x32->64 products; hipcc lowers the accumulations to v_mad_u64_u32
  u64 a0 = (u32)a, a1 = a >> 32, b0 = (u32)b, b1 = b >> 32;
  u64 p00 = a0 * b0;
  u64 m1 = a0 * b1 + (p00 >> 32);
  u64 m2 = a1 * b0 + (m1 & GL_EPS);
  lo = (m2 << 32) | (p00 & GL_EPS);
  hi = a1 * b1 + (m1 >> 32) + (m2 >> 32);
#else
  unsigned __int128 x = (unsigned __int128)a * b;
  lo = (u64)x;
  hi = (u64)(x >> 64);
#endif
}
// a * b + c as a 128-bit integer (any u64 a, b, c; the sum is below 2^128): the halves of c ride in the addend slots of the first two
// multiply-adds -- [c_lo, 0] where gl_mul_wide adds nothing, c_hi with the carry word of the first product (a0 b1 + 2^33 - 2 still
// fits 64 bits) -- so the addition costs no carry chain at all
GLHD void gl_mul_add_wide(u64 a, u64 b, u64 c, u64& lo, u64& hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  u64 a0 = (u32)a, a1 = a >> 32, b0 = (u32)b, b1 = b >> 32;
  u64 p00 = a0 * b0 + (u64)(u32)c;
  u64 m1 = a0 * b1 + ((p00 >> 32) + (c >> 32));
  u64 m2 = a1 * b0 + (m1 & GL_EPS);
  lo = (m2 << 32) | (p00 & GL_EPS);
  hi = a1 * b1 + (m1 >> 32) + (m2 >> 32);
#else
  unsigned __int128 x = (unsigned __int128)a * b + c;
  lo = (u64)x;
  hi = (u64)(x >> 64);
#endif
}
GLHD u64 gl_mul(u64 a, u64 b) {
  u64 lo, hi;
  gl_mul_wide(a, b, lo, hi);
  return gl_reduce128(lo, hi);
}
GLHD u64 gl_sqr(u64 a) { return gl_mul(a, a); }
// a * c for a small constant c < 2^32 (MDS / M4 rows, W=7, W=3, 263)
GLHD u64 gl_mul_small(u64 a, u32 c) {
  u64 p0 = (u64)(u32)a * c;
  u64 p1 = (a >> 32) * c + (p0 >> 32);
  return gl_canon(gl_reduce96w((p1 << 32) | (p0 & GL_EPS), p1 >> 32));
}
// the same for any u64 a, as some u64 representative (no canonicalisation)
GLHD u64 gl_mul_small_w(u64 a, u32 c) {
  u64 p0 = (u64)(u32)a * c;
  u64 p1 = (a >> 32) * c + (p0 >> 32);
  return gl_reduce96w((p1 << 32) | (p0 & GL_EPS), p1 >> 32);
}
GLHD u64 gl_pow7(u64 x) {
  u64 x2 = gl_sqr(x), x4 = gl_sqr(x2), x3 = gl_mul(x, x2);
  return gl_mul(x3, x4);
}
GLHD u64 gl_pow(u64 b, u64 e) {
  u64 r = 1;
  while (e) {
    if (e & 1) r = gl_mul(r, b);
    b = gl_sqr(b);
    e >>= 1;
  }
  return r;
}
GLHD u64 gl_inv(u64 a) { return gl_pow(a, GL_P - 2); }
GLHD u64 gl_root_of_unity(unsigned k) {
  u64 g = GL_TWO_GEN;
  for (unsigned i = k; i < 32; i++) g = gl_sqr(g);
  return g;
}
GLHD u32 bitrev32(u32 x, unsigned bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return bits ? (__brev(x) >> (32 - bits)) : 0;
#else
  u32 r = 0;
  for (unsigned i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
  return r;
#endif
}

// a * b + c as some u64 representative (any u64 a, b, c)
GLHD u64 gl_mul_addw(u64 a, u64 b, u64 c) {
  u64 lo, hi;
  gl_mul_add_wide(a, b, c, lo, hi);
  return gl_reduce128w(lo, hi);
}
GLHD u64 gl_mul_add(u64 a, u64 b, u64 c) { return gl_canon(gl_mul_addw(a, b, c)); }  // canonical a b + c, any u64 inputs
// a * d + c as some u64 representative for a CONSTANT d whose fold e = d 2^32 mod p is known when the library is built: with
// a = a0 + 2^32 a1 the integer X = a0 d + a1 e + c is congruent to a d + c and has 97 bits at most, not 128, so the tail is
// gl_reduce96w (one multiply-add, one select, one carry-less add) where gl_mul_addw pays gl_reduce128w with its subtract chain: 16.2
// (narrow; 15.4 re-associated, below) and 18.7 (any pair) against 23.7 issue slots (tools/ubench, profiles/p2_diag). a, c: any u64;
// d, e: canonical and wave-uniform (they are read from SGPRs), e = d 2^32 (mod p). Write d = d0 + 2^32 d1, e = e0 + 2^32 e1, c = c0 + 2^32 c1, M = 2^32 - 1:
//   p0 = a0 d0 + c0               <= M^2 + M         = 2^64 - 2^32
//   p1 = a0 d1 + (p0 >> 32) + c1  <= M d1 + 2 M      <= 2^64 - 1                a0 d + c = lo32(p0) + 2^32 p1
//   q0 = a1 e0 + lo32(p0)         <= M^2 + M         = 2^64 - 2^32
//   q1 = a1 e1 + p1 + (q0 >> 32)  <= M (d1 + e1) + 3 M                          X = lo32(q0) + 2^32 q1
// The halves of c ride in the addend slots as in gl_mul_add_wide, p1 as a whole in q1's: the 64-bit addend p1 + (q0 >> 32) cannot wrap
// (d1 <= M - 1 bounds it by M^2 + 2 M = 2^64 - 1; a canonical d with d1 = M has d0 = 0, hence p0 >> 32 = 0 and the same bound). Only q1
// can exceed 64 bits, and how far is a property of the pair:
//   NARROW, d1 + e1 <= 2^32 - 3 (GL_MULC_NARROW): q1 <= M (M - 2) + 3 M = 2^64 - 2^32. Nothing wraps and no carry is taken.
//   any canonical pair: q1 <= 2 M^2 + 3 M = 2^65 - 2^32 - 1. The multiply-add hands its carry k over in an SGPR pair; k has weight 2^96 in
//     X, and since 2^32 p k = 0 (mod p), X = lo32(q0) + 2^32 (q1 - k p): the 64-bit register, which holds q1 - k 2^64, takes + k EPS
//     (2^64 - p = EPS). With k = 1 it holds at most 2^64 - 2^32 - 1, so the carry-less add of the mask cannot wrap, for every input. The
//     correction is an addition: folding 2^96 = -1 into the result instead would wrap at X = 2^96, which operands do reach.
// Either way X = lo32(q0) + 2^32 lo32(q1) + 2^64 (q1 >> 32) (mod p) with a top word below 2^32, which is what gl_reduce96w takes for any
// lo. Hazards as in gl_reduce128w: the carry pair is read by one v_cndmask two wait states after the multiply-add that wrote it.
#define GL_MULC_NARROW(d, e) (((d) >> 32) + ((e) >> 32) <= 0xFFFFFFFDULL)
// The multiply-adds are spelled out and kept in program order (asm volatile; those that cannot carry name VCC as the carry
// they do not use): left to the compiler the last one loses its addend to a separate 64-bit add and the products of neighbouring
// limbs interleave, which costs 10-20 VGPRs in the sponge kernels (an occupancy step) and 2 % of the permutation.
// The NARROW form is re-associated: the same integer columns, but each product's carry word (the odd register of its pair) enters the
// next column as the MULTIPLICAND of a multiply-add by one, which reads a 32-bit word from any register, where the order above has it
// moved into an aligned (word, 0) pair and added with a 64-bit add. The addends that remain are [c0, 0] and [c1, 0], which all twelve
// limbs of the internal layer share, and [lo32(p0), 0]:
//   p0 = a0 d0 + c0               <= M^2 + M         = 2^64 - 2^32          q0 = a1 e0 + lo32(p0)   <= M^2 + M
//   p1 = a0 d1 + c1               <= M d1 + M                               q1 = a1 e1 + t          <= M (d1 + e1) + 2 M
//   t  = (p0 >> 32) 1 + p1        <= M d1 + 2 M      <= 2^64 - 1            u  = (q0 >> 32) 1 + q1  <= M (d1 + e1) + 3 M <= 2^64 - 2^32
// t is the p1 of the table above and u its q1, so their bounds carry over: nothing wraps, X = lo32(q0) + 2^32 u. Six multiply-adds,
// no 64-bit add and two moves fewer a product than the order above: 15.4 against 16.6 issue slots, the permutation 3.20 -> 3.26
// G perm/s (tools/ubench, profiles/p2_carry). The pairs that take the carry (limbs 0, 8 and 9) keep the order above.
template <bool NARROW>
GLHD u64 gl_mulc_addw(u64 a, u64 d, u64 e, u64 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  const u32 a0 = (u32)a, a1 = (u32)(a >> 32);
  u64 p0, p1, q0, q1;
#define GL_MAD_(r, x, y, z) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=&v"(r) : "v"(x), "s"((u32)(y)), "v"((u64)(z)) : "vcc")
  if (NARROW) {
#define GL_MAD1_(r, w, z) asm volatile("v_mad_u64_u32 %0, vcc, %1, 1, %2" : "=&v"(r) : "v"((u32)(w)), "v"((u64)(z)) : "vcc")
    u64 t, u;
    GL_MAD_(p0, a0, d, (u64)(u32)c);
    GL_MAD_(p1, a0, d >> 32, c >> 32);
    GL_MAD1_(t, p0 >> 32, p1);
    GL_MAD_(q0, a1, e, p0 & GL_EPS);
    GL_MAD_(q1, a1, e >> 32, t);
    GL_MAD1_(u, q0 >> 32, q1);
#undef GL_MAD1_
    return gl_reduce96w(gl_mk((u32)q0, (u32)u), u >> 32);
  }
  u64 k;
  GL_MAD_(p0, a0, d, (u64)(u32)c);
  GL_MAD_(p1, a0, d >> 32, (p0 >> 32) + (c >> 32));
  GL_MAD_(q0, a1, e, p0 & GL_EPS);
#undef GL_MAD_
  asm volatile("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=&v"(q1), "=s"(k) : "v"(a1), "s"((u32)(e >> 32)), "v"(p1 + (q0 >> 32)));
  u32 m;
  asm("s_nop 1\n\t"  // 2 wait states between the mad's SGPR carry and its first VALU reader
      "v_cndmask_b32 %0, 0, -1, %1" : "=v"(m) : "s"(k));
  q1 += (u64)m;
  return gl_reduce96w(gl_mk((u32)q0, (u32)q1), q1 >> 32);
#else
  (void)e;  // the host path is not the target
  return gl_mul_addw(a, d, c);
#endif
}
GLHD u64 gl_mulw(u64 a, u64 b) {
  u64 lo, hi;
  gl_mul_wide(a, b, lo, hi);
  return gl_reduce128w(lo, hi);
}
// gl_mulw for the S-boxes of the permutations (poseidon.cuh): the same 128-bit product, hence the same result for every input, with the
// four multiply-adds spelled out. The two middle products share ONE accumulator, and the bit it can carry past 64 is the third
// multiply-add's own carry-out. With a = a0 + 2^32 a1, b = b0 + 2^32 b1, M = 2^32 - 1:
//   P  = a0 b0                     <= M^2             = 2^64 - 2^33 + 1
//   m1 = a0 b1 + (P >> 32)         <= M^2 + M - 1     = 2^64 - 2^32 - 1         (P >> 32 <= M - 1): fits 64 bits
//   m2 = a1 b0 + m1 = q + 2^64 k   <= 2 M^2 + M - 1   < 2^65: k is 0 or 1, the carry that the multiply-add hands over in an SGPR pair
//   hi = a1 b1 + [q >> 32, k]      <= M^2 + 2 M - 1   = 2^64 - 2: the exact high word of a b <= (2^64 - 1)^2, so it cannot wrap
//   lo = [lo32(P), lo32(q)]
// m1 enters the third multiply-add as the whole register pair it was written to, and [q >> 32, k] pairs a word with the 0 / 1 that one
// v_cndmask makes of the carry: of the addends only P >> 32 is zero-extended. gl_mul_wide, left to hipcc (m2 = a1 b0 + lo32(m1), then
// hi = a1 b1 + (m1 >> 32) + (m2 >> 32)), zero-extends three more words into aligned pairs and joins the two high words in a 64-bit add of
// their own: two moves and one v_lshl_add_u64 a product more, one v_cndmask less (profiles/mul_carry). Hazards as in gl_reduce96w: the
// carry pair is read by the v_cndmask two wait states after the multiply-add that wrote it. The three multiply-adds that cannot carry
// name VCC as the carry they do not use, as in gl_mulc_addw.
// Only p2_sbox0 calls it. In gl_mul_wide itself, in gl_mulw and gl_mul_addw, or in the S-box of the gate evaluators the same form takes a
// wave per SIMD from gate kernels (gate_constraints_lde_kernel<11> 90 -> 107 VGPRs, <18> 74 -> 98, gate_check_kernel 230 -> 260) and, in
// gl_mul_wide, adds scratch to NTT kernels (profiles/mul_carry lists every scope).
GLHD u64 gl_mulw_k(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
  const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
  u64 p, m1, q, hi, k;
  u32 kw;
#define GL_MADV_(r, x, y, z) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=&v"(r) : "v"(x), "v"(y), "v"((u64)(z)) : "vcc")
  asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=&v"(p) : "v"(a0), "v"(b0) : "vcc");
  GL_MADV_(m1, a0, b1, p >> 32);
  asm volatile("v_mad_u64_u32 %0, %1, %3, %4, %5\n\t"
               "s_nop 1\n\t"  // 2 wait states between the mad's SGPR carry and its first VALU reader
               "v_cndmask_b32 %2, 0, 1, %1"
               : "=&v"(q), "=&s"(k), "=&v"(kw) : "v"(a1), "v"(b0), "v"(m1));
  GL_MADV_(hi, a1, b1, gl_mk((u32)(q >> 32), kw));
#undef GL_MADV_
  return gl_reduce128w(gl_mk((u32)p, (u32)q), hi);
#else
  return gl_mulw(a, b);
#endif
}

// ---- sums of products without carry chains ------------------------------------------------------------------------------
// sum_k a_k b_k as four 64-bit columns of 32-bit words: on gfx950 a 64-bit add without carry-out costs 1.6 issue slots, an
// add_co / addc pair with its hazard nop 4.4. Fewer than 2^32 terms, so no column overflows.
struct gl_cols {
  u64 c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  GLHD void add(u64 a, u64 b) {
    u64 pl, ph;
    gl_mul_wide(a, b, pl, ph);
    c0 += (u32)pl; c1 += pl >> 32; c2 += (u32)ph; c3 += ph >> 32;
  }
  // f times the product a b for a small factor f (a symmetric term counted twice, a wrapped term times z^5 = 3: f <= 6): the
  // factor multiplies the 32-bit words on their way into the columns (one multiply-add per column instead of one add)
  GLHD void add_scaled(u64 a, u64 b, u32 f) {
    u64 pl, ph;
    gl_mul_wide(a, b, pl, ph);
    c0 += (u64)(u32)pl * f; c1 += (pl >> 32) * f; c2 += (u64)(u32)ph * f; c3 += (ph >> 32) * f;
  }
  // the sum as a canonical element: lo + hi 2^64 + top 2^128, 2^128 = -2^32 (mod p)
  GLHD u64 value() const {
    const u64 w1 = c1 + (c0 >> 32), w2 = c2 + (w1 >> 32), w3 = c3 + (w2 >> 32);
    return gl_sub(gl_reduce128(gl_mk((u32)c0, (u32)w1), gl_mk((u32)w2, (u32)w3)), (w3 >> 32) << 32);
  }
};

// ---- quadratic extension ------------------------------------------------------------------
struct gl2 { u64 a, b; };
GLHD gl2 gl2_make(u64 a, u64 b) { gl2 r; r.a = a; r.b = b; return r; }
GLHD gl2 gl2_add(gl2 x, gl2 y) { return gl2_make(gl_add(x.a, y.a), gl_add(x.b, y.b)); }
GLHD gl2 gl2_sub(gl2 x, gl2 y) { return gl2_make(gl_sub(x.a, y.a), gl_sub(x.b, y.b)); }
GLHD gl2 gl2_mul(gl2 x, gl2 y) {
  // (a + b X)(c + d X) = ac + 7 bd + (ad + bc) X: the second product of each coefficient rides in the first one's addend slots
  return gl2_make(gl_mul_add(x.a, y.a, gl_mul_small_w(gl_mulw(x.b, y.b), 7)), gl_mul_add(x.a, y.b, gl_mulw(x.b, y.a)));
}
GLHD gl2 gl2_scale(gl2 x, u64 s) { return gl2_make(gl_mul(x.a, s), gl_mul(x.b, s)); }
GLHD gl2 gl2_inv(gl2 x) {
  u64 n = gl_sub(gl_sqr(x.a), gl_mul_small(gl_sqr(x.b), 7));
  u64 ni = gl_inv(n);
  return gl2_make(gl_mul(x.a, ni), gl_mul(gl_neg(x.b), ni));
}
GLHD gl2 gl2_pow(gl2 b, u64 e) {
  gl2 r = gl2_make(1, 0);
  while (e) {
    if (e & 1) r = gl2_mul(r, b);
    b = gl2_mul(b, b);
    e >>= 1;
  }
  return r;
}
