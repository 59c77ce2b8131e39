// Width-12 permutations over Goldilocks for gfx950: Poseidon2 (the reference's default hasher,
// mp2-common/src/lib.rs:37-42) and Poseidon (WrapC, verifiable-db/src/api.rs:148), plus the
// plonky2 sponge conventions restated in-tree at mp2-common/src/hash.rs:24-45 and
// mp2-common/src/poseidon.rs:151-170 (overwrite-mode absorb, rate 8, squeeze from the front).
//
// One lane owns one 12-limb state (24 VGPRs). Round constants sit in __constant__ memory and
// are read with wave-uniform indices, so they arrive through the scalar cache into SGPRs and
// cost no vector registers. Rounds are loops, not unrolled: the external-round body is ~6 KB
// of ISA and stays resident in the instruction cache shared by neighbouring CUs.
#pragma once
#include "gl.cuh"
#include "perm_constants.h"

// What gl_mulc_addw needs beside the diagonal is no table of literals: the compiler derives it here from POSEIDON2_DIAG_M1, the one
// place where the diagonal is written down,
//   POSEIDON2_DIAG_M1_SHL32[i] = d_i 2^32 mod p, in constant memory beside the diagonal and read like it,
//   POSEIDON2_DIAG_NARROW, bit i set: the pair (d_i, d_i 2^32 mod p) is narrow (GL_MULC_NARROW).
// perm_constants.h itself stays what tools/gen_constants.py writes and tests/test_oracle_pins.py pins name by name against the CPU
// checker's header: a thirteenth table of literals there would be one that no second generator vouches for, and that test refuses it.
// To read the diagonal in constant expressions the header is included a second time, on purpose past its include guard, inside a
// namespace with its tables as `static constexpr` (<stdint.h> is in already through gl.cuh, so nothing else lands in the namespace;
// no copy is odr-used, so none reaches the code object). tests/test_p2_diag_constants.py recomputes what comes out.
#pragma push_macro("MP2G_DEVCONST")
#undef MP2G_DEVCONST
#undef MP2G_PERM_CONSTANTS_H
#define MP2G_DEVCONST static constexpr
namespace p2_cx {
#include "perm_constants.h"
constexpr u64 diag_shl32(int i) { return (u64)(((unsigned __int128)POSEIDON2_DIAG_M1[i] << 32) % GL_P); }
constexpr unsigned diag_narrow(int i = 0) {
  return i == 12 ? 0u : (GL_MULC_NARROW(POSEIDON2_DIAG_M1[i], diag_shl32(i)) ? 1u << i : 0u) | diag_narrow(i + 1);
}
}  // namespace p2_cx
#pragma pop_macro("MP2G_DEVCONST")
MP2G_DEVCONST uint64_t POSEIDON2_DIAG_M1_SHL32[12] = {
  p2_cx::diag_shl32(0), p2_cx::diag_shl32(1), p2_cx::diag_shl32(2), p2_cx::diag_shl32(3), p2_cx::diag_shl32(4), p2_cx::diag_shl32(5),
  p2_cx::diag_shl32(6), p2_cx::diag_shl32(7), p2_cx::diag_shl32(8), p2_cx::diag_shl32(9), p2_cx::diag_shl32(10), p2_cx::diag_shl32(11),
};
constexpr unsigned POSEIDON2_DIAG_NARROW = p2_cx::diag_narrow();
static_assert(POSEIDON2_DIAG_NARROW == 0xcfeu, "limbs 0, 8 and 9 take gl_mulc_addw's carry (profiles/p2_diag measured this split)");

#define MP2G_POSEIDON2 0
#define MP2G_POSEIDON 1

#define c_p2_ext POSEIDON2_RC_EXT
#define c_p2_int POSEIDON2_RC_INT
#define c_p2_diag POSEIDON2_DIAG_M1
#define c_p2_diag_shl32 POSEIDON2_DIAG_M1_SHL32
#define c_p_rc POSEIDON_RC

// ---- Poseidon2, weak-representative form ------------------------------------------------------
// State limbs are arbitrary u64 representatives between rounds (gl.cuh "weak"); outputs are
// canonicalised once at the end. Linear layers run on the 32-bit halves of the limbs in plain
// 64-bit arithmetic (all weights are small) and reduce once per output limb.
// x <- (x + rc)^7 ; x any u64, rc canonical. For the gate evaluators and the lane-cooperative permutation: products in the order hipcc
// chooses (gl_mulw_k here costs gate_check_kernel and the Poseidon gate's kernel a wave per SIMD)
GLHD u64 p2_sbox(u64 x, u64 rc) {
  u64 t = gl_addw(x, rc);
  u64 t2 = gl_mulw(t, t), t4 = gl_mulw(t2, t2), t3 = gl_mulw(t, t2);
  return gl_mulw(t3, t4);
}
// M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]] with additions only (HorizenLabs matmul_m4), on
// un-reduced integers: inputs < 2^32 give outputs < 2^37.
GLHD void p2_m4_plain(u64& a, u64& b, u64& c, u64& d) {
  u64 t0 = a + b, t1 = c + d;
  u64 t2 = (b << 1) + t1, t3 = (d << 1) + t0;
  u64 t4 = (t1 << 2) + t3, t5 = (t0 << 2) + t2;
  a = t3 + t5; b = t5; c = t2 + t4; d = t4;
}
GLHD void p2_external_half(u64 v[12]) {
  p2_m4_plain(v[0], v[1], v[2], v[3]);
  p2_m4_plain(v[4], v[5], v[6], v[7]);
  p2_m4_plain(v[8], v[9], v[10], v[11]);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    u64 sum = v[i] + v[4 + i] + v[8 + i];
    v[i] += sum; v[4 + i] += sum; v[8 + i] += sum;  // < 2^39
  }
}
// circ(2 M4, M4, M4) on weak limbs; RC: also add the next round's constants rc[0..12) before the one
// reduction per limb (a carry into the top word instead of a separate weak addition per limb)
template <bool RC>
GLHD void p2_external_rc(u64 s[12], const u64* rc) {
  u64 lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 12; i++) { lo[i] = (u32)s[i]; hi[i] = s[i] >> 32; }
  p2_external_half(lo);
  p2_external_half(hi);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int i = 0; i < 12; i++) {
    // value = lo + hi * 2^32 (+ rc), lo, hi < 2^39: carry-less 64-bit adds of the halves, the high part of the low half moves up
    u64 L = lo[i], H = hi[i];
    if (RC) { L += (u64)(u32)rc[i]; H += rc[i] >> 32; }
    H += L >> 32;  // < 2^41
    s[i] = gl_reduce96w(gl_mk((u32)L, (u32)H), H >> 32);
  }
#else
#pragma unroll
  for (int i = 0; i < 12; i++) {
    // value = lo + hi * 2^32, lo, hi < 2^39
    u32 c0, c1, top = (u32)(hi[i] >> 32);
    u32 l0 = (u32)lo[i];
    u32 l1 = __builtin_addc((u32)(lo[i] >> 32), (u32)hi[i], 0u, &c0);
    top += c0;
    if (RC) {
      const u64 k = rc[i];
      l0 = __builtin_addc(l0, (u32)k, 0u, &c0);
      l1 = __builtin_addc(l1, (u32)(k >> 32), c0, &c1);
      top += c1;
    }
    s[i] = gl_reduce96w(gl_mk(l0, l1), top);
  }
#endif
}
GLHD void p2_external(u64 s[12]) { p2_external_rc<false>(s, nullptr); }
// x^7 for a limb whose round constant is already in (p2_external_rc). The S-box of the sponge, tree and proof-of-work kernels: its four
// products take their middle column's carry from the multiply-add (gl_mulw_k; the permutation 3.09 -> 3.19 G perm/s: profiles/mul_carry)
GLHD u64 p2_sbox0(u64 t) {
  u64 t2 = gl_mulw_k(t, t), t4 = gl_mulw_k(t2, t2), t3 = gl_mulw_k(t, t2);
  return gl_mulw_k(t3, t4);
}
// d_i a + c for limb i of the internal layer's diagonal, as some u64 representative (a, c: any u64; i a constant after unrolling). d_i is
// known when the library is built, so the product takes gl_mulc_addw and its 96-bit tail: without the carry for the nine limbs whose
// pair (d_i, d_i 2^32 mod p) is narrow, with it for limbs 0, 8 and 9 (the permutation 2.83 -> 3.10 G perm/s: profiles/p2_diag)
GLHD u64 p2_diag_mul_addw(int i, u64 a, u64 c) {
  if ((POSEIDON2_DIAG_NARROW >> i) & 1) return gl_mulc_addw<true>(a, c_p2_diag[i], c_p2_diag_shl32[i], c);
  return gl_mulc_addw<false>(a, c_p2_diag[i], c_p2_diag_shl32[i], c);
}
// The sum S of the twelve limbs (any u64 each, so S < 12 2^64 has 68 bits at most) as some u64 representative, without splitting the
// limbs into zero-extended halves. Write s_i = l_i + 2^32 h_i, L = sum l_i, H = sum h_i (both exact, below 12 2^32), so S = L + 2^32 H:
//   W = sum s_i mod 2^64            eleven carry-less 64-bit adds on the limbs' own register pairs
//   H                               twelve multiply-adds by one; as the multiplicand a high word is read in place, from the odd register
//   c = L >> 32 <= 11               the carry of the low words. hi32(W) = (c + lo32(H)) mod 2^32 and c < 2^32, so
//                                   c = (hi32(W) - lo32(H)) mod 2^32 exactly: one 32-bit subtract, which may wrap
//   T = H + c <= 12 M + 11          S = lo32(L) + 2^32 T, and lo32(T) = hi32(W), hence S = W + 2^64 (T >> 32)
// with a top word T >> 32 <= 11, which gl_reduce96w takes. The multiply-adds are spelled out (asm volatile; they name VCC as the carry
// they do not use, as in gl_mulc_addw): a multiplication by one written in C is folded back into two moves and a 64-bit add. Against
// the sum of zero-extended halves (24 moves into aligned pairs, 24 64-bit adds) this is 29.5 moves and 10 adds a round fewer for 13
// multiply-adds more: the permutation 3.26 -> 3.28 G perm/s on top of the re-associated gl_mulc_addw (tools/ubench, profiles/p2_carry).
GLD u64 p2_limb_sum(const u64 s[12]) {
#if defined(__HIP_DEVICE_COMPILE__)
  u64 w = s[0], ha, hb;
#pragma unroll
  for (int i = 1; i < 12; i++) w += s[i];
#define P2_MAD1_(r, x, z) asm volatile("v_mad_u64_u32 %0, vcc, %1, 1, %2" : "=v"(r) : "v"((u32)((x) >> 32)), "v"(z) : "vcc")
  asm volatile("v_mad_u64_u32 %0, vcc, %1, 1, 0" : "=v"(ha) : "v"((u32)(s[0] >> 32)) : "vcc");
  asm volatile("v_mad_u64_u32 %0, vcc, %1, 1, 0" : "=v"(hb) : "v"((u32)(s[1] >> 32)) : "vcc");
#pragma unroll
  for (int i = 2; i < 12; i += 2) {  // two chains
    P2_MAD1_(ha, s[i], ha);
    P2_MAD1_(hb, s[i + 1], hb);
  }
  const u64 h = ha + hb;
  const u32 c = (u32)(w >> 32) - (u32)h;
  u64 t;
  asm volatile("v_mad_u64_u32 %0, vcc, %1, 1, %2" : "=v"(t) : "v"(c), "v"(h) : "vcc");
#undef P2_MAD1_
  return gl_reduce96w(w, t >> 32);
#else
  unsigned __int128 x = 0;  // device code only: the host pass merely has to parse a body
  for (int i = 0; i < 12; i++) x += s[i];
  return gl_reduce96w((u64)x, (u64)(x >> 64));
#endif
}
// s_i <- d_i s_i + sum_j s_j. Device code: sum reduced once, then a weak multiply and a weak add per limb (2.60 -> 2.71 G perm/s against the
// fused form of the host code below -- 128-bit product plus the 68-bit sum, one reduction --, whose carry chains cost more than the second
// reduction saves)
GLHD void p2_internal(u64 s[12]) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the 68-bit sum reduced ONCE to some representative (any will do below); every limb is then weak multiply + weak add
  const u64 sum = p2_limb_sum(s);
#pragma unroll
  for (int i = 0; i < 12; i++) {
    s[i] = p2_diag_mul_addw(i, s[i], sum);  // the sum rides in the product's addend slots
    // one limb after the other: without the fence hipcc zeroes the high words of every limb's addend pairs ahead of time, 10 VGPRs in
    // the sponge and 12-14 in the tree kernels of index_hash.hip (past 128, an occupancy step) for no gain in rate (profiles/p2_diag)
    __builtin_amdgcn_sched_barrier(0);
  }
#else
  u64 acc = s[0];
  u64 top = 0;
#pragma unroll
  for (int i = 1; i < 12; i++) {
    bool c = __builtin_add_overflow(acc, s[i], &acc);
    top += c ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < 12; i++) {
    u64 lo, hi;
    gl_mul_wide(s[i], c_p2_diag[i], lo, hi);  // hi <= 2^64 - 2^32 - 1: adding top + carry cannot wrap
    bool c = __builtin_add_overflow(lo, acc, &lo);
    s[i] = gl_reduce128w(lo, hi + top + (c ? 1 : 0));
  }
#endif
}
GLHD void poseidon2_perm(u64 s[12]) {
  p2_external_rc<true>(s, c_p2_ext);  // the constants of a full round ride on the preceding linear layer
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = p2_sbox0(s[i]);
    if (r < 3) p2_external_rc<true>(s, c_p2_ext + 12 * (r + 1)); else p2_external(s);
  }
  // the 22 internal rounds in two unrolled halves: 2.79 -> 2.84 G perm/s against no unrolling (tools/ubench; 4: 2.82, 22: 2.82)
#pragma unroll 11
  for (int r = 0; r < 22; r++) {
    s[0] = p2_sbox0(gl_addw(s[0], c_p2_int[r]));  // p2_sbox's operations, with p2_sbox0's product
    p2_internal(s);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = gl_addw(s[i], c_p2_ext[48 + i]);  // round 4 follows an internal layer
#pragma unroll 1
  for (int r = 4; r < 8; r++) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = p2_sbox0(s[i]);
    if (r < 7) p2_external_rc<true>(s, c_p2_ext + 12 * (r + 1)); else p2_external(s);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = gl_canon(s[i]);
}

// Poseidon (WrapC), weak-representative form like Poseidon2 above. MDS: circulant
// [17,15,41,16,2,28,13,13,39,18,34,20] + diag [8,0,...]; all entries < 2^6, so the 32-bit halves of the
// limbs accumulate in u64 without overflow (< 2^41) and reduce once per row.
// RC: also add the next round's constants rc[0..12) before the one reduction per limb
template <bool RC>
GLHD void poseidon_mds_rc(u64 s[12], const u64* rc) {
  const u32 circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
  u64 lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 12; i++) { lo[i] = (u32)s[i]; hi[i] = s[i] >> 32; }
  u64 out[12];
#pragma unroll
  for (int r = 0; r < 12; r++) {
    u64 al = 0, ah = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
      al += lo[(i + r) % 12] * circ[i];
      ah += hi[(i + r) % 12] * circ[i];
    }
    if (r == 0) { al += lo[0] * 8; ah += hi[0] * 8; }
    // value = al + ah * 2^32, al, ah < 2^41
    u32 c0, c1, top = (u32)(ah >> 32);
    u32 l0 = (u32)al;
    u32 l1 = __builtin_addc((u32)(al >> 32), (u32)ah, 0u, &c0);
    top += c0;
    if (RC) {
      const u64 k = rc[r];
      l0 = __builtin_addc(l0, (u32)k, 0u, &c0);
      l1 = __builtin_addc(l1, (u32)(k >> 32), c0, &c1);
      top += c1;
    }
    out[r] = gl_reduce96w(gl_mk(l0, l1), top);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = out[i];
}
GLHD void poseidon_mds(u64 s[12]) { poseidon_mds_rc<false>(s, nullptr); }
GLHD void poseidon_perm(u64 s[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = gl_addw(s[i], c_p_rc[i]);
#pragma unroll 1
  for (int r = 0; r < 30; r++) {  // the constants of round r + 1 ride on round r's MDS reduction
    if (r < 4 || r >= 26) {
#pragma unroll
      for (int i = 0; i < 12; i++) s[i] = p2_sbox0(s[i]);
    } else {
      s[0] = p2_sbox0(s[0]);
    }
    if (r < 29) poseidon_mds_rc<true>(s, c_p_rc + 12 * (r + 1)); else poseidon_mds(s);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = gl_canon(s[i]);
}
template <int VARIANT>
GLHD void perm(u64 s[12]) {
  if (VARIANT == MP2G_POSEIDON2) poseidon2_perm(s); else poseidon_perm(s);
}
// compress(l, r) = perm(l || r || 0)[0..4]   (plonky2 hashing.rs)
template <int VARIANT>
GLD void two_to_one(const u64 l[4], const u64 r[4], u64 out[4]) {
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 4; i++) { s[i] = l[i]; s[4 + i] = r[i]; s[8 + i] = 0; }
  perm<VARIANT>(s);
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = s[i];
}
