// The witness tape's wide opcodes (include/mp2g.h enum mp2g_witness_op_wide): ONE definition for the host replay (witness.hip) and
// the device replay (witness_dev.hip). Restates, of mp2-common/src/serialization/circuit_data_serialization.rs:186-231, the
// generators of [dep] plonky2_crypto's bit-interleaving gates (U32InterleaveGenerator, UninterleaveToB32Generator,
// UninterleaveToU32Generator; wire layouts of the gate evaluators, gates.hip / oracle/gates_body.inc), UInt256DivGenerator
// (mp2-common/src/u256.rs:920-952), [dep] plonky2_ecdsa's BigUintDivRemGenerator and PoseidonMdsGenerator. t = the operands after
// the opcode (validated at create: witness_ops.h op_shape, witness.hip), vals = the proof's slot table, put(col, row, value)
// writes a wire. The divisions are plain integer code, one lane per instruction like every other opcode. MP2G_OP_U256_DIV is a
// restoring division, one quotient bit per step, with 8 limbs and compile-time indices, so its operands stay in registers;
// MP2G_OP_BIGUINT_DIV_REM's limb counts are operands, its arrays (3 x 32 words) are addressed at run time and sit in private
// memory, and it divides digit by digit (Knuth D).
#pragma once
#include "gl.cuh"
#include "perm_constants.h"
#include "witness.h"

namespace mp2g {
// bit k of x -> bit 2k
GLHD u64 wide_spread32(u32 x32) {
  u64 x = x32;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}
// bit 2k of x -> bit k (the odd bits are dropped)
GLHD u32 wide_compact32(u64 x) {
  x &= 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
  return (u32)x;
}

// (a, r) <- (a / b, a % b) over 8 limbs, b != 0. The pair (r : a) is shifted left one bit a step, the quotient bits entering a from
// below as the dividend bits leave it above; every index is a compile-time constant.
GLHD void wide_divrem8(u32 (&a)[8], const u32 (&b)[8], u32 (&r)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) r[k] = 0;
#pragma unroll 1
  for (int step = 0; step < 256; step++) {
    const u32 top = r[7] >> 31;  // r < b before the step, so 2 r + bit < 2 b: when the shift carries out, b fits once
#pragma unroll
    for (int k = 7; k > 0; k--) r[k] = (r[k] << 1) | (r[k - 1] >> 31);
    r[0] = (r[0] << 1) | (a[7] >> 31);
#pragma unroll
    for (int k = 7; k > 0; k--) a[k] = (a[k] << 1) | (a[k - 1] >> 31);
    a[0] <<= 1;
    u32 d[8];
    u64 borrow = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const u64 x = (u64)r[k] - b[k] - borrow;
      d[k] = (u32)x;
      borrow = (x >> 32) & 1;
    }
    if (top | (u32)(borrow ^ 1)) {
#pragma unroll
      for (int k = 0; k < 8; k++) r[k] = d[k];
      a[0] |= 1;
    }
  }
}

// q[0 .. na) = u / v, and u[0 .. nb) = u % v, for u of na limbs and v != 0 of nb limbs (run-time counts): Knuth's algorithm D on 32-bit
// digits (TAOCP 4.3.1; the formulation of Hacker's Delight, divmnu). u has na + 1 words (the last one takes the digit the
// normalising shift pushes out), v is normalised in place. The limbs above the operands' highest non-zero ones take no part. One
// quotient digit costs one pass over v, so a 32-by-32-limb division is a few hundred limb steps (a bit-serial loop over arrays in
// private memory would be a hundred thousand). Out of line: inlined into the executor's switch, its live values cost the whole kernel
// 48 more registers and spills (256 VGPRs and 98 spilled against 208 and none).
__host__ __device__ __attribute__((noinline)) inline void wide_divrem(u32* u, u32 na, u32* v, u32 nb, u32* q) {
  u32 m = na, n = nb;
  while (m > 0 && u[m - 1] == 0) m--;
  while (n > 1 && v[n - 1] == 0) n--;
  for (u32 k = 0; k < na; k++) q[k] = 0;
  if (m < n) return;  // u < v: quotient 0, remainder u
  if (n == 1) {       // one digit: short division
    u64 rem = 0;
    for (u32 k = m; k-- > 0;) {
      const u64 cur = (rem << 32) | u[k];
      q[k] = (u32)(cur / v[0]);
      rem = cur % v[0];
      u[k] = 0;
    }
    u[0] = (u32)rem;
    return;
  }
  u32 s = 0;  // the shift that sets the top bit of v's highest digit
  while (((v[n - 1] << s) & 0x80000000u) == 0) s++;
  if (s) {
    for (u32 k = n - 1; k > 0; k--) v[k] = (v[k] << s) | (v[k - 1] >> (32 - s));
    v[0] <<= s;
    u[m] = u[m - 1] >> (32 - s);
    for (u32 k = m - 1; k > 0; k--) u[k] = (u[k] << s) | (u[k - 1] >> (32 - s));
    u[0] <<= s;
  } else {
    u[m] = 0;
  }
  for (u32 j = m - n + 1; j-- > 0;) {
    // the digit's estimate from the two highest digits of what is left of u, corrected with the third (at most twice)
    const u64 num = ((u64)u[j + n] << 32) | u[j + n - 1];
    u64 qhat = num / v[n - 1], rhat = num % v[n - 1];
    while (qhat >> 32 || qhat * v[n - 2] > ((rhat << 32) | u[j + n - 2])) {
      qhat--;
      rhat += v[n - 1];
      if (rhat >> 32) break;
    }
    // u[j .. j + n] -= qhat v
    int64_t k = 0, t;
    for (u32 i = 0; i < n; i++) {
      const u64 p = qhat * v[i];
      t = (int64_t)u[i + j] - k - (int64_t)(p & 0xFFFFFFFFull);
      u[i + j] = (u32)t;
      k = (int64_t)(p >> 32) - (t >> 32);
    }
    t = (int64_t)u[j + n] - k;
    u[j + n] = (u32)t;
    if (t < 0) {  // the estimate was one too large (probability about 2^-31): add v back
      qhat--;
      u64 c = 0;
      for (u32 i = 0; i < n; i++) {
        c += (u64)u[i + j] + v[i];
        u[i + j] = (u32)c;
        c >>= 32;
      }
      u[j + n] += (u32)c;
    }
    q[j] = (u32)qhat;
  }
  // the remainder, shifted back
  if (s) {
    for (u32 k = 0; k + 1 < n; k++) u[k] = (u[k] >> s) | (u[k + 1] << (32 - s));
    u[n - 1] >>= s;
  }
  for (u32 k = n; k <= m; k++) u[k] = 0;
}

// Poseidon's MDS layer on canonical values: circ POSEIDON_MDS_CIRC + diag POSEIDON_MDS_DIAG, entries < 2^6. The 32-bit halves of
// the limbs accumulate in 64 bits (< 2^42), one reduction per output limb.
GLHD void wide_poseidon_mds(const u64 (&s)[12], u64 (&out)[12]) {
#pragma unroll
  for (int r = 0; r < 12; r++) {
    u64 al = (u64)(u32)s[r] * POSEIDON_MDS_DIAG[r], ah = (s[r] >> 32) * POSEIDON_MDS_DIAG[r];
#pragma unroll
    for (int i = 0; i < 12; i++) {
      al += (u64)(u32)s[(i + r) % 12] * POSEIDON_MDS_CIRC[i];
      ah += (s[(i + r) % 12] >> 32) * POSEIDON_MDS_CIRC[i];
    }
    // al + 2^32 ah as a 128-bit integer
    const u64 lo = al + (ah << 32);
    out[r] = gl_reduce128(lo, (ah >> 32) + (lo < al ? 1 : 0));
  }
}

template <class Put>
GLHD bool exec_wide_op(u64 op, const u64* t, u64* vals, Put put) {
  switch (op) {
    case OP_U32_INTERLEAVE: {
      const u64 row = t[0], i = t[1], ops = t[2], x = vals[t[3]];
      const u32 lo = (u32)x;
      const u64 xi = wide_spread32(lo);
      put(2 * i, row, x); put(2 * i + 1, row, xi);
      for (u32 j = 0; j < 32; j++) put(2 * ops + 32 * i + j, row, (lo >> (31 - j)) & 1);
      vals[t[4]] = xi;
      return true;
    }
    case OP_UNINTERLEAVE_TO_B32: case OP_UNINTERLEAVE_TO_U32: {
      const u64 row = t[0], i = t[1], ops = t[2], x = vals[t[3]];
      const bool spread = op == OP_UNINTERLEAVE_TO_B32;
      const u64 ev = spread ? x & 0x5555555555555555ull : wide_compact32(x);
      const u64 od = spread ? (x >> 1) & 0x5555555555555555ull : wide_compact32(x >> 1);
      put(3 * i, row, x); put(3 * i + 1, row, ev); put(3 * i + 2, row, od);
      for (u32 j = 0; j < 64; j++) put(3 * ops + 64 * i + j, row, (x >> (63 - j)) & 1);
      vals[t[4]] = ev; vals[t[5]] = od;
      return true;
    }
    case OP_U256_DIV: {
      u32 a[8], b[8], r[8];
      u32 any = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) { a[k] = (u32)vals[t[k]]; b[k] = (u32)vals[t[8 + k]]; any |= b[k]; }
      if (vals[t[16]] == 0) {
        // is_div false: quotient 1, remainder = dividend - dividend divisor mod 2^256 (the low 8 limbs of the schoolbook product)
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          u64 carry = 0;
#pragma unroll
          for (int j = 0; i + j < 8; j++) {
            const u64 x = (u64)a[j] * b[i] + r[i + j] + carry;
            r[i + j] = (u32)x;
            carry = x >> 32;
          }
        }
        u64 borrow = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const u64 x = (u64)a[k] - r[k] - borrow;
          r[k] = (u32)x;
          borrow = (x >> 32) & 1;
          a[k] = k == 0 ? 1 : 0;
        }
      } else if (any == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) { r[k] = a[k]; a[k] = 0; }
      } else {
        wide_divrem8(a, b, r);
      }
#pragma unroll
      for (int k = 0; k < 8; k++) { vals[t[17 + k]] = a[k]; vals[t[25 + k]] = r[k]; }
      return true;
    }
    case OP_BIGUINT_DIV_REM: {
      const u32 na = (u32)t[0], nb = (u32)t[1];  // 1 .. BIGUINT_MAX_LIMBS each (op_shape)
      const u64* sa = t + 2;
      const u64* sb = sa + na;
      const u64* dq = sb + nb;
      const u64* dr = dq + na;
      u32 a[BIGUINT_MAX_LIMBS + 1], b[BIGUINT_MAX_LIMBS], q[BIGUINT_MAX_LIMBS];
      u32 any = 0;
      for (u32 k = 0; k <= BIGUINT_MAX_LIMBS; k++) a[k] = k < na ? (u32)vals[sa[k]] : 0;
      for (u32 k = 0; k < nb; k++) { b[k] = (u32)vals[sb[k]]; any |= b[k]; }
      if (any == 0) {  // this library's choice (the generator of [dep] plonky2_ecdsa panics): div = 0, rem = a cut to nb limbs
        for (u32 k = 0; k < na; k++) q[k] = 0;
      } else {
        wide_divrem(a, na, b, nb, q);  // the remainder takes a's place
      }
      for (u32 k = 0; k < na; k++) vals[dq[k]] = q[k];
      for (u32 k = 0; k < nb; k++) vals[dr[k]] = a[k];
      return true;
    }
    case OP_POSEIDON_MDS: {
      const u64 row = t[0];
#pragma unroll 1
      for (u32 c = 0; c < 2; c++) {
        u64 s[12], o[12];
#pragma unroll
        for (int i = 0; i < 12; i++) { s[i] = vals[t[1 + 2 * i + c]]; put(2 * i + c, row, s[i]); }
        wide_poseidon_mds(s, o);
#pragma unroll
        for (int i = 0; i < 12; i++) { put(24 + 2 * i + c, row, o[i]); vals[t[25 + 2 * i + c]] = o[i]; }
      }
      return true;
    }
    default: return false;
  }
}
}  // namespace mp2g
