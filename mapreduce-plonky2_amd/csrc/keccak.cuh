// Keccak-f[1600] and the Keccak-256 sponge (rate 136 bytes, domain byte 0x01, final bit 0x80: Ethereum's keccak256, not SHA3-256,
// whose domain byte is 0x06), one body for every kernel of storage.hip and for the host test (tools/hosttest/keccak_host_test.cpp).
// Replaces, on the value (non-circuit) side, [dep] alloy keccak256 as mp2-common/src/eth.rs:233-276 and the `keccak256(node)` sites
// of mp2-v1/src/values_extraction call it.
//
// One lane per message. The state is 25 u64 whose every index is static after unrolling (rho/pi runs over two constexpr tables in
// fully unrolled loops), so it lives in 50 VGPRs; only the round loop stays a loop (24 x ~400 VALU instructions unrolled would not
// fit the instruction cache), and its round constant is the one table read by a runtime index: it is uniform and comes through the
// scalar cache. No private array is indexed by a runtime value, so nothing goes to scratch. What the compiler makes of one round
// (read in the saved ISA): 152 v_xor_b32 (theta, and chi's outer xor), 50 v_bfi_b32 (chi's and-not, one per half lane), 58
// v_alignbit_b32 (the 29 rotations, see keccak_rotl): 260 VALU instructions, 6240 per permutation, which is the operation count of
// the algorithm on 32-bit halves. No hand-written assembly.
//
// The bodies are GLHD, not GLD: the text is the same for device and host, and the host test calls it from its main().
#pragma once
#include "gl.cuh"

namespace mp2g {
#define KECCAK_RATE 136  // bytes: 17 lanes
#define KECCAK_RATE_LANES 17

// Rotation by a constant. The portable body is two plain shifts of the 64-bit value. From that text the gfx950 compiler makes
// v_lshlrev_b64 + v_lshrrev_b32/_b64 + v_or_b32 (85 instructions for the 29 rotations of a round, 19 + 10 of them 64-bit shifts), so
// the device body says what a rotation is on two halves: each half of the result is one 32-bit funnel shift (v_alignbit_b32) of the
// two halves of the input, and a rotation by 32 or more swaps the halves first. A builtin, not assembly.
template <int N>
GLHD u64 keccak_rotl(u64 v) {
  if constexpr (N == 0) return v;
#if defined(__HIP_DEVICE_COMPILE__)
  else if constexpr (N % 32 == 0) return (v << 32) | (v >> 32);
  else {
    const u32 a = N < 32 ? (u32)(v >> 32) : (u32)v, b = N < 32 ? (u32)v : (u32)(v >> 32);  // the halves after the swap: a high, b low
    return gl_mk(__builtin_amdgcn_alignbit(b, a, 32 - N % 32), __builtin_amdgcn_alignbit(a, b, 32 - N % 32));
  }
#else
  else return (v << N) | (v >> (64 - N));
#endif
}

// theta, rho, pi, chi of one round; lane (x, y) is a[x + 5 y]
GLHD void keccak_round(u64 a[25], u64 rc) {
  // rho's offset of lane x + 5 y, and where pi sends it: (x, y) -> (y, 2 x + 3 y)
  constexpr int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  u64 c[5], b[25];
#pragma unroll
  for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; x++) {
    const u64 d = c[(x + 4) % 5] ^ keccak_rotl<1>(c[(x + 1) % 5]);
#pragma unroll
    for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
  }
#define KECCAK_RHO_PI(i) b[((i) / 5) + 5 * ((2 * ((i) % 5) + 3 * ((i) / 5)) % 5)] = keccak_rotl<ROT[i]>(a[i]);
  KECCAK_RHO_PI(0) KECCAK_RHO_PI(1) KECCAK_RHO_PI(2) KECCAK_RHO_PI(3) KECCAK_RHO_PI(4)
  KECCAK_RHO_PI(5) KECCAK_RHO_PI(6) KECCAK_RHO_PI(7) KECCAK_RHO_PI(8) KECCAK_RHO_PI(9)
  KECCAK_RHO_PI(10) KECCAK_RHO_PI(11) KECCAK_RHO_PI(12) KECCAK_RHO_PI(13) KECCAK_RHO_PI(14)
  KECCAK_RHO_PI(15) KECCAK_RHO_PI(16) KECCAK_RHO_PI(17) KECCAK_RHO_PI(18) KECCAK_RHO_PI(19)
  KECCAK_RHO_PI(20) KECCAK_RHO_PI(21) KECCAK_RHO_PI(22) KECCAK_RHO_PI(23) KECCAK_RHO_PI(24)
#undef KECCAK_RHO_PI
#pragma unroll
  for (int y = 0; y < 25; y += 5) {
#pragma unroll
    for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
  }
  a[0] ^= rc;
}

GLHD void keccak_f1600(u64 a[25]) {
  constexpr u64 RC[24] = {
      0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
      0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
      0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
      0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
      0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
#pragma unroll 1
  for (int r = 0; r < 24; r++) keccak_round(a, RC[r]);
}

// Keccak-256 of the len bytes at msg (8-byte aligned; the message's row ends at a multiple of 8 bytes at or after len, and no byte
// at or past that end is read): out[0..4) are the 32 digest bytes as little-endian lanes, out[k] = bytes 8 k .. 8 k + 7. The last,
// partial block is loaded in whole words, the bytes at or past len are masked out of the loaded word and the padding is xored in:
// a byte past len never reaches the state. `domain` is 0x01 for Keccak-256 (0x06 would be SHA3-256: the host test's cross-check).
GLHD void keccak256_lanes(const u64* msg, u32 len, u64 out[4], u64 domain = 0x01) {
  u64 a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  const u32 full = len / KECCAK_RATE;
  for (u32 blk = 0; blk < full; blk++) {  // per lane: the lanes of one wave may run different block counts
#pragma unroll
    for (int j = 0; j < KECCAK_RATE_LANES; j++) a[j] ^= msg[j];
    msg += KECCAK_RATE_LANES;
    keccak_f1600(a);
  }
  const u32 rem = len - full * KECCAK_RATE;  // 0..135
#pragma unroll
  for (int j = 0; j < KECCAK_RATE_LANES; j++) {
    u64 w = 0;
    if (8u * j < rem) {  // the word's first byte is a message byte, so the whole word lies inside the row
      w = msg[j];
      const u32 have = rem - 8u * j;
      if (have < 8) w &= ~(~(u64)0 << (8 * have));
    }
    if ((u32)j == rem / 8) w ^= domain << (8 * (rem % 8));
    a[j] ^= w;
  }
  a[KECCAK_RATE_LANES - 1] ^= 0x8000000000000000ULL;  // the same byte as the domain's when rem == 135
  keccak_f1600(a);
#pragma unroll
  for (int k = 0; k < 4; k++) out[k] = a[k];
}

// Keccak-256 of a message that is already in registers as n_lanes <= 16 whole little-endian lanes (32- and 64-byte messages: one
// rate block, built without touching memory)
template <int LANES>
GLHD void keccak256_regs(const u64 m[LANES], u64 out[4]) {
  static_assert(LANES < KECCAK_RATE_LANES - 1, "one block, the padding in lanes of its own");
  u64 a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = i < LANES ? m[i] : 0;
  a[LANES] = 0x01;
  a[KECCAK_RATE_LANES - 1] = 0x8000000000000000ULL;
  keccak_f1600(a);
#pragma unroll
  for (int k = 0; k < 4; k++) out[k] = a[k];
}
}  // namespace mp2g
