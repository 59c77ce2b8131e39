// Host-side run of csrc/keccak.cuh: the same text the kernels of storage.hip compile, for the host alone.
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -I../../mapreduce-plonky2_amd/csrc keccak_host_test.cpp -o keccak_host_test
// (tests/test_keccak_host.py; a sanitizer pass over the portable body goes here: add -fsanitize=address,undefined to the flags).
// `keccak_host_test REQUEST RESULT`: REQUEST is u32 count, stride, domain byte, pad; u32 lens[count]; u8 rows[count][stride], the
// layout mp2g_keccak256_batch takes (stride a multiple of 8). RESULT receives [count][32] digests, then per message the digest of
// keccak256_regs when the message is 32 or 64 bytes long and the domain is 0x01 (zeros otherwise). Nothing is judged here.
// Every row is copied into a buffer of exactly `stride` bytes before it is hashed, so a read at or past the stride is a heap
// overflow that a sanitizer build reports.
#include "keccak.cuh"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace mp2g;

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: keccak_host_test REQUEST RESULT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  u32 h[4];
  if (!f || fread(h, 4, 4, f) != 4) { fprintf(stderr, "bad request\n"); return 2; }
  const u32 count = h[0], stride = h[1], domain = h[2];
  if (!stride || stride % 8) { fprintf(stderr, "stride %u is not a multiple of 8\n", stride); return 2; }
  std::vector<u32> lens(count);
  std::vector<uint8_t> rows((size_t)count * stride);
  if (fread(lens.data(), 4, count, f) != count || fread(rows.data(), 1, rows.size(), f) != rows.size()) { fprintf(stderr, "short request\n"); return 2; }
  fclose(f);
  std::vector<u64> out((size_t)count * 8, 0);
  for (u32 i = 0; i < count; i++) {
    if (lens[i] > stride) { fprintf(stderr, "lens[%u] above the stride\n", i); return 2; }
    u64* row = (u64*)malloc(stride);  // exactly the row: 8-byte aligned, nothing readable behind it
    memcpy(row, rows.data() + (size_t)i * stride, stride);
    keccak256_lanes(row, lens[i], &out[4 * (size_t)i], domain);
    if (domain == 0x01 && lens[i] == 32) keccak256_regs<4>(row, &out[4 * ((size_t)count + i)]);
    if (domain == 0x01 && lens[i] == 64) keccak256_regs<8>(row, &out[4 * ((size_t)count + i)]);
    free(row);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) { fprintf(stderr, "cannot write the result\n"); return 2; }
  fclose(f);
  return 0;
}
