// The portable (#else) body of gl_mulc_addw (csrc/gl.cuh) compiled for the host, for tests/test_p2_diag_constants.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 "-DMP2G_DEVCONST=static const" -I mapreduce-plonky2_amd/csrc mulc_host_test.cpp
//   mulc_host_test REQUEST RESULT
// REQUEST: u64 n, u64 k, then a[n], c[n]. RESULT: out[n] = gl_mulc_addw(a[i], d_k, e_k, c[i]) for the diagonal entry k < 12 of Poseidon2's
// internal layer and its fold e_k = POSEIDON2_DIAG_M1_SHL32[k]. No checking happens here. Exit status 2: a malformed request.
//   mulc_host_test --constants
// prints what poseidon.cuh derives from the diagonal at compile time: the twelve e_k in hex, one a line, then POSEIDON2_DIAG_NARROW.
#include <cstring>
#include <cstdio>
#include <vector>
#include "poseidon.cuh"

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--constants")) {
    for (int k = 0; k < 12; k++) printf("%016llx\n", (unsigned long long)c_p2_diag_shl32[k]);
    printf("%x\n", POSEIDON2_DIAG_NARROW);
    return 0;
  }
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  u64 head[2];
  if (fread(head, sizeof(u64), 2, f) != 2 || head[0] == 0 || head[0] > (1u << 24) || head[1] >= 12) return 2;
  const size_t n = head[0];
  const int k = (int)head[1];
  std::vector<u64> a(n), c(n), out(n);
  if (fread(a.data(), sizeof(u64), n, f) != n || fread(c.data(), sizeof(u64), n, f) != n) return 2;
  fclose(f);
  for (size_t i = 0; i < n; i++) {
    out[i] = gl_mulc_addw<false>(a[i], c_p2_diag[k], c_p2_diag_shl32[k], c[i]);
    // the host has one body for both forms, and p2_internal's helper picks between them
    if (gl_mulc_addw<true>(a[i], c_p2_diag[k], c_p2_diag_shl32[k], c[i]) != out[i] || p2_diag_mul_addw(k, a[i], c[i]) != out[i]) return 3;
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(u64), n, f) != n) return 2;
  fclose(f);
  return 0;
}
