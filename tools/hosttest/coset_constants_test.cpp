// Host-side check of csrc/coset_constants.h against the field code of gl.cuh (gl_root_of_unity, gl_inv, gl_mul).
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -DMP2G_DEVCONST="static const" -I../../mapreduce-plonky2_amd/csrc \
//        coset_constants_test.cpp -o coset_constants_test
#include "gl.cuh"
#include "coset_constants.h"
#include <cstdio>
int main() {
  long bad = 0, n_checked = 0;
  for (unsigned bits = 2; bits <= 5; bits++) {
    const uint64_t npts = 1ull << bits, om = gl_root_of_unity(bits), ninv = gl_inv(npts);
    const uint64_t* xs = COSET_POINTS + MP2G_COSET_TABLE(bits);
    const uint64_t* ws = COSET_WEIGHTS + MP2G_COSET_TABLE(bits);
    uint64_t x = 1;
    for (uint64_t i = 0; i < npts; i++, x = gl_mul(x, om), n_checked++) {
      if (xs[i] != x || xs[i] >= GL_P) bad++;
      if (ws[i] != gl_mul(x, ninv) || ws[i] >= GL_P) bad++;
    }
    if (x != 1) bad++;  // om has order 2^bits
  }
  if (MP2G_COSET_TABLE(5) + 32 != sizeof(COSET_POINTS) / 8 || sizeof(COSET_WEIGHTS) != sizeof(COSET_POINTS)) bad++;
  printf("checked %ld bad %ld\n", n_checked, bad);
  return bad != 0;
}
