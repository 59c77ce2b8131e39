// Host-side view of csrc/witness_ops.h op_shape: walks a witness tape and prints every instruction's shape, so that a test can hold
// recursion.py's table (_OPS) against it (tests/test_witness_shape_host.py).
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -I../../mapreduce-plonky2_amd/csrc -I../../include witness_shape_test.cpp -o witness_shape_test
// run:   witness_shape_test < tape (decimal words separated by white space); prints "pos op len first_slot r0 nr w0 nw" per instruction -- the
//        sections of a parallel region follow its header as ordinary instructions -- and exits 1 at a malformed or truncated one
#include "witness_ops.h"
#include <cinttypes>
#include <cstdio>
#include <vector>
using namespace mp2g;
int main() {
  std::vector<u64> tape;
  for (uint64_t w; scanf("%" SCNu64, &w) == 1;) tape.push_back(w);
  for (size_t pos = 0; pos < tape.size();) {
    const size_t left = tape.size() - pos - 1;
    const OpShape s = op_shape(tape[pos], tape.data() + pos + 1, left);
    if (s.len == ~0u || s.len > left) { printf("%zu %" PRIu64 " malformed\n", pos, (uint64_t)tape[pos]); return 1; }
    printf("%zu %" PRIu64 " %u %u %u %u %u %u\n", pos, (uint64_t)tape[pos], s.len, s.first_slot, s.r0, s.nr, s.w0, s.nw);
    pos += 1 + s.len;
  }
  return 0;
}
