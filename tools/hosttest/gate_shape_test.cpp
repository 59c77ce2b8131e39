// Host-side view of csrc/gate_shape.h gate_shape (what a gate kind is: parameter ranges, constraint count, degree, wires and gate
// constants touched, light or not) and of gate_table_make (csrc/gates.h), so that a test can hold circuits.py's counts, the ranges
// include/mp2g.h documents and the counts recorded before the table had one definition against them (tests/test_gate_shape_host.py).
// build: hipcc -x hip --cuda-host-only -O1 -fsanitize=undefined -fno-sanitize-recover=undefined -std=c++17
//        -I../../mapreduce-plonky2_amd/csrc -I../../include gate_shape_test.cpp -o gate_shape_test
// run:   gate_shape_test < descriptors ("kind p0 p1 p2" in decimal, separated by white space); prints per descriptor
//        "shape CONSTRAINTS DEGREE WIRES CONSTS LIGHT" or "shape refused", then "table ok" or "table refused" for the one-gate table
//        of a circuit with 135 wires, 64 constants and one selector, then "# " and the message of a refusal
#include "gates.h"
#include <cinttypes>
#include <cstdio>
using namespace mp2g;
int main() {
  for (uint64_t w[4]; scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, w, w + 1, w + 2, w + 3) == 4;) {
    const mp2g_gate g{(uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], (uint32_t)w[3], 0, 0, 1};
    const GateShape s = gate_shape(g);
    if (s.err) printf("shape refused ");
    else printf("shape %u %u %u %u %d ", s.constraints, s.degree, s.wires, s.consts, (int)s.light);
    GateTable t;
    uint32_t max_j = ~0u;
    const char* msg = gate_table_make(&g, 1, 1, 0, 64, 135, t, &max_j);
    if (!msg && max_j != s.constraints) msg = "max_j is not the gate's constraint count";
    printf("table %s # %s\n", msg ? "refused" : "ok", msg ? msg : "");
  }
  return 0;
}
