// The ONE table of what a gate kind is (include/mp2g.h names the kinds and documents their parameters): gate_shape() checks a
// descriptor's parameters and gives Gate::num_constraints, Gate::degree and what the evaluator (eval_gate, gates.hip) touches.
// Table validation, the launch lists of gates.hip, the public queries and the verifier's line-point count all read it; nothing else
// restates a kind. Host code only, no HIP: tools/hosttest/gate_shape_test.cpp compiles it alone. Descriptors are caller data, so
// every parameter is range-checked before it is shifted or divided by, and the counts are formed in 64 bits: one that does not fit
// 32 bits makes the descriptor malformed. A new kind is one case here, one entry of MP2G_CONSTRAINT_GATES and one case of eval_gate.
#pragma once
#include <stdint.h>
#include "mp2g.h"

namespace mp2g {

// the kinds of the fused "light" launch (gate_constraints_lde_light_kernel), and all kinds that have constraints of their own
#define MP2G_LIGHT_GATES(X)                                                                                                   \
  X(MP2G_GATE_CONSTANT) X(MP2G_GATE_PUBLIC_INPUT) X(MP2G_GATE_ARITHMETIC) X(MP2G_GATE_BASE_SUM) X(MP2G_GATE_ARITHMETIC_EXT)  \
  X(MP2G_GATE_MUL_EXT)
#define MP2G_CONSTRAINT_GATES(X)                                                                                              \
  MP2G_LIGHT_GATES(X)                                                                                                         \
  X(MP2G_GATE_POSEIDON2) X(MP2G_GATE_EXPONENTIATION) X(MP2G_GATE_REDUCING) X(MP2G_GATE_REDUCING_EXT) X(MP2G_GATE_RANDOM_ACCESS) \
  X(MP2G_GATE_POSEIDON) X(MP2G_GATE_POSEIDON_MDS) X(MP2G_GATE_COSET_INTERPOLATION) X(MP2G_GATE_U32_ARITHMETIC)               \
  X(MP2G_GATE_U32_RANGE_CHECK) X(MP2G_GATE_U32_SUBTRACTION) X(MP2G_GATE_U32_ADD_MANY) X(MP2G_GATE_COMPARISON)                \
  X(MP2G_GATE_U32_INTERLEAVE) X(MP2G_GATE_UNINTERLEAVE_TO_B32) X(MP2G_GATE_UNINTERLEAVE_TO_U32)

struct GateShape {
  uint32_t constraints, degree;  // Gate::num_constraints, Gate::degree
  uint32_t wires, consts;        // highest wire index + 1 and gate constants (after the selector prefix) the evaluator touches
  bool light;                    // a kind of MP2G_LIGHT_GATES
  const char* err;               // nullptr, or why the descriptor is malformed (every other field is then 0)
};

inline GateShape gate_shape(const mp2g_gate& g) {
  const uint64_t p0 = g.p0, p1 = g.p1, p2 = g.p2;
  uint64_t k = 0, d = 0, w = 0, c = 0;  // constraints, degree, wires, constants
  const char* err = nullptr;
  bool light = false;
  switch (g.kind) {
#define MP2G_X(K) case K:
    MP2G_LIGHT_GATES(MP2G_X) light = true; break;
#undef MP2G_X
    default: break;
  }
  switch (g.kind) {
    case MP2G_GATE_NOOP: break;
    case MP2G_GATE_CONSTANT: k = p0; d = 1; w = p0; c = p0; break;
    case MP2G_GATE_PUBLIC_INPUT: k = 4; d = 1; w = 4; break;
    case MP2G_GATE_ARITHMETIC: k = p0; d = 3; w = 4 * p0; c = 2; break;
    case MP2G_GATE_BASE_SUM:
      if (p1 < 2 || p0 < 1) { err = "BaseSumGate needs base >= 2 and a limb"; break; }
      k = 1 + p0; d = p1; w = 1 + p0;
      break;
    case MP2G_GATE_ARITHMETIC_EXT: k = 2 * p0; d = 3; w = 8 * p0; c = 2; break;
    case MP2G_GATE_MUL_EXT: k = 2 * p0; d = 3; w = 6 * p0; c = 1; break;
    case MP2G_GATE_POSEIDON2: case MP2G_GATE_POSEIDON: k = 1 + 4 + 36 + 22 + 48 + 12; d = 7; w = 135; break;
    case MP2G_GATE_POSEIDON_MDS: k = 24; d = 1; w = 48; break;
    case MP2G_GATE_COSET_INTERPOLATION: {
      if (p0 < 2 || p0 > 5 || p1 < 2 || p1 > ((uint64_t)1 << p0)) {
        err = "CosetInterpolationGate needs 2..5 subgroup bits and 2 <= degree <= 2^bits";
        break;
      }
      const uint64_t npts = (uint64_t)1 << p0, nint = (npts - 2) / (p1 - 1);  // intermediate (eval, prod) pairs between the chunks
      k = 4 + 4 * nint; d = p1; w = 1 + 2 * npts + 6 + 4 * nint;
      break;
    }
    case MP2G_GATE_U32_ARITHMETIC: case MP2G_GATE_U32_RANGE_CHECK: case MP2G_GATE_U32_SUBTRACTION:
      if (p0 < 1) { err = "u32 gate needs at least one operation"; break; }
      k = (g.kind == MP2G_GATE_U32_ARITHMETIC ? 36 : g.kind == MP2G_GATE_U32_RANGE_CHECK ? 17 : 19) * p0;
      w = (g.kind == MP2G_GATE_U32_ARITHMETIC ? 38 : g.kind == MP2G_GATE_U32_RANGE_CHECK ? 17 : 21) * p0;
      d = 4;
      break;
    case MP2G_GATE_U32_ADD_MANY:
      if (p0 < 1 || p0 > 16 || p1 < 1) { err = "U32AddManyGate needs 1..16 addends and an operation"; break; }
      k = 21 * p1; d = 4; w = (p0 + 3 + 18) * p1;
      break;
    case MP2G_GATE_COMPARISON: {
      const uint64_t bits = p1 ? (p0 + p1 - 1) / p1 : 0;  // of a chunk
      if (p1 < 1 || p0 < p1 || bits > 4) { err = "ComparisonGate needs num_chunks >= 1 and chunks of at most 4 bits"; break; }
      k = 6 + 5 * p1 + bits; d = (uint64_t)1 << bits; w = 4 + 5 * p1 + bits + 1;
      break;
    }
    case MP2G_GATE_EXPONENTIATION:
      if (p0 < 1) { err = "ExponentiationGate needs at least one power bit"; break; }
      k = p0 + 1; d = 4; w = 2 * p0 + 2;
      break;
    case MP2G_GATE_REDUCING: case MP2G_GATE_REDUCING_EXT:
      if (p0 < 1) { err = "ReducingGate needs at least one coefficient"; break; }
      k = 2 * p0; d = 2; w = 6 + (g.kind == MP2G_GATE_REDUCING_EXT ? 2 : 1) * p0 + 2 * (p0 - 1);
      break;
    case MP2G_GATE_RANDOM_ACCESS:
      if (p0 < 1 || p0 > 6 || p1 < 1) { err = "RandomAccessGate needs 1..6 bits and a copy"; break; }
      k = (p0 + 2) * p1 + p2; d = p0 + 1; w = (2 + ((uint64_t)1 << p0)) * p1 + p2 + p0 * p1; c = p2;
      break;
    case MP2G_GATE_LOOKUP: case MP2G_GATE_LOOKUP_TABLE:  // no constraints of their own
      if (p0 < 1) { err = "lookup gate needs at least one slot"; break; }
      w = (g.kind == MP2G_GATE_LOOKUP ? 2 : 3) * p0;
      break;
    case MP2G_GATE_U32_INTERLEAVE: case MP2G_GATE_UNINTERLEAVE_TO_B32: case MP2G_GATE_UNINTERLEAVE_TO_U32:
      if (p0 < 1) { err = "interleave gate needs at least one operation"; break; }
      k = w = (g.kind == MP2G_GATE_U32_INTERLEAVE ? 34 : 67) * p0; d = 2;
      break;
    default: err = "unknown gate kind"; break;
  }
  if (!err && ((k | w | c | d) >> 32)) err = "gate's wire or constraint count does not fit 32 bits";
  if (err) return GateShape{0, 0, 0, 0, false, err};
  return GateShape{(uint32_t)k, (uint32_t)d, (uint32_t)w, (uint32_t)c, light, nullptr};
}
// Gate::num_constraints / Gate::degree; 0 for a malformed descriptor
inline uint32_t gate_num_constraints(const mp2g_gate& g) { return gate_shape(g).constraints; }
inline uint32_t gate_degree(const mp2g_gate& g) { return gate_shape(g).degree; }
// degree of the gate's constraints times its selector filter (gates/selectors.rs: one factor per other gate of the group, one
// more for the unused-slot value when the circuit has several selector polynomials), for a gate inside its group; 64 bits, as a
// BaseSumGate's degree is its base
inline uint64_t gate_filtered_degree(const mp2g_gate& g, uint32_t num_selectors) {
  return (uint64_t)gate_degree(g) + (g.group_end - g.group_start - 1) + (num_selectors > 1 ? 1 : 0);
}
}  // namespace mp2g
