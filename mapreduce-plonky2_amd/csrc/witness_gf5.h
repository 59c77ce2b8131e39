// The witness tape's GF(p^5) opcodes (include/mp2g.h enum mp2g_witness_op_gf5): ONE definition for the host replay (witness.hip)
// and the device replay (witness_dev.hip), on the Ecgfp5 field arithmetic of gl5.cuh. Restates the hints that
// mp2-common/src/group_hashing/sswu_gadget.rs:57-96 records through [dep] plonky2_ecgfp5 (QuinticSqrtGenerator,
// QuinticQuotientGenerator), with the root fixed by the sgn0 rule of the header. t = the operands after the opcode, vals = the
// proof's slot table.
#pragma once
#include "gl5.cuh"
#include "witness.h"

namespace mp2g {
GLHD gl5 gf5_load(const u64* vals, const u64* s) { return gl5_make(vals[s[0]], vals[s[1]], vals[s[2]], vals[s[3]], vals[s[4]]); }
GLHD void gf5_store(u64* vals, const u64* d, const gl5& x) {
  for (int k = 0; k < 5; k++) vals[d[k]] = x.c[k];
}
GLHD bool exec_gf5_op(u64 op, const u64* t, u64* vals) {
  switch (op) {
    case OP_QUINTIC_SQRT: {
      gl5 r;
      const bool ok = gl5_sqrt(gf5_load(vals, t), r);  // 0 when x is not a square
      if (gl5_sgn0(r)) r = gl5_neg(r);                // the root with sgn0 = 0 (-r flips the parity of the first non-zero limb)
      gf5_store(vals, t + 5, r);
      vals[t[10]] = ok ? 1 : 0;
      return true;
    }
    case OP_QUINTIC_QUOTIENT:
      gf5_store(vals, t + 10, gl5_mul(gf5_load(vals, t), gl5_inv(gf5_load(vals, t + 5))));  // inverse-or-zero: b = 0 gives 0
      return true;
    default: return false;
  }
}
}  // namespace mp2g
