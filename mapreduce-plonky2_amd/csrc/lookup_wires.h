// prove()'s set_lookup_wires ([dep] plonk/prover.rs): the padding of the LookupGate rows and the LookupTableGate rows (table entries
// and their multiplicities) of a wire matrix, for the prover (mp2g_prover_lookup_wires_dev) and the witness tape's replays
// (MP2G_OP_LOOKUP, witness_ops.h). One description of a circuit's tables serves the kernel, its plain C++ twin for the host replays
// (both in lookup_wires.hip) and the opcode's body: the pointers are device memory on the device, host memory on the host.
#pragma once
#include "ctx.h"
#include <vector>

namespace mp2g {
typedef uint16_t u16;
const u32 LUT_ABSENT = 0xFFFFFFFFu;  // index[input]: the table has no entry with that input
const u32 LUT_INPUTS = 65536;        // table inputs are u16
struct LutIndex {
  u32 n_luts;
  u32 lu_slots, lut_slots;  // LookupGate / LookupTableGate num_slots (40, 26 under standard_recursion_config)
  u32 last_lu_row[MP2G_MAX_LUTS], last_lut_row[MP2G_MAX_LUTS], first_lut_row[MP2G_MAX_LUTS], table_len[MP2G_MAX_LUTS];
  u32 n_lookups[MP2G_MAX_LUTS];     // the table's looked-up slots; the rest of its LookupGate rows is padding
  const u16* table[MP2G_MAX_LUTS];  // [table_len][2] = (input, output)
  const u32* index[MP2G_MAX_LUTS];  // [LUT_INPUTS]: input -> entry, LUT_ABSENT
};
// the entry a looked-up pair counts for; LUT_ABSENT: the pair is not in the table (nothing is counted, the proof fails the lookup
// argument later)
GLHD u32 lut_entry(const LutIndex& L, u32 t, u64 inp, u64 out) {
  if (inp >= LUT_INPUTS) return LUT_ABSENT;
  const u32 e = L.index[t][inp];
  return e != LUT_ABSENT && L.table[t][2 * e + 1] == out ? e : LUT_ABSENT;
}
// index[t] of every table, [n_luts][LUT_INPUTS], built once at set-up; false: a table holds an input twice
inline bool lut_build_index(const mp2g_lookup* luts, u32 n_luts, std::vector<u32>& index) {
  index.assign((size_t)n_luts * LUT_INPUTS, LUT_ABSENT);
  bool unique = true;
  for (u32 t = 0; t < n_luts; t++)
    for (u32 e = 0; e < luts[t].table_len; e++) {
      u32& slot = index[(size_t)t * LUT_INPUTS + luts[t].table[2 * e]];
      if (slot != LUT_ABSENT) unique = false; else slot = e;
    }
  return unique;
}
// wire (col, row) of proof b sits at wires[b * bstride + col * cs + row * rs]: (n, 1) = the prover's [batch][wires_w][n],
// (1, 135) = the witness executor's row-major staging [batch][n][135]. One block per (proof, table); every row, column and n_lookups
// of L must have been checked against the matrix by the caller.
hipError_t lookup_wires_launch(hipStream_t s, const LutIndex& L, u64* d_wires, u32 batch, u64 bstride, u64 cs, u64 rs);
// the plain C++ twin, one proof (host pointers in L)
void lookup_wires_host(const LutIndex& L, u64* wires, u64 cs, u64 rs);
}  // namespace mp2g
