// Shared by witness.hip (host executor, program validation, level schedule) and witness_dev.hip (device executor).
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>
#include "ctx.h"
#include "lookup_wires.h"

namespace mp2g {
// the opcodes are the PUBLIC ones (include/mp2g.h enum mp2g_witness_op: operand layouts and rules are documented there)
enum { OP_ARITH = MP2G_OP_ARITH, OP_ARITH_EXT = MP2G_OP_ARITH_EXT, OP_P2 = MP2G_OP_P2, OP_BASE_SUM = MP2G_OP_BASE_SUM, OP_RA = MP2G_OP_RA,
       OP_REDUCING = MP2G_OP_REDUCING, OP_REDUCING_EXT = MP2G_OP_REDUCING_EXT, OP_COSET = MP2G_OP_COSET, OP_WIRE = MP2G_OP_WIRE,
       OP_HINT_DIV_EXT = MP2G_OP_HINT_DIV_EXT, OP_HINT_LO63 = MP2G_OP_HINT_LO63, OP_HINT_HI = MP2G_OP_HINT_HI, OP_HINT_SPLIT = MP2G_OP_HINT_SPLIT,
       OP_PAR = MP2G_OP_PAR, OP_POSEIDON = MP2G_OP_POSEIDON, OP_U32_ARITH = MP2G_OP_U32_ARITH, OP_U32_SUB = MP2G_OP_U32_SUB,
       OP_U32_ADD_MANY = MP2G_OP_U32_ADD_MANY, OP_U32_RANGE_CHECK = MP2G_OP_U32_RANGE_CHECK, OP_COMPARISON = MP2G_OP_COMPARISON,
       OP_BASE_SPLIT = MP2G_OP_BASE_SPLIT, OP_MUL_EXT = MP2G_OP_MUL_EXT, OP_EXP = MP2G_OP_EXP, OP_END = MP2G_OP_END };
// the second block (include/mp2g.h enum mp2g_witness_op_gf5): GF(p^5) hints, witness_gf5.h
enum { OP_QUINTIC_SQRT = MP2G_OP_QUINTIC_SQRT, OP_QUINTIC_QUOTIENT = MP2G_OP_QUINTIC_QUOTIENT, OP_GF5_END = MP2G_OP_GF5_END };
GLHD bool op_is_gf5(u64 op) { return op >= OP_QUINTIC_SQRT && op < OP_GF5_END; }
// the third block (include/mp2g.h enum mp2g_witness_op_lut): lookups into the circuit's tables (mp2g_witness_program_set_lookups)
enum { OP_LOOKUP = MP2G_OP_LOOKUP, OP_LUT_END = MP2G_OP_LUT_END };
GLHD bool op_is_lut(u64 op) { return op >= OP_LOOKUP && op < OP_LUT_END; }
// the fourth block (include/mp2g.h enum mp2g_witness_op_wide): interleave gates, multi-limb division hints, PoseidonMds; witness_wide.h
enum { OP_U32_INTERLEAVE = MP2G_OP_U32_INTERLEAVE, OP_UNINTERLEAVE_TO_B32 = MP2G_OP_UNINTERLEAVE_TO_B32,
       OP_UNINTERLEAVE_TO_U32 = MP2G_OP_UNINTERLEAVE_TO_U32, OP_U256_DIV = MP2G_OP_U256_DIV, OP_BIGUINT_DIV_REM = MP2G_OP_BIGUINT_DIV_REM,
       OP_POSEIDON_MDS = MP2G_OP_POSEIDON_MDS, OP_WIDE_END = MP2G_OP_WIDE_END };
GLHD bool op_is_wide(u64 op) { return op >= OP_U32_INTERLEAVE && op < OP_WIDE_END; }
const u32 BIGUINT_MAX_LIMBS = 32;  // MP2G_OP_BIGUINT_DIV_REM: limbs of either operand
const u32 BASE_SUM_LIMBS = 63, RA_BITS = 4, RA_COPIES = 4, RED_COEFFS = 43, RED_EXT_COEFFS = 32, NUM_WIRES = 135;

// the program's read-only data on one device (uploaded at the first device run there)
struct WitnessDev {
  int device = -1;
  DevBuf tape, sched, level_off, level_p2, input_sids, consts, domtab, probe;
  // the program's lookup tables (n_luts = 0: none): tables and input index on the device, the description by value for the
  // lookup-wires pass and in device memory (lut_desc) for the executor's MP2G_OP_LOOKUP
  DevBuf lut_tables, lut_index, lut_desc;
  LutIndex lut{};
};
// device executor (witness_dev.hip): one block per proof walks the level schedule; gf5 = the program holds GF(p^5) opcodes (a tape
// without them runs the kernel instance that has no code for them). witness_exec_launch_wide (witness_dev_wide.hip): the same for a
// program that holds wide opcodes, with the instances that carry their code.
hipError_t witness_exec_launch(hipStream_t s, const WitnessDev& d, bool gf5, u32 n_levels, u32 n_slots, u32 log_n, u32 n_inputs, u32 n_consts,
                               u32 n_probe, const u64* d_inputs, u32 batch, u64* d_vals, u64* d_wires, u64* d_probe_out);
hipError_t witness_exec_launch_wide(hipStream_t s, const WitnessDev& d, bool gf5, u32 n_levels, u32 n_slots, u32 log_n, u32 n_inputs, u32 n_consts,
                                    u32 n_probe, const u64* d_inputs, u32 batch, u64* d_vals, u64* d_wires, u64* d_probe_out);
const u32 WIT_LU_SLOTS = 40, WIT_LUT_SLOTS = 26;  // LookupGate / LookupTableGate num_slots with 80 routed wires
}  // namespace mp2g

struct mp2g_witness_program {
  std::vector<u64> tape;
  std::vector<u32> input_sids;
  std::vector<u64> consts;  // (sid, value) pairs
  u32 n_slots = 0, log_n = 0;
  u64 dom[6][32], bw[6][32];  // two-adic subgroup of 2^bits points and its barycentric weights, bits <= 5
  // level schedule for the device executor: instruction offsets ordered by (dependency level, opcode); a level's instructions
  // read only slots written at lower levels (every slot is written once: the builder's programs are in SSA form)
  std::vector<u32> sched, level_off;
  std::vector<u32> level_p2;  // per level: first schedule index and count of its Poseidon2 rows (one opcode = one contiguous run)
  bool ssa = true;
  bool gf5 = false;        // the tape holds GF(p^5) opcodes (include/mp2g.h enum mp2g_witness_op_gf5)
  bool wide = false;       // the tape holds wide opcodes (include/mp2g.h enum mp2g_witness_op_wide)
  // lookup tables (mp2g_witness_program_set_lookups): the copied tables, their input index, and the description the host replay
  // and its lookup-wires pass read (host pointers into the two vectors)
  bool has_lookup = false;  // the tape holds MP2G_OP_LOOKUP
  std::vector<mp2g::u16> lut_tables;
  std::vector<u32> lut_index;
  mp2g::LutIndex lut{};
  std::vector<u32> probe;  // slots returned next to the wires by the device run (mp2g_witness_program_set_probe)
  std::mutex dev_mu;
  std::vector<mp2g::WitnessDev*> dev;  // per device
  ~mp2g_witness_program() { for (auto* d : dev) delete d; }
};
