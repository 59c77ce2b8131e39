// Witness generation for circuits built by recursion.py (host code; no GPU involved).
//
// Replaces [dep] plonky2 iop/generator.rs generate_partial_witness for the circuits of the recursion framework
// (first line of prove(), recursion-framework/src/circuit_builder.rs:308, wrap_circuit.rs:143): the wrap circuit,
// the universal-verifier circuits and their logic. plonky2 walks a dependency graph of per-gate generators; here the
// builder's operations are recorded once, in order, as a straight-line program over value slots (recursion.py OP_*),
// because the structure of these circuits does not depend on the witness. Replaying the program for one input
// vector (the inner proof, its verifier data, the circuit's own inputs) fills the 135 x n wire matrix; a batch of
// input vectors is replayed by a pool of host threads, one proof per thread at a time, straight into the layout
// mp2g_prover_prove_dev takes ([batch][135][n]).
#define MP2G_DEVCONST static const
#include "gl.cuh"
#include "perm_constants.h"
#include "ctx.h"
#include "witness.h"
#include "witness_ops.h"
#include "witness_gf5.h"
#include "witness_wide.h"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

using namespace mp2g;

namespace {
// Poseidon2 linear layers on canonical values (poseidon.cuh keeps weak forms for the device; the witness wants the
// intermediate states, canonical, as the gate's wires)
// circ(2 M4, M4, M4) with M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]]: M4 by its addition chain (t0 = x0 + x1, t1 = x2 + x3,
// t2 = 2 x1 + t1, t3 = 2 x3 + t0, t4 = 4 t1 + t3, t5 = 4 t0 + t2, rows = t3 + t5, t5, t2 + t4, t4) in 128-bit integers -- every
// entry of the layer stays below 2^70 -- and ONE reduction per output limb (a third of a host permutation was spent here on
// 16 modular multiply-by-constant and 28 modular additions per block)
void p2_external(u64 s[12]) {
  typedef unsigned __int128 u128;
  u128 t[12];
  for (int c = 0; c < 3; c++) {
    const u128 x0 = s[4 * c], x1 = s[4 * c + 1], x2 = s[4 * c + 2], x3 = s[4 * c + 3];
    const u128 t0 = x0 + x1, t1 = x2 + x3, t2 = 2 * x1 + t1, t3 = 2 * x3 + t0, t4 = 4 * t1 + t3, t5 = 4 * t0 + t2;
    t[4 * c] = t3 + t5; t[4 * c + 1] = t5; t[4 * c + 2] = t2 + t4; t[4 * c + 3] = t4;
  }
  for (int i = 0; i < 4; i++) {
    const u128 sum = t[i] + t[4 + i] + t[8 + i];
    for (int c = 0; c < 3; c++) {
      const u128 v = t[4 * c + i] + sum;
      s[4 * c + i] = gl_reduce128((u64)v, (u64)(v >> 64));
    }
  }
}
// x_i <- mu_i x_i + sum_j x_j: the sum and each product in 128 bits, one reduction per limb
void p2_internal(u64 s[12]) {
  typedef unsigned __int128 u128;
  u128 sum = 0;
  for (int i = 0; i < 12; i++) sum += s[i];
  const u64 sr = gl_reduce128((u64)sum, (u64)(sum >> 64));
  for (int i = 0; i < 12; i++) {
    const u128 v = (u128)s[i] * POSEIDON2_DIAG_M1[i];
    // lo + hi 2^64 + sr: add sr into the low word with carry into hi (hi <= 2^64 - 2 for canonical factors)
    u64 lo = (u64)v, hi = (u64)(v >> 64);
    const u64 l2 = lo + sr;
    hi += l2 < lo ? 1 : 0;
    s[i] = gl_reduce128(l2, hi);
  }
}
// Poseidon's MDS layer on canonical values: circ [17,15,41,16,2,28,13,13,39,18,34,20] + diag [8,0,...]; entries < 2^6, so a row sum
// stays below 2^74: one reduction per output limb
void poseidon_mds_host(u64 s[12]) {
  typedef unsigned __int128 u128;
  u64 out[12];
  for (int r = 0; r < 12; r++) {
    u128 acc = (u128)s[r] * POSEIDON_MDS_DIAG[r];
    for (int i = 0; i < 12; i++) acc += (u128)s[(i + r) % 12] * POSEIDON_MDS_CIRC[i];
    out[r] = gl_reduce128((u64)acc, (u64)(acc >> 64));
  }
  for (int i = 0; i < 12; i++) s[i] = out[i];
}
}  // namespace

namespace {
// the instructions of [t, end). A parallel region (OP_PAR) is a run of sections that read what came before the region and each
// other's nothing: the builder brackets the query rounds of a FRI verifier this way (28 per verified proof). With inner > 1 the
// sections of a region are dealt to that many threads; every instruction writes value slots and wire cells of its own.
void exec(const mp2g_witness_program& P, const u64* t, const u64* end, u64* vals, u64* wires, u32 inner, u64 cs, u64 rs) {
  // wire (col, row) sits at col * cs + row * rs: (n, 1) = the prover's polynomial-major matrix, (1, 135) = one contiguous row per
  // gate row (what the host writes fastest: a Poseidon2 row is 135 consecutive words instead of 135 cache lines)
#define W(col, row) wires[(u64)(col) * cs + (u64)(row) * rs]
  while (t < end) {
    const u64 op = *t++;
    const u32 oplen = op_shape(op, t, (size_t)(end - t)).len;  // validated at create
    switch (op) {
      case OP_PAR: {
        const u32 ns = (u32)t[0];
        const u64* len = t + 1;
        const u64* body = t + oplen;
        u64 total = 0;
        for (u32 i = 0; i < ns; i++) total += len[i];
        if (inner <= 1 || ns <= 1) {
          exec(P, body, body + total, vals, wires, 1, cs, rs);
        } else {
          std::vector<const u64*> start(ns + 1);
          start[0] = body;
          for (u32 i = 0; i < ns; i++) start[i + 1] = start[i] + len[i];
          std::atomic<u32> next{0};
          auto worker = [&]() {
            for (;;) {
              const u32 i = next.fetch_add(1);
              if (i >= ns) return;
              exec(P, start[i], start[i + 1], vals, wires, 1, cs, rs);
            }
          };
          const u32 nt = inner < ns ? inner : ns;
          std::vector<std::thread> pool;
          try {
            for (u32 i = 1; i < nt; i++) pool.emplace_back(worker);
          } catch (...) {
            // fewer threads than hoped for: the sections are dealt from a shared counter
          }
          worker();
          for (auto& th : pool) th.join();
        }
        t += total;  // the sections; the header goes with the other instructions' operands below
        break;
      }
      case OP_P2: {  // Poseidon2Gate: inputs 0..11, outputs 12..23, swap 24, deltas 25..28, S-box inputs 29.., 65.., 87..
        const u64 row = t[0];
        u64 in[12], s[12];
        for (int i = 0; i < 12; i++) { in[i] = vals[t[1 + i]]; W(i, row) = in[i]; }
        const u64 swap = vals[t[13]];
        W(24, row) = swap;
        for (int i = 0; i < 4; i++) {
          const u64 delta = gl_mul(swap, gl_sub(in[i + 4], in[i]));
          W(25 + i, row) = delta;
          s[i] = gl_add(in[i], delta);
          s[i + 4] = gl_sub(in[i + 4], delta);
        }
        for (int i = 8; i < 12; i++) s[i] = in[i];
        p2_external(s);
        for (int r = 0; r < 4; r++) {
          for (int i = 0; i < 12; i++) s[i] = gl_add(s[i], POSEIDON2_RC_EXT[12 * r + i]);
          if (r) for (int i = 0; i < 12; i++) W(29 + 12 * (r - 1) + i, row) = s[i];
          for (int i = 0; i < 12; i++) s[i] = gl_pow7(s[i]);
          p2_external(s);
        }
        for (int r = 0; r < 22; r++) {
          s[0] = gl_add(s[0], POSEIDON2_RC_INT[r]);
          W(65 + r, row) = s[0];
          s[0] = gl_pow7(s[0]);
          p2_internal(s);
        }
        for (int r = 0; r < 4; r++) {
          for (int i = 0; i < 12; i++) { s[i] = gl_add(s[i], POSEIDON2_RC_EXT[12 * (4 + r) + i]); W(87 + 12 * r + i, row) = s[i]; }
          for (int i = 0; i < 12; i++) s[i] = gl_pow7(s[i]);
          p2_external(s);
        }
        for (int i = 0; i < 12; i++) { W(12 + i, row) = s[i]; vals[t[14 + i]] = s[i]; }
        break;
      }
      case OP_POSEIDON: {  // PoseidonGate: the wire layout of the Poseidon2 gate, the original permutation (30 rounds, 4 + 22 + 4)
        const u64 row = t[0];
        u64 in[12], s[12];
        for (int i = 0; i < 12; i++) { in[i] = vals[t[1 + i]]; W(i, row) = in[i]; }
        const u64 swap = vals[t[13]];
        W(24, row) = swap;
        for (int i = 0; i < 4; i++) {
          const u64 delta = gl_mul(swap, gl_sub(in[i + 4], in[i]));
          W(25 + i, row) = delta;
          s[i] = gl_add(in[i], delta);
          s[i + 4] = gl_sub(in[i + 4], delta);
        }
        for (int i = 8; i < 12; i++) s[i] = in[i];
        for (int r = 0; r < 30; r++) {
          for (int i = 0; i < 12; i++) s[i] = gl_add(s[i], POSEIDON_RC[12 * r + i]);
          if (r >= 4 && r < 26) {
            W(65 + r - 4, row) = s[0];
            s[0] = gl_pow7(s[0]);
          } else {
            if (r) { const int base = r < 4 ? 29 + 12 * (r - 1) : 87 + 12 * (r - 26); for (int i = 0; i < 12; i++) W(base + i, row) = s[i]; }
            for (int i = 0; i < 12; i++) s[i] = gl_pow7(s[i]);
          }
          poseidon_mds_host(s);
        }
        for (int i = 0; i < 12; i++) { W(12 + i, row) = s[i]; vals[t[14 + i]] = s[i]; }
        break;
      }
      default: {  // every other opcode has one body, shared with the device executor (witness_ops.h, witness_gf5.h, witness_wide.h)
        const auto put = [&](u64 col, u64 row, u64 v) { W(col, row) = v; };
        if (!exec_core_op(op, t, vals, put, &P.dom[0][0], &P.bw[0][0]) && !exec_gate_op(op, t, vals, put) && !exec_gf5_op(op, t, vals) &&
            !exec_lut_op(op, t, vals, put, P.lut) && !exec_wide_op(op, t, vals, put)) return;  // refused at create (MP2G_OP_LOOKUP without tables: at run)
        break;
      }
    }
    t += oplen;
  }
#undef W
}
// one proof: vals = scratch of n_slots words, wires = [135][n] (zero-filled here)
void run_one(const mp2g_witness_program& P, const u64* inputs, u64* vals, u64* wires, u32 inner, bool rows) {
  const u64 n = (u64)1 << P.log_n;
  memset(wires, 0, NUM_WIRES * n * sizeof(u64));
  for (size_t i = 0; i < P.consts.size(); i += 2) vals[P.consts[i]] = P.consts[i + 1];
  for (size_t i = 0; i < P.input_sids.size(); i++) vals[P.input_sids[i]] = inputs[i];
  exec(P, P.tape.data(), P.tape.data() + P.tape.size(), vals, wires, inner, rows ? 1 : n, rows ? NUM_WIRES : 1);
  // prove()'s set_lookup_wires: padding, table rows and multiplicities (the twin of the kernel the device replay runs)
  if (P.lut.n_luts) lookup_wires_host(P.lut, wires, rows ? 1 : n, rows ? NUM_WIRES : 1);
}
}  // namespace

extern "C" {
static int witness_program_create(const uint64_t* tape, size_t tape_len, uint32_t n_slots, uint32_t log_n, const uint32_t* input_sids,
                                  uint32_t n_inputs, const uint64_t* const_slots, uint32_t n_consts, mp2g_witness_program** out) {
  NEED(out && (tape || !tape_len) && (input_sids || !n_inputs) && (const_slots || !n_consts), "pointers");
  NEED(log_n >= 1 && log_n <= 20 && n_slots >= 1, "log_n / n_slots");
  mp2g_witness_program* P = new (std::nothrow) mp2g_witness_program();
  if (!P) return fail("out of memory");
  P->tape.assign(tape, tape + tape_len);
  P->input_sids.assign(input_sids, input_sids + n_inputs);
  P->consts.assign(const_slots, const_slots + 2 * (size_t)n_consts);
  P->n_slots = n_slots; P->log_n = log_n;
  const u64 n = (u64)1 << log_n;
  // validate: opcodes, lengths, slot and row / column bounds -- the tape indexes host memory
  auto bad = [&](const char* msg) { delete P; return fail("invalid witness program: %s", msg); };
  for (uint32_t i = 0; i < n_inputs; i++) if (input_sids[i] >= n_slots) return bad("input slot out of range");
  for (uint32_t i = 0; i < n_consts; i++) if (const_slots[2 * i] >= n_slots || const_slots[2 * i + 1] >= GL_P) return bad("constant slot / value");
  const u64* t = P->tape.data();
  const u64* end = t + tape_len;
  const u64* par_end = nullptr;        // end of the parallel region being scanned (regions do not nest)
  std::vector<const u64*> boundaries;  // its section boundaries: each must fall on an instruction start
  size_t next_boundary = 0;
  while (t < end) {
    if (par_end) {
      while (next_boundary < boundaries.size() && t == boundaries[next_boundary]) next_boundary++;
      if (next_boundary < boundaries.size() && t > boundaries[next_boundary]) return bad("a parallel section ends inside an instruction");
      if (t >= par_end) { par_end = nullptr; boundaries.clear(); next_boundary = 0; }
    }
    const u64 op = *t++;
    if ((op < OP_ARITH || op >= OP_END) && !op_is_gf5(op) && !op_is_lut(op) && !op_is_wide(op)) return bad("unknown opcode");
    if (op_is_gf5(op)) P->gf5 = true;
    if (op_is_lut(op)) P->has_lookup = true;
    if (op_is_wide(op)) P->wide = true;
    if (op == OP_PAR && par_end) return bad("parallel regions do not nest");
    const OpShape shape = op_shape(op, t, (size_t)(end - t));
    const u32 len = shape.len;
    if (len == ~0u || len > (size_t)(end - t)) return bad("malformed or truncated instruction");
    if (op == OP_PAR) {
      const u64* body = t + len;
      const u64* b = body;
      for (u32 i = 1; i < len; i++) {
        if (t[i] > (u64)(end - b)) return bad("parallel section length");
        b += t[i];
        boundaries.push_back(b);
      }
      par_end = b;
      next_boundary = 0;
      t += len;
      continue;
    }
    // what is not shape (witness_ops.h op_shape): rows < n, columns, copy and operation indices within the gate, canonical constants
    switch (op) {
      case OP_ARITH: case OP_ARITH_EXT: if (t[0] >= n || t[1] >= (op == OP_ARITH ? 20u : 10u) || t[2] >= GL_P || t[3] >= GL_P) return bad("arithmetic operands"); break;
      case OP_P2: case OP_POSEIDON: case OP_BASE_SUM: case OP_REDUCING: case OP_REDUCING_EXT: case OP_COSET: case OP_EXP: if (t[0] >= n) return bad("row"); break;
      case OP_RA: if (t[0] >= n || t[1] >= RA_COPIES) return bad("random access operands"); break;
      case OP_WIRE: if (t[0] >= n || t[1] >= NUM_WIRES) return bad("wire"); break;
      case OP_HINT_SPLIT: if (t[0] >= n_slots || t[1] < 1 || t[1] > 63) return bad("split hint"); break;
      case OP_U32_ARITH: if (t[0] >= n || t[2] < 1 || t[2] > 3 || t[1] >= t[2]) return bad("U32Arithmetic operands"); break;
      case OP_U32_SUB: if (t[0] >= n || t[2] < 1 || t[2] > 6 || t[1] >= t[2]) return bad("U32Subtraction operands"); break;
      // t[2] is bounded before it is multiplied: the product wraps in 64 bits otherwise (t[3] <= 16 by op_shape)
      case OP_U32_ADD_MANY: if (t[0] >= n || t[2] < 1 || t[2] > NUM_WIRES || t[1] >= t[2] || (t[3] + 3 + 18) * t[2] > NUM_WIRES) return bad("U32AddMany operands"); break;
      case OP_U32_RANGE_CHECK: if (t[0] >= n || t[2] < 1 || t[2] > 7 || t[1] >= t[2]) return bad("U32RangeCheck operands"); break;
      case OP_COMPARISON: {
        if (t[0] >= n || t[1] < 1 || t[1] > 63 || t[2] < 1 || t[2] > 16) return bad("Comparison operands");
        const u64 cb = (t[1] + t[2] - 1) / t[2];
        if (4 + 5 * t[2] + cb + 1 > NUM_WIRES) return bad("Comparison operands");
        break;
      }
      case OP_BASE_SPLIT: if (t[0] >= n || t[1] < 1 || t[1] > 2 || t[1] * t[2] > 63) return bad("BaseSplit operands"); break;
      // the table's own rows are known at mp2g_witness_program_set_lookups, which checks the row against them
      case OP_LOOKUP: if (t[0] >= n || t[1] >= WIT_LU_SLOTS || t[2] >= MP2G_MAX_LUTS) return bad("Lookup operands"); break;
      case OP_MUL_EXT: if (t[0] >= n || t[1] >= 13 || t[2] >= GL_P) return bad("MulExtension operands"); break;
      // 2 ops + 32 ops = 102 and 3 ops + 64 ops = 134 wires at the most (the limb counts of MP2G_OP_BIGUINT_DIV_REM: op_shape)
      case OP_U32_INTERLEAVE: if (t[0] >= n || t[2] < 1 || t[2] > 3 || t[1] >= t[2]) return bad("U32Interleave operands"); break;
      case OP_UNINTERLEAVE_TO_B32: case OP_UNINTERLEAVE_TO_U32: if (t[0] >= n || t[2] < 1 || t[2] > 2 || t[1] >= t[2]) return bad("Uninterleave operands"); break;
      case OP_POSEIDON_MDS: if (t[0] >= n) return bad("row"); break;
      default: break;
    }
    for (u32 i = shape.first_slot; i < len; i++) if (t[i] >= n_slots) return bad("slot out of range");
    t += len;
  }
  for (; par_end && next_boundary < boundaries.size(); next_boundary++)
    if (boundaries[next_boundary] != end) return bad("a parallel section ends inside an instruction");
  for (u32 bits = 2; bits <= 5; bits++) {
    const u32 npts = 1u << bits;
    const u64 w = gl_root_of_unity(bits);
    u64 x = 1;
    for (u32 i = 0; i < npts; i++) { P->dom[bits][i] = x; x = gl_mul(x, w); }
    for (u32 i = 0; i < npts; i++) {
      u64 pr = 1;
      for (u32 j = 0; j < npts; j++) if (j != i) pr = gl_mul(pr, gl_sub(P->dom[bits][i], P->dom[bits][j]));
      P->bw[bits][i] = gl_inv(pr);
    }
  }
  // level schedule for the device executor (witness_dev.hip): level(i) = 1 + max level of the slots i reads
  {
    struct Ins { u32 off, lvl, op; };
    std::vector<Ins> ins;
    std::vector<u32> lvl(n_slots, 0);
    std::vector<uint8_t> written(n_slots, 0), was_read(n_slots, 0);
    for (uint32_t i = 0; i < n_inputs; i++) written[input_sids[i]] = 1;
    for (uint32_t i = 0; i < n_consts; i++) written[const_slots[2 * i]] = 1;
    const u64* base = P->tape.data();
    u32 max_lvl = 0;
    for (const u64* q = base; q < end;) {
      const u64 op = *q;
      const u64* a = q + 1;
      const OpShape sh = op_shape(op, a, (size_t)(end - a));
      if (op == OP_PAR) { q = a + sh.len; continue; }  // the sections follow as ordinary instructions
      u32 l = 0;
      for (u32 i = 0; i < sh.nr; i++) { const u32 sl = (u32)a[sh.r0 + i]; if (lvl[sl] > l) l = lvl[sl]; was_read[sl] = 1; }
      l += 1;
      for (u32 i = 0; i < sh.nw; i++) {
        const u32 sl = (u32)a[sh.w0 + i];
        // a slot written twice, or written after an earlier instruction read it (the host replay saw 0 there): the level
        // schedule would reorder the accesses, so the device replay refuses the program
        if (written[sl] || was_read[sl]) P->ssa = false;
        written[sl] = 1;
        lvl[sl] = l;
      }
      if ((size_t)(q - base) > 0xFFFFFFFFu) return bad("tape too long");
      ins.push_back({(u32)(q - base), l, (u32)op});
      if (l > max_lvl) max_lvl = l;
      q = a + sh.len;
    }
    std::stable_sort(ins.begin(), ins.end(), [](const Ins& x, const Ins& y) { return x.lvl != y.lvl ? x.lvl < y.lvl : x.op < y.op; });
    P->sched.resize(ins.size());
    P->level_off.assign(max_lvl + 1, 0);
    for (size_t i = 0; i < ins.size(); i++) { P->sched[i] = ins[i].off; P->level_off[ins[i].lvl]++; }
    // counts per level (index 1..max_lvl) -> offsets: level l's instructions are sched[level_off[l-1] .. level_off[l])
    u32 acc = 0;
    for (u32 l = 0; l <= max_lvl; l++) { acc += P->level_off[l]; P->level_off[l] = acc; }
    P->level_p2.assign(2 * (size_t)max_lvl, 0);
    for (size_t i = 0; i < ins.size(); i++)
      if (ins[i].op == OP_P2) {
        u32* e = &P->level_p2[2 * (ins[i].lvl - 1)];
        if (!e[1]) e[0] = (u32)i;
        e[1]++;
      }
  }
  *out = P;
  return 0;
}
// no C++ exception crosses the C ABI: allocation and thread-creation failures become error returns
int mp2g_witness_program_create(const uint64_t* tape, size_t tape_len, uint32_t n_slots, uint32_t log_n, const uint32_t* input_sids,
                                uint32_t n_inputs, const uint64_t* const_slots, uint32_t n_consts, mp2g_witness_program** out) {
  try {
    return witness_program_create(tape, tape_len, n_slots, log_n, input_sids, n_inputs, const_slots, n_consts, out);
  } catch (const std::bad_alloc&) {
    return fail("out of memory while building the witness program");
  } catch (...) {
    return fail("witness program creation failed");
  }
}
uint32_t mp2g_witness_program_num_inputs(const mp2g_witness_program* P) { return P ? (uint32_t)P->input_sids.size() : 0; }
uint32_t mp2g_witness_program_num_levels(const mp2g_witness_program* P) { return P && !P->level_off.empty() ? (uint32_t)P->level_off.size() - 1 : 0; }
int mp2g_witness_program_set_probe(mp2g_witness_program* P, const uint32_t* probe_sids, uint32_t n_probe) {
  NEED(P && (probe_sids || !n_probe), "program / probe");
  for (uint32_t i = 0; i < n_probe; i++) NEED(probe_sids[i] < P->n_slots, "probe slot");
  std::lock_guard<std::mutex> g(P->dev_mu);
  NEED(P->dev.empty(), "set the probe before the first device run");
  P->probe.assign(probe_sids, probe_sids + n_probe);
  return 0;
}
static int witness_program_set_lookups(mp2g_witness_program* P, const mp2g_lookup* luts, uint32_t n_luts) {
  NEED(P && (luts || !n_luts) && n_luts <= MP2G_MAX_LUTS, "program / tables (at most MP2G_MAX_LUTS)");
  std::lock_guard<std::mutex> g(P->dev_mu);
  NEED(P->dev.empty(), "set the lookup tables before the first device run");
  const u64 n = (u64)1 << P->log_n;
  LutIndex L{};
  L.n_luts = n_luts; L.lu_slots = WIT_LU_SLOTS; L.lut_slots = WIT_LUT_SLOTS;
  size_t words = 0;
  for (uint32_t t = 0; t < n_luts; t++) {
    const mp2g_lookup& u = luts[t];
    NEED(u.table && u.table_len >= 1 && u.table_len <= LUT_INPUTS, "table (1 .. 65536 entries)");
    NEED(u.last_lu_row < u.last_lut_row && u.last_lut_row <= u.first_lut_row && (u64)u.first_lut_row + 1 < n, "lookup rows");
    NEED((u64)u.first_lut_row - u.last_lut_row + 1 == ((u64)u.table_len + WIT_LUT_SLOTS - 1) / WIT_LUT_SLOTS,
         "the LookupTableGate rows must be ceil(table_len / 26)");
    for (uint32_t o = 0; o < t; o++)
      NEED(u.last_lu_row > luts[o].first_lut_row || u.first_lut_row < luts[o].last_lu_row, "two tables share rows");
    L.last_lu_row[t] = u.last_lu_row; L.last_lut_row[t] = u.last_lut_row; L.first_lut_row[t] = u.first_lut_row; L.table_len[t] = u.table_len;
    words += (size_t)u.table_len * 2;
  }
  std::vector<u32> index;
  NEED(lut_build_index(luts, n_luts, index), "a lookup table holds an input twice");
  // the instructions of a table take the slots 0 .. n_t - 1 of its LookupGate rows, each once
  std::vector<std::vector<uint8_t>> used(n_luts);
  for (uint32_t t = 0; t < n_luts; t++) used[t].assign((size_t)(luts[t].last_lut_row - luts[t].last_lu_row) * WIT_LU_SLOTS, 0);
  const u64* end = P->tape.data() + P->tape.size();
  for (const u64* q = P->tape.data(); q < end;) {
    const u64 op = *q;
    const u64* a = q + 1;
    q = a + op_shape(op, a, (size_t)(end - a)).len;  // validated at create; a parallel region's sections follow its header
    if (op != OP_LOOKUP) continue;
    NEED(a[2] < n_luts, "an MP2G_OP_LOOKUP names a table that was not given");
    const mp2g_lookup& u = luts[a[2]];
    NEED(a[0] >= u.last_lu_row && a[0] < u.last_lut_row, "an MP2G_OP_LOOKUP row outside its table's LookupGate rows");
    uint8_t& slot = used[a[2]][(size_t)(a[0] - u.last_lu_row) * WIT_LU_SLOTS + a[1]];
    NEED(!slot, "two MP2G_OP_LOOKUP instructions use one slot");
    slot = 1;
  }
  for (uint32_t t = 0; t < n_luts; t++) {
    size_t cnt = 0;
    while (cnt < used[t].size() && used[t][cnt]) cnt++;
    for (size_t j = cnt; j < used[t].size(); j++) NEED(!used[t][j], "the MP2G_OP_LOOKUP instructions of a table leave a slot free before a used one");
    L.n_lookups[t] = (u32)cnt;
  }
  P->lut_tables.resize(words);
  P->lut_index.swap(index);
  size_t off = 0;
  for (uint32_t t = 0; t < n_luts; t++) {
    memcpy(P->lut_tables.data() + off, luts[t].table, (size_t)luts[t].table_len * 2 * sizeof(u16));
    L.table[t] = P->lut_tables.data() + off;
    L.index[t] = P->lut_index.data() + (size_t)t * LUT_INPUTS;
    off += (size_t)luts[t].table_len * 2;
  }
  P->lut = L;
  return 0;
}
int mp2g_witness_program_set_lookups(mp2g_witness_program* P, const mp2g_lookup* luts, uint32_t n_luts) {
  try {
    return witness_program_set_lookups(P, luts, n_luts);
  } catch (const std::bad_alloc&) {
    return fail("out of memory while copying the lookup tables");
  } catch (...) {
    return fail("mp2g_witness_program_set_lookups failed");
  }
}
// the program's read-only data on the context's device, uploaded once
static int witness_dev_data(mp2g_witness_program* P, mp2g_ctx* c, WitnessDev** out) {
  std::lock_guard<std::mutex> g(P->dev_mu);
  for (auto* d : P->dev)
    if (d->device == c->device) { *out = d; return 0; }
  WitnessDev* d = new (std::nothrow) WitnessDev();
  if (!d) return fail("out of memory");
  d->device = c->device;
  auto up = [&](DevBuf& b, const void* src, size_t bytes) -> hipError_t {
    hipError_t e = b.alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    return e;
  };
  hipError_t e = up(d->tape, P->tape.data(), P->tape.size() * 8);
  if (e == hipSuccess) e = up(d->sched, P->sched.data(), P->sched.size() * 4);
  if (e == hipSuccess) e = up(d->level_off, P->level_off.data(), P->level_off.size() * 4);
  if (e == hipSuccess) e = up(d->level_p2, P->level_p2.data(), P->level_p2.size() * 4);
  if (e == hipSuccess) e = up(d->input_sids, P->input_sids.data(), P->input_sids.size() * 4);
  if (e == hipSuccess) e = up(d->consts, P->consts.data(), P->consts.size() * 8);
  if (e == hipSuccess) e = up(d->probe, P->probe.data(), P->probe.size() * 4);
  if (e == hipSuccess) {
    std::vector<u64> tab(2 * 6 * 32, 0);
    memcpy(tab.data(), P->dom, sizeof(P->dom));
    memcpy(tab.data() + 6 * 32, P->bw, sizeof(P->bw));
    e = up(d->domtab, tab.data(), tab.size() * 8);
  }
  if (e == hipSuccess && P->lut.n_luts) {
    e = up(d->lut_tables, P->lut_tables.data(), P->lut_tables.size() * sizeof(u16));
    if (e == hipSuccess) e = up(d->lut_index, P->lut_index.data(), P->lut_index.size() * sizeof(u32));
    d->lut = P->lut;
    for (u32 t = 0; t < P->lut.n_luts && e == hipSuccess; t++) {
      d->lut.table[t] = (const u16*)d->lut_tables.p + (P->lut.table[t] - P->lut_tables.data());
      d->lut.index[t] = (const u32*)d->lut_index.p + (size_t)t * LUT_INPUTS;
    }
    if (e == hipSuccess) e = up(d->lut_desc, &d->lut, sizeof(LutIndex));
  }
  if (e != hipSuccess) { delete d; return fail("witness program upload: %s", hipGetErrorString(e)); }
  P->dev.push_back(d);
  *out = d;
  return 0;
}
int mp2g_witness_program_run_dev(mp2g_witness_program* P, mp2g_ctx* c, const uint64_t* d_inputs, uint32_t batch, uint64_t* d_wires,
                                 uint64_t* d_probe_out) {
  NEED(P && c && d_inputs && d_wires && batch >= 1, "program / ctx / inputs / wires");
  NEED(P->probe.empty() || d_probe_out, "probe output");
  if (!P->ssa) return fail("the witness program writes a slot twice, or writes a slot an earlier instruction read: it cannot be level-scheduled for the device");
  NEED(!P->has_lookup || P->lut.n_luts, "the program holds MP2G_OP_LOOKUP: call mp2g_witness_program_set_lookups first");
  WitnessDev* d = nullptr;
  int rc = witness_dev_data(P, c, &d);
  if (rc) return rc;
  const size_t vals_words = (size_t)batch * P->n_slots, wire_words = (size_t)batch * NUM_WIRES << P->log_n;
  if (c->wit_vals.bytes < vals_words * 8 || c->wit_rows.bytes < wire_words * 8) {
    CK(hipStreamSynchronize(c->stream));  // a kernel queued earlier may still use the old buffers
    if (c->wit_vals.bytes < vals_words * 8) CK(c->wit_vals.alloc(vals_words * 8));
    if (c->wit_rows.bytes < wire_words * 8) CK(c->wit_rows.alloc(wire_words * 8));
  }
  CK(hipMemsetAsync(c->wit_vals.p, 0, vals_words * 8, c->stream));
  CK(hipMemsetAsync(c->wit_rows.p, 0, wire_words * 8, c->stream));
  // the executor fills a row-major staging matrix (one contiguous run of words per gate row); the prover's polynomial-major
  // [batch][135][n] is made from it by the tiled transpose (every word of d_wires is written)
  CK((P->wide ? witness_exec_launch_wide : witness_exec_launch)(c->stream, *d, P->gf5, (u32)P->level_off.size() - 1, P->n_slots, P->log_n, (u32)P->input_sids.size(), (u32)(P->consts.size() / 2),
                          (u32)P->probe.size(), (const u64*)d_inputs, batch, c->wit_vals.p, c->wit_rows.p, (u64*)d_probe_out));
  // prove()'s set_lookup_wires on the staging matrix, where a LookupGate row is contiguous (lookup_wires.hip)
  CK(lookup_wires_launch(c->stream, d->lut, c->wit_rows.p, batch, (u64)NUM_WIRES << P->log_n, 1, NUM_WIRES));
  {
    int rc2 = mp2g_wires_from_rows_dev(c, c->wit_rows.p, d_wires, P->log_n, NUM_WIRES, batch);
    if (rc2) return rc2;
  }
  return 0;
}
static int witness_run(const mp2g_witness_program* P, const uint64_t* inputs, uint32_t batch, uint32_t threads, uint64_t* wires,
                       const uint32_t* probe_sids, uint32_t n_probe, uint64_t* probe_out, bool rows) {
  NEED(P && inputs && wires && batch >= 1, "program / inputs / wires");
  NEED(!n_probe || (probe_sids && probe_out), "probe");
  NEED(!P->has_lookup || P->lut.n_luts, "the program holds MP2G_OP_LOOKUP: call mp2g_witness_program_set_lookups first");
  for (uint32_t i = 0; i < n_probe; i++) NEED(probe_sids[i] < P->n_slots, "probe slot");
  const size_t n_in = P->input_sids.size();
  for (size_t i = 0; i < (size_t)batch * n_in; i++) NEED(inputs[i] < GL_P, "inputs must be canonical field elements");
  const size_t per = (size_t)NUM_WIRES << P->log_n;
  if (!threads) threads = std::thread::hardware_concurrency();
  if (!threads) threads = 1;
  // fewer proofs than threads: the spare ones work inside the proofs, on the sections of their parallel regions
  const uint32_t inner = threads > batch ? (threads / batch > 16 ? 16 : threads / batch) : 1;  // 16: past that the thread starts cost more than they save
  if (threads > batch) threads = batch;
  std::atomic<uint32_t> next{0};
  auto worker = [&]() {
    std::vector<u64> vals(P->n_slots);
    for (;;) {
      const uint32_t b = next.fetch_add(1);
      if (b >= batch) return;
      std::fill(vals.begin(), vals.end(), 0);
      run_one(*P, inputs + (size_t)b * n_in, vals.data(), wires + (size_t)b * per, inner, rows);
      for (uint32_t i = 0; i < n_probe; i++) probe_out[(size_t)b * n_probe + i] = vals[probe_sids[i]];
    }
  };
  std::atomic<int> failed{0};
  auto guarded = [&]() {
    try { worker(); } catch (...) { failed.store(1); }  // bad_alloc of a slot table / an inner pool: report, do not terminate
  };
  std::vector<std::thread> pool;
  try {
    for (uint32_t i = 1; i < threads; i++) pool.emplace_back(guarded);
  } catch (...) {
    // the host refuses more threads: go on with the ones that started (the work queue is shared)
  }
  guarded();
  for (auto& th : pool) th.join();
  if (failed.load()) return fail("witness replay: out of memory or thread creation failed");
  return 0;
}
int mp2g_witness_program_run(const mp2g_witness_program* P, const uint64_t* inputs, uint32_t batch, uint32_t threads, uint64_t* wires,
                             const uint32_t* probe_sids, uint32_t n_probe, uint64_t* probe_out) {
  return witness_run(P, inputs, batch, threads, wires, probe_sids, n_probe, probe_out, false);
}
int mp2g_witness_program_run_rows(const mp2g_witness_program* P, const uint64_t* inputs, uint32_t batch, uint32_t threads, uint64_t* rows,
                                  const uint32_t* probe_sids, uint32_t n_probe, uint64_t* probe_out) {
  return witness_run(P, inputs, batch, threads, rows, probe_sids, n_probe, probe_out, true);
}
void mp2g_witness_program_free(mp2g_witness_program* P) { delete P; }
}  // extern "C"
