// Witness generation on the device for circuits built by recursion.py: the executor of csrc/witness.hip as a kernel.
//
// Replaces [dep] plonky2 iop/generator.rs generate_partial_witness (first line of prove(), recursion-framework/src/
// circuit_builder.rs:308, universal_verifier_gadget/wrap_circuit.rs:143) for a BATCH of proofs of one circuit without the host:
// the recorded witness program is data independent and the same for every proof, so it is scheduled once (witness.hip:
// dependency levels; ~300 levels for a 10-20 k instruction verifier circuit, the long ones being the Merkle paths and leaf
// hashes of the 28 FRI query rounds) and replayed by one 512-lane block per proof: at every level lane i takes the level's
// i-th instruction (instructions of a level are ordered by opcode so that waves stay uniform), one block barrier between
// levels. Values live in a per-proof slot table in global memory (written once each: SSA), wires go into a row-major staging
// matrix [B][n][135] (a gate row's wires are one contiguous run) that witness.hip transposes into the prover's [B][135][n]. Arithmetic is gl.cuh / poseidon.cuh: the Poseidon2 gate's S-box inputs are the weak
// representatives of the sponge kernels, canonicalised where they become wires.
//
// This file is compiled TWICE: as itself, and from witness_dev_wide.hip with MP2G_WITNESS_WIDE set, which gives the instances that
// also carry the wide block (include/mp2g.h enum mp2g_witness_op_wide, witness_wide.h) under names of their own
// (witness_exec_kernel_wide, witness_exec_launch_wide). The wide instances sit in an object of their own so that this one --
// code, layout and the PC-relative addresses of its constants -- is what it was before they existed.
#ifndef MP2G_WITNESS_WIDE
#define MP2G_WITNESS_WIDE 0
#endif
#include "gl.cuh"
#include "poseidon.cuh"
#include "poseidon_wave.cuh"
#include "witness.h"
#include "witness_ops.h"
#include "witness_gf5.h"
#if MP2G_WITNESS_WIDE
#include "witness_wide.h"
#define witness_exec_kernel witness_exec_kernel_wide
#define witness_exec_launch witness_exec_launch_wide
#endif

namespace mp2g {
namespace {
// wires: this proof's staging matrix in ROW-major order [n][135] (a gate row's wires are consecutive words: a Poseidon2 row's 135 stores
// touch 17 sectors instead of 135; witness.hip transposes the batch into the prover's polynomial-major layout afterwards)
#define W(col, row) wires[(u64)(row) * NUM_WIRES + (u64)(col)]

GLD void exec_p2(const u64* t, u64* vals, u64* wires, u64 n) {
  // Poseidon2Gate: inputs 0..11, outputs 12..23, swap 24, deltas 25..28, S-box inputs 29.., 65.., 87..
  const u64 row = t[0];
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 12; i++) { s[i] = vals[t[1 + i]]; W(i, row) = s[i]; }
  const u64 swap = vals[t[13]];
  W(24, row) = swap;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const u64 delta = gl_mul(swap, gl_sub(s[i + 4], s[i]));
    W(25 + i, row) = delta;
    s[i] = gl_add(s[i], delta);
    s[i + 4] = gl_sub(s[i + 4], delta);
  }
  p2_external(s);
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
      s[i] = gl_canon(gl_addw(s[i], c_p2_ext[12 * r + i]));
      if (r) W(29 + 12 * (r - 1) + i, row) = s[i];
      s[i] = p2_sbox0(s[i]);
    }
    p2_external(s);
  }
#pragma unroll 1
  for (int r = 0; r < 22; r++) {
    const u64 x = gl_canon(gl_addw(s[0], c_p2_int[r]));
    W(65 + r, row) = x;
    s[0] = p2_sbox0(x);
    p2_internal(s);
  }
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
      s[i] = gl_canon(gl_addw(s[i], c_p2_ext[12 * (4 + r) + i]));
      W(87 + 12 * r + i, row) = s[i];
      s[i] = p2_sbox0(s[i]);
    }
    p2_external(s);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) { const u64 o = gl_canon(s[i]); W(12 + i, row) = o; vals[t[14 + i]] = o; }
}

// The same gate with its state spread over lanes 0..11 of an aligned 16-lane group (poseidon_wave.cuh): a level that holds only a
// few Poseidon2 rows -- the Fiat-Shamir chain, the upper part of a Merkle path -- is a chain of dependent permutations, and one
// permutation takes a lone lane ~45 us but a 12-lane group ~12 us. Every lane of the group calls; l = lane & 15.
GLD void exec_p2_coop(const u64* t, u64* vals, u64* wires, u64 n, int l) {
  const u64 row = t[0];
  const bool on = l < 12;
  const int li = on ? l : 0;
  u64 x = on ? vals[t[1 + li]] : 0;
  if (on) W(l, row) = x;
  const u64 swap = vals[t[13]];
  if (l == 0) W(24, row) = swap;
  {  // the swap of inputs[0..4) and [4..8): delta_i = swap (in[i + 4] - in[i]), lanes i and i + 4 both form it
    const u64 other = wp_shfl(x, (l ^ 4) & 15);
    const u64 lo_v = l < 4 ? x : other, hi_v = l < 4 ? other : x;
    const u64 delta = gl_mul(swap, gl_sub(hi_v, lo_v));
    if (l < 4) { W(25 + l, row) = delta; x = gl_add(x, delta); }
    else if (l < 8) x = gl_sub(x, delta);
  }
  u64 rc[8];
#pragma unroll
  for (int r = 0; r < 8; r++) rc[r] = c_p2_ext[12 * r + li];
  const u64 d = c_p2_diag[li];
  x = wp2_external(x, l);
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
    const u64 k = r == 0 ? rc[0] : (r == 1 ? rc[1] : (r == 2 ? rc[2] : rc[3]));
    const u64 in = gl_canon(gl_addw(x, k));
    if (r && on) W(29 + 12 * (r - 1) + l, row) = in;
    x = wp2_external(p2_sbox0(in), l);
  }
#pragma unroll 1
  for (int r = 0; r < 22; r++) {
    const u64 in = gl_canon(gl_addw(x, c_p2_int[r]));
    if (l == 0) W(65 + r, row) = in;
    x = wp2_internal(l == 0 ? p2_sbox0(in) : x, l, d);
  }
#pragma unroll 1
  for (int r = 4; r < 8; r++) {
    const u64 k = r == 4 ? rc[4] : (r == 5 ? rc[5] : (r == 6 ? rc[6] : rc[7]));
    const u64 in = gl_canon(gl_addw(x, k));
    if (on) W(87 + 12 * (r - 4) + l, row) = in;
    x = wp2_external(p2_sbox0(in), l);
  }
  if (on) { const u64 o = gl_canon(x); W(12 + l, row) = o; vals[t[14 + l]] = o; }
}

GLD void exec_poseidon(const u64* t, u64* vals, u64* wires, u64 n) {
  // PoseidonGate ([dep] gates/poseidon.rs): the wire layout of the Poseidon2 gate, the original permutation (4 + 22 + 4 rounds)
  const u64 row = t[0];
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 12; i++) { s[i] = vals[t[1 + i]]; W(i, row) = s[i]; }
  const u64 swap = vals[t[13]];
  W(24, row) = swap;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const u64 delta = gl_mul(swap, gl_sub(s[i + 4], s[i]));
    W(25 + i, row) = delta;
    s[i] = gl_add(s[i], delta);
    s[i + 4] = gl_sub(s[i + 4], delta);
  }
#pragma unroll 1
  for (int r = 0; r < 30; r++) {
    if (r >= 4 && r < 26) {
#pragma unroll
      for (int i = 1; i < 12; i++) s[i] = gl_addw(s[i], c_p_rc[12 * r + i]);
      const u64 x = gl_canon(gl_addw(s[0], c_p_rc[12 * r]));
      W(65 + r - 4, row) = x;
      s[0] = p2_sbox0(x);
    } else {
      const int base = r < 4 ? 29 + 12 * (r - 1) : 87 + 12 * (r - 26);
#pragma unroll
      for (int i = 0; i < 12; i++) {
        const u64 x = gl_canon(gl_addw(s[i], c_p_rc[12 * r + i]));
        if (r) W(base + i, row) = x;
        s[i] = p2_sbox0(x);
      }
    }
    poseidon_mds(s);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) { const u64 o = gl_canon(s[i]); W(12 + i, row) = o; vals[t[14 + i]] = o; }
}

template <bool GF5, bool LUT>
GLD void exec_one(const u64* t, u64* vals, u64* wires, u64 n, const u64* domtab, const LutIndex* lut) {
  const u64 op = *t++;
  switch (op) {
    case OP_P2: exec_p2(t, vals, wires, n); break;
    case OP_POSEIDON: exec_poseidon(t, vals, wires, n); break;
    default: {  // every other opcode has one body, shared with the host executor (witness_ops.h, witness_gf5.h, witness_wide.h);
                // anything else was refused at create
      const auto put = [wires](u64 col, u64 row, u64 v) { W(col, row) = v; };
      if (exec_core_op(op, t, vals, put, domtab, domtab + 6 * 32)) break;
      if constexpr (GF5) {
        if (exec_gf5_op(op, t, vals)) break;
      }
      if constexpr (LUT) {
        if (exec_lut_op(op, t, vals, put, *lut)) break;
      }
#if MP2G_WITNESS_WIDE
      if (exec_wide_op(op, t, vals, put)) break;
#endif
      exec_gate_op(op, t, vals, put);
      break;
    }
  }
}
#undef W

constexpr int WIT_LANES = 512;
// GF5: the program holds GF(p^5) opcodes. Only that instance carries their code (the field's square root and inverse are long
// out-of-line bodies); a tape without them runs the instance that is the kernel as it was before they existed. LUT: the same for
// MP2G_OP_LOOKUP, whose tables `lut` describes (device memory). The wide block is the third such flag, MP2G_WITNESS_WIDE of the
// head of this file: its divisions keep multi-limb integers per lane, MP2G_OP_BIGUINT_DIV_REM in private memory.
template <bool GF5, bool LUT>
__global__ void __launch_bounds__(WIT_LANES) witness_exec_kernel(const u64* __restrict__ tape, const u32* __restrict__ sched,
                                                                const u32* __restrict__ level_off, const u32* __restrict__ level_p2, u32 n_levels, u32 n_slots, u32 log_n,
                                                                const u32* __restrict__ input_sids, u32 n_inputs, const u64* __restrict__ consts,
                                                                u32 n_consts, const u64* __restrict__ domtab, const u32* __restrict__ probe,
                                                                u32 n_probe, const u64* __restrict__ inputs, u64* vals_all, u64* wires_all,
                                                                u64* probe_out, const LutIndex* __restrict__ lut) {
  const u32 b = blockIdx.x, tid = threadIdx.x;
  const u64 n = (u64)1 << log_n;
  u64* vals = vals_all + (u64)b * n_slots;
  u64* wires = wires_all + (u64)b * NUM_WIRES * n;
  for (u32 i = tid; i < n_consts; i += WIT_LANES) vals[consts[2 * i]] = consts[2 * i + 1];
  for (u32 i = tid; i < n_inputs; i += WIT_LANES) vals[input_sids[i]] = inputs[(u64)b * n_inputs + i];
  __syncthreads();
  for (u32 l = 0; l < n_levels; l++) {
    const u32 lo = level_off[l], hi = level_off[l + 1];
    const u32 p2_lo = level_p2[2 * l], p2_n = level_p2[2 * l + 1];  // the level's Poseidon2 rows are sched[p2_lo .. p2_lo + p2_n)
    if (p2_n && p2_n * 16 <= 2 * WIT_LANES) {
      // few Poseidon2 rows: one 16-lane group each (latency; up to two rounds of groups: 2 x ~23 us against ~62 us one lane per
      // row), the level's other instructions one lane each
      for (u32 g = tid >> 4; g < p2_n; g += WIT_LANES / 16) exec_p2_coop(tape + sched[p2_lo + g] + 1, vals, wires, n, (int)(tid & 15));
      const u32 rest = (hi - lo) - p2_n;
      for (u32 i = tid; i < rest; i += WIT_LANES) {
        const u32 j = lo + i;
        exec_one<GF5, LUT>(tape + sched[j < p2_lo ? j : j + p2_n], vals, wires, n, domtab, lut);
      }
    } else {
      for (u32 i = lo + tid; i < hi; i += WIT_LANES) exec_one<GF5, LUT>(tape + sched[i], vals, wires, n, domtab, lut);
    }
    __syncthreads();  // the level's slot writes (global memory, this block's) are visible to the next level's reads
  }
  for (u32 i = tid; i < n_probe; i += WIT_LANES) probe_out[(u64)b * n_probe + i] = vals[probe[i]];
}
}  // namespace

hipError_t witness_exec_launch(hipStream_t s, const WitnessDev& d, bool gf5, u32 n_levels, u32 n_slots, u32 log_n, u32 n_inputs,
                               u32 n_consts, u32 n_probe, const u64* d_inputs, u32 batch, u64* d_vals, u64* d_wires, u64* d_probe_out) {
  const bool lut = d.lut.n_luts != 0;
  const auto kernel = lut ? (gf5 ? witness_exec_kernel<true, true> : witness_exec_kernel<false, true>)
                          : (gf5 ? witness_exec_kernel<true, false> : witness_exec_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(batch), dim3(WIT_LANES), 0, s, d.tape.p, (const u32*)d.sched.p, (const u32*)d.level_off.p,
                     (const u32*)d.level_p2.p, n_levels, n_slots, log_n, (const u32*)d.input_sids.p, n_inputs, d.consts.p, n_consts, d.domtab.p,
                     (const u32*)d.probe.p, n_probe, d_inputs, d_vals, d_wires, d_probe_out, lut ? (const LutIndex*)d.lut_desc.p : nullptr);
  return hipGetLastError();
}
}  // namespace mp2g
