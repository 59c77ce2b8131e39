// Launchers of the gate-constraint kernels (gates.hip).
#pragma once
#include <stdio.h>
#include "gate_shape.h"
#include "gl.cuh"
namespace mp2g {
struct GateTable {
  u32 n_gates, num_selectors;
  u32 num_lookup_selectors;  // 0, or 4 + n_luts constants between the selectors and the gate constants
  mp2g_gate g[MP2G_MAX_GATES];
};
// validates a table against the wire and constant counts of its circuit (the kinds and their parameters: gate_shape); returns
// nullptr or a message, which names the offending gate by index and kind and stays valid until the thread's next call.
// max_j (may be NULL): the largest constraint count of a gate
inline const char* gate_table_check(const GateTable& t, u32 num_constants, u32 wires_w, u32* max_j = nullptr) {
  if (t.n_gates > MP2G_MAX_GATES) return "too many gates";
  if (t.num_selectors == 0 || t.num_selectors > num_constants) return "num_selectors must be in 1..num_constants";
  u32 mj = 0;
  for (u32 i = 0; i < t.n_gates; i++) {
    const mp2g_gate& g = t.g[i];
    const GateShape sh = gate_shape(g);
    const char* msg = sh.err;
    if (msg) {}
    else if (sh.wires > wires_w) msg = "gate needs more wires than the wires oracle has";
    else if ((u64)t.num_selectors + t.num_lookup_selectors + sh.consts > num_constants) msg = "gate needs more constants than the preprocessed oracle has";
    else if (g.selector_index >= t.num_selectors) msg = "selector_index out of range";
    else if (!(g.group_start <= i && i < g.group_end && g.group_end <= t.n_gates)) msg = "gate is not inside its selector group";
    else if (sh.constraints > MP2G_MAX_GATE_CONSTRAINTS) msg = "gate has too many constraints";
    if (msg) {
      static thread_local char named[192];
      snprintf(named, sizeof named, "gate %u (kind %u): %s", i, g.kind, msg);
      return named;
    }
    if (sh.constraints > mj) mj = sh.constraints;
  }
  if (max_j) *max_j = mj;
  return nullptr;
}
// the table of a caller's gate array (n_gates <= MP2G_MAX_GATES), validated when it has gates: the message of gate_table_check
// or nullptr, and max_j (may be NULL) from the shapes it validated
inline const char* gate_table_make(const mp2g_gate* gates, u32 n_gates, u32 num_selectors, u32 num_lookup_selectors, u32 num_constants,
                                   u32 wires_w, GateTable& out, u32* max_j) {
  out = GateTable{};
  out.n_gates = n_gates; out.num_selectors = num_selectors; out.num_lookup_selectors = num_lookup_selectors;
  for (u32 i = 0; i < n_gates; i++) out.g[i] = gates[i];
  if (max_j) *max_j = 0;
  return n_gates ? gate_table_check(out, num_constants, wires_w, max_j) : nullptr;
}
// q[b][a][i] (natural order i) = sum_g filter_g sum_j alpha_a^j c_{g,j} at the LDE point of memory column
// p = bitrev(i): C / W are the bit-reversed LDE value matrices [.][N] of the constants (shared) and the
// wires (per proof), N = 8n. quotient_perm_values(..., gates = true) folds q into the vanishing sum.
// apw: the batch's alpha powers [B][2][MP2G_MAX_GATE_CONSTRAINTS] (alpha_powers).
hipError_t gate_constraints_lde(hipStream_t s, u32 B, const GateTable& t, const u64* C, const u64* W, u64 w_bstride, u32 lg,
                                const u64* apw, u32 nc, const u64* pi_hash, u64* q);
// apw[b][a][e] = alpha_a^e for the nc <= 2 challenges alphas[b * al_bstride + a] (0 for a >= nc), e < MP2G_MAX_GATE_CONSTRAINTS:
// the powers every alpha-reduction of the quotient reads (gate_constraints_lde, quotient_perm_values)
hipError_t alpha_powers(hipStream_t s, u32 B, const u64* alphas, u64 al_bstride, u32 nc, u64* apw);
// out[b][j][p] = C_j at point p of proof b (device pointers), B proofs with npts points each: consts / wires of proof b at
// b * c_bstride / b * w_bstride ([.][npts] each), out [B][max_j][npts], pi_hash [B][4]
hipError_t gate_constraints_points_batch(hipStream_t s, u32 B, const GateTable& t, const u64* consts, u64 c_bstride, const u64* wires,
                                         u64 w_bstride, u32 npts, u32 max_j, const u64* pi_hash, u64* out);
// the same for one set of points
hipError_t gate_constraints_points(hipStream_t s, const GateTable& t, const u64* consts, const u64* wires, u32 npts, u32 max_j,
                                   const u64* pi_hash, u64* out);
// flags[b] |= 2 where a gate constraint of proof b is non-zero on the subgroup: consts [.][npts] (shared),
// wires [B][.][npts] with batch stride w_bstride, pi_hash [B][4]
hipError_t gate_check(hipStream_t s, u32 B, const GateTable& t, const u64* consts, const u64* wires, u64 w_bstride, u64 npts,
                      const u64* pi_hash, u32* flags);
}  // namespace mp2g
