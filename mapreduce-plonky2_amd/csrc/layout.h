// The ONE definition of where a proof's words lie (include/mp2g.h describes the same layout in prose). Writers (fri.hip's query
// kernel, prover.hip, chain.hip, forest.hip) and readers (verifier.hip, wire.hip) take their offsets from here; nothing else
// does index arithmetic on a proof. Plain structs, passed to kernels by value; the functions rely on params_check (ctx.h)
// having accepted the parameters, which bounds every subtraction below.
//
//   flat FRI proof   caps of the n_layers commit-phase trees | num_queries x { per oracle: leaf, siblings; per layer: evals,
//                    siblings } | final polynomial (2 words a coefficient) | proof-of-work witness
//   openings         2 words each, in FRI batch order (fri_batch_poly): at zeta every polynomial in oracle order except the lookup
//                    polynomials, which come last; at g zeta the Z polynomials, then the lookup polynomials. For plonky2's four
//                    oracles: constants, sigmas | wires | Z, partial products | quotient chunks | lookup | Z next | lookup next
//   a proof in a parent's input order   public inputs | caps of oracles 1.. | openings | flat FRI proof
#pragma once
#include "gl.cuh"
#include "mp2g.h"

namespace mp2g {

#define MP2G_MAX_PATHS 16  // Merkle paths of a query: n_oracles <= 8 initial trees, then n_layers <= 8 commit-phase trees

struct FriProofLayout {
  u32 lg, capw;  // log2 of the LDE size; words of one cap
  u32 n_paths, final_len;
  u32 q_off, q_words, final_off, pow_off;  // query r starts at q_off + r * q_words
  u64 proof_words;  // the 32-bit offsets above are exact for every proof of less than 2^32 words (who stores proofs checks that)
  // path p of a query, relative to the query's start: leaf_len words of leaf (an oracle's row / a layer's 2 * arity evaluation
  // words), then n_sib siblings of 4 words; the path's leaf index is the query index >> x_shift
  u32 leaf_off[MP2G_MAX_PATHS], leaf_len[MP2G_MAX_PATHS], n_sib[MP2G_MAX_PATHS], x_shift[MP2G_MAX_PATHS];
};
GLHD FriProofLayout fri_proof_layout(const mp2g_fri_params& P) {
  FriProofLayout L{};
  L.lg = P.log_n + P.rate_bits;
  L.capw = 4u << P.cap_height;
  L.n_paths = P.n_oracles + P.n_layers;
  u64 off = 0;
  u32 clg = L.lg, shift = 0, deg = P.log_n;
  for (u32 p = 0; p < L.n_paths && p < MP2G_MAX_PATHS; p++) {
    if (p >= P.n_oracles) {
      const u32 ab = P.arity_bits[p - P.n_oracles];
      clg -= ab; shift += ab; deg -= ab;
    }
    L.leaf_off[p] = (u32)off;
    L.leaf_len[p] = p < P.n_oracles ? P.oracle_w[p] : 2u << P.arity_bits[p - P.n_oracles];
    L.n_sib[p] = clg - P.cap_height;
    L.x_shift[p] = shift;
    off += (u64)L.leaf_len[p] + 4 * L.n_sib[p];
  }
  L.final_len = 1u << deg;
  L.q_off = P.n_layers * L.capw;
  L.q_words = (u32)off;
  L.final_off = L.q_off + P.num_queries * L.q_words;
  L.pow_off = L.final_off + 2 * L.final_len;
  L.proof_words = (u64)L.q_off + P.num_queries * off + 2 * (u64)L.final_len + 1;
  return L;
}

// FRI batch order (plonk/circuit_data.rs fri_all_polys / fri_next_batch_polys; also the order of the flat openings and of the
// transcript, OpeningSet::to_fri_openings). `sh` is anything with n_oracles, n_polys, zs_oracle, zs_count, lookup_count and
// o[].w: the kernels' FriShape (fri.h).
template <class Shape>
GLHD u32 fri_batch_len(const Shape& sh, u32 batch) { return batch ? sh.zs_count + sh.lookup_count : sh.n_polys; }
template <class Shape>
GLHD void fri_batch_poly(const Shape& sh, u32 batch, u32 j, u32& o, u32& p) {
  const u32 zo = sh.zs_oracle, wz = sh.o[zo].w - sh.lookup_count;
  if (batch) { o = zo; p = j < sh.zs_count ? j : wz + (j - sh.zs_count); return; }
  for (u32 oi = 0; oi < sh.n_oracles; oi++) {
    const u32 w = oi == zo ? wz : sh.o[oi].w;
    if (j < w) { o = oi; p = j; return; }
    j -= w;
  }
  o = zo; p = wz + j;
}
// The same order as offsets into the flat openings (in openings, i.e. pairs of words).
struct OpeningLayout {
  u32 n_open, n_zeta;  // all openings; those at zeta
  struct { u32 off, len; } oracle[8];  // oracle o at zeta (the zs oracle without its lookup polynomials); empty if the proof lacks it
  // plonky2's names for them (oracle 0 = constants, sigmas; 1 = wires; 2 = Z, partial products; 3 = quotient chunks)
  static constexpr u32 constants = 0;
  u32 sigmas, wires, zs, partial_products, quotient, lookup, zs_next, lookup_next;
  u32 n_lookup;  // zs_count * num_lookup_polys
};
GLHD OpeningLayout opening_layout(const mp2g_fri_params& P, u32 num_constants) {
  OpeningLayout L{};
  L.n_lookup = P.zs_count * P.num_lookup_polys;
  u32 off = 0;
  for (u32 o = 0; o < 8; o++) {
    L.oracle[o].off = off;
    L.oracle[o].len = o < P.n_oracles ? P.oracle_w[o] - (o == P.zs_oracle ? L.n_lookup : 0) : 0;
    off += L.oracle[o].len;
  }
  L.sigmas = num_constants; L.wires = L.oracle[1].off;
  L.zs = L.oracle[P.zs_oracle & 7].off; L.partial_products = L.zs + P.zs_count; L.quotient = L.oracle[3].off;
  L.lookup = off;
  L.n_zeta = L.lookup + L.n_lookup;
  L.zs_next = L.n_zeta;
  L.lookup_next = L.zs_next + P.zs_count;
  L.n_open = L.lookup_next + L.n_lookup;
  return L;
}

// A proof as one run of words, in the order a parent circuit takes it as witness inputs (plonky2's ProofWithPublicInputsTarget)
struct ProofParts {
  u32 n[4];    // words of: public inputs | caps of oracles 1.. | openings | flat FRI proof
  u64 off[4];  // where each starts
  u64 words;
  u32 capw;  // words of one cap
};
GLHD ProofParts proof_parts(const mp2g_fri_params& P, u32 n_public_inputs) {
  ProofParts T{};
  T.n[0] = n_public_inputs;
  T.capw = 4u << P.cap_height;
  T.n[1] = (P.n_oracles - 1) * T.capw;
  T.n[2] = 2 * opening_layout(P, 0).n_open;
  T.n[3] = (u32)fri_proof_layout(P).proof_words;
  for (int k = 0; k < 4; k++) { T.off[k] = T.words; T.words += T.n[k]; }
  return T;
}

// plonk/prover.rs, get_challenges.rs: how many challenges the transcript draws after observing the cap of oracle o. Wires cap ->
// num_challenges betas, then as many gammas (with lookups: twice that, the deltas); Z / partial products cap -> num_challenges
// alphas; every other cap -> none. The prover and the verifier must agree on this or every proof is rejected.
GLHD u32 plonk_challenges_after_cap(u32 o, u32 num_challenges, bool has_lookup) {
  return o == 1 ? (has_lookup ? 4 : 2) * num_challenges : o == 2 ? num_challenges : 0;
}
}  // namespace mp2g
