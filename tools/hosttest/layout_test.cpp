// Host-side check of csrc/layout.h: the flat FRI proof's sections are contiguous and in the order of include/mp2g.h, the opening
// offsets enumerate the openings exactly once and agree with fri_batch_poly, the parts of a proof add up.
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -I../../mapreduce-plonky2_amd/csrc -I../../include layout_test.cpp -o layout_test
// run:   layout_test num_constants n_public_inputs <the 27 words of mp2g_fri_params>; prints "proof_words N n_open M bad K"
#include "fri.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace mp2g;
int main(int argc, char** argv) {
  static_assert(sizeof(mp2g_fri_params) == 27 * sizeof(uint32_t), "mp2g_fri_params is 27 words");
  if (argc != 3 + 27) return 2;
  const u32 num_constants = (u32)strtoul(argv[1], nullptr, 10), n_pi = (u32)strtoul(argv[2], nullptr, 10);
  uint32_t words[27];
  for (int i = 0; i < 27; i++) words[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
  mp2g_fri_params P;
  memcpy(&P, words, sizeof P);
  long bad = 0;
#define CHECK(c) do { if (!(c)) { bad++; fprintf(stderr, "failed: %s\n", #c); } } while (0)
  const FriProofLayout L = fri_proof_layout(P);
  const u32 lg = P.log_n + P.rate_bits;
  CHECK(L.lg == lg && L.capw == (4u << P.cap_height) && L.n_paths == P.n_oracles + P.n_layers);
  // caps of the layers | queries | final polynomial | proof-of-work witness
  CHECK(L.q_off == P.n_layers * L.capw);
  CHECK(L.final_off == L.q_off + (u64)P.num_queries * L.q_words);
  CHECK(L.pow_off == L.final_off + 2 * L.final_len);
  CHECK(L.final_off + 2 * (u64)L.final_len + 1 == L.proof_words);
  // a query: per oracle {leaf, siblings}, then per layer {evals, siblings}
  u32 clg = lg, shift = 0, deg = P.log_n;
  CHECK(L.leaf_off[0] == 0);
  for (u32 p = 0; p < L.n_paths; p++) {
    if (p < P.n_oracles) {
      CHECK(L.leaf_len[p] == P.oracle_w[p]);
    } else {
      const u32 ab = P.arity_bits[p - P.n_oracles];
      clg -= ab; shift += ab; deg -= ab;
      CHECK(L.leaf_len[p] == 2u << ab);
    }
    CHECK(L.n_sib[p] == clg - P.cap_height && L.x_shift[p] == shift);
    const u32 end = L.leaf_off[p] + L.leaf_len[p] + 4 * L.n_sib[p];
    if (p + 1 < L.n_paths) CHECK(L.leaf_off[p + 1] == end);
    else CHECK(L.q_words == end);
  }
  CHECK(L.final_len == 1u << deg);

  const OpeningLayout O = opening_layout(P, num_constants);
  const FriShape sh = fri_shape(P);
  std::vector<int> seen(O.n_open, 0);
  CHECK(O.n_zeta == fri_batch_len(sh, 0) && O.n_open == O.n_zeta + fri_batch_len(sh, 1));
  for (u32 batch = 0; batch < 2; batch++)
    for (u32 j = 0; j < fri_batch_len(sh, batch); j++) {
      u32 o, p;
      fri_batch_poly(sh, batch, j, o, p);
      const bool lookup = o == P.zs_oracle && p >= O.oracle[o].len;  // one of the oracle's trailing lookup polynomials
      u32 at;
      if (batch == 0) at = lookup ? O.lookup + (p - O.oracle[o].len) : O.oracle[o].off + p;
      else at = lookup ? O.lookup_next + (p - O.oracle[o].len) : O.zs_next + p;
      CHECK(o == P.zs_oracle || batch == 0);
      CHECK(at == (batch ? O.n_zeta : 0) + j);
      if (at < O.n_open) seen[at]++;
    }
  for (u32 i = 0; i < O.n_open; i++) CHECK(seen[i] == 1);
  CHECK(O.constants == 0 && O.sigmas == num_constants && O.wires == O.oracle[1].off && O.quotient == O.oracle[3].off);
  CHECK(O.zs == O.oracle[P.zs_oracle].off && O.partial_products == O.zs + P.zs_count);
  CHECK(O.n_lookup == P.zs_count * P.num_lookup_polys && O.lookup_next == O.zs_next + P.zs_count);
  for (u32 o = 0; o + 1 < 8; o++) CHECK(O.oracle[o + 1].off == O.oracle[o].off + O.oracle[o].len);
  CHECK(O.lookup == O.oracle[7].off + O.oracle[7].len);

  const ProofParts T = proof_parts(P, n_pi);
  CHECK(T.n[0] == n_pi && T.n[1] == (P.n_oracles - 1) * L.capw && T.n[2] == 2 * O.n_open && T.n[3] == L.proof_words);
  CHECK(T.off[0] == 0 && T.words == T.off[3] + T.n[3]);
  for (int k = 0; k < 3; k++) CHECK(T.off[k + 1] == T.off[k] + T.n[k]);
  printf("proof_words %llu n_open %u bad %ld\n", (unsigned long long)L.proof_words, O.n_open, bad);
  return bad != 0;
}
