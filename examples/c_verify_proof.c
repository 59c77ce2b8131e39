/* Plain-C client of the device verifier: prove a small gate-level circuit as c_prove_circuit.c does, verify the proof where the
 * prover left it on the device (mp2g_verifier_verify_dev), flip one opening word, verify again, print both statuses: "status=0"
 * then a non-zero code (the PLONK identity fails: 10 or 11). What a Rust host does instead of keeping plonky2's CPU verifier around
 * for proofs it has just made on the GPU (VerifierCircuitData::verify).
 *
 * The circuit file is the one tests/test_gpu_c_abi.py writes for c_prove_circuit (layout: see there). The verifier's
 * constants_sigmas cap is taken from a commitment to the preprocessed polynomials (mp2g_commit_from_values).
 * build: gcc -std=c11 -Wall -Iinclude examples/c_verify_proof.c -Lmapreduce-plonky2_amd -lmp2gpu -o examples/c_verify_proof */
#include "mp2g.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if ((x) != 0) { fprintf(stderr, "%s failed: %s\n", #x, mp2g_last_error()); return 1; } } while (0)
#define READ(ptr, count) do { if (fread((ptr), sizeof *(ptr), (count), f) != (size_t)(count)) { fprintf(stderr, "short read\n"); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s circuit.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t hdr[8];
  READ(hdr, 8);
  const uint32_t log_n = hdr[0], num_constants = hdr[1], num_routed = hdr[2], wires_w = hdr[3], n_gates = hdr[4], num_selectors = hdr[5];
  const size_t n = (size_t)1 << log_n;
  mp2g_gate gates[MP2G_MAX_GATES];
  if (n_gates > MP2G_MAX_GATES) return 2;
  READ(gates, n_gates);
  uint64_t pi_hash[4], digest[4];
  READ(pi_hash, 4);
  READ(digest, 4);
  const size_t pre_words = (size_t)(num_constants + num_routed) * n, wire_words = (size_t)wires_w * n;
  uint64_t* pre = malloc(pre_words * 8);
  uint64_t* wires = malloc(wire_words * 8);
  READ(pre, pre_words);
  READ(wires, wire_words);
  fclose(f);

  mp2g_fri_params fp;
  memset(&fp, 0, sizeof fp);
  fp.variant = MP2G_POSEIDON2; fp.log_n = log_n; fp.rate_bits = 3; fp.cap_height = 4; fp.pow_bits = hdr[6]; fp.num_queries = hdr[7];
  fp.n_layers = mp2g_reduction_arity_bits(log_n, fp.rate_bits, fp.cap_height, 4, 5, fp.arity_bits);
  fp.n_oracles = 4;
  fp.oracle_w[0] = num_constants + num_routed; fp.oracle_w[1] = wires_w; fp.oracle_w[2] = 2 * (num_routed / 8); fp.oracle_w[3] = 16;
  fp.zs_oracle = 2; fp.zs_count = 2;
  const size_t capw = (size_t)4 << fp.cap_height, n_open = mp2g_fri_n_openings(&fp), pw = mp2g_fri_proof_words(&fp);

  mp2g_ctx* ctx;
  CHECK(mp2g_ctx_create(0, &ctx));
  void *d_pre, *d_wires, *d_pi, *d_cd, *d_caps, *d_open, *d_proof;
  CHECK(mp2g_dev_alloc(ctx, pre_words * 8, &d_pre));
  CHECK(mp2g_dev_alloc(ctx, wire_words * 8, &d_wires));
  CHECK(mp2g_dev_alloc(ctx, 32, &d_pi));
  CHECK(mp2g_dev_alloc(ctx, 32, &d_cd));
  CHECK(mp2g_dev_alloc(ctx, 4 * capw * 8, &d_caps));
  CHECK(mp2g_dev_alloc(ctx, n_open * 16, &d_open));
  CHECK(mp2g_dev_alloc(ctx, pw * 8, &d_proof));
  CHECK(mp2g_h2d(ctx, d_pre, pre, pre_words * 8));
  CHECK(mp2g_h2d(ctx, d_wires, wires, wire_words * 8));
  CHECK(mp2g_h2d(ctx, d_pi, pi_hash, 32));
  CHECK(mp2g_h2d(ctx, d_cd, digest, 32));

  mp2g_prover* pr;
  CHECK(mp2g_prover_create(ctx, &fp, 1, &pr));
  CHECK(mp2g_prover_set_preprocessed_dev(pr, d_pre));
  CHECK(mp2g_prover_enable_permutation(pr, num_routed, 8));
  CHECK(mp2g_prover_enable_quotient(pr));
  CHECK(mp2g_prover_set_gates(pr, gates, n_gates, num_selectors));
  const uint64_t* d_values[3] = {d_wires, NULL, NULL};
  CHECK(mp2g_prover_prove_dev(pr, d_values, d_cd, d_pi, d_caps, d_open, d_proof));

  /* VerifierOnlyCircuitData: the cap of the constants_sigmas commitment and the circuit digest */
  mp2g_batch* pre_batch;
  uint64_t* cap0 = malloc(capw * 8);
  CHECK(mp2g_commit_from_values(ctx, MP2G_POSEIDON2, pre, log_n, num_constants + num_routed, fp.rate_bits, fp.cap_height, &pre_batch));
  CHECK(mp2g_batch_cap(pre_batch, cap0));
  mp2g_batch_free(pre_batch);
  mp2g_verifier* v;
  CHECK(mp2g_verifier_create(ctx, &fp, cap0, digest, num_routed, 8, gates, n_gates, num_selectors, NULL, 0, MP2G_PI_HASH_GIVEN, 1, &v));
  uint32_t part_words[4];
  const size_t words = mp2g_verifier_proof_words(v, part_words);
  /* the four parts where the prover left them: pi hash | caps of oracles 1..3 | openings | FRI words */
  const uint64_t* d_parts[4] = {d_pi, (const uint64_t*)d_caps + capw, d_open, d_proof};
  const uint64_t strides[4] = {4, 4 * capw, 2 * n_open, pw};
  uint32_t status = 99;
  CHECK(mp2g_verifier_verify_dev(v, d_parts, strides, 1, &status));
  printf("proof_words=%zu line_points=%u\nstatus=%u\n", words, mp2g_gate_table_line_points(gates, n_gates, num_selectors), status);

  /* flip one opening word (the low bit of the first limb of wire 3's opening: still a canonical element) */
  uint64_t word;
  uint64_t* d_word = (uint64_t*)d_open + 2 * (fp.oracle_w[0] + 3);
  CHECK(mp2g_d2h(ctx, &word, d_word, 8));
  word ^= 1;
  CHECK(mp2g_h2d(ctx, d_word, &word, 8));
  status = 99;
  CHECK(mp2g_verifier_verify_dev(v, d_parts, strides, 1, &status));
  printf("status=%u\n", status);
  mp2g_verifier_free(v);
  mp2g_prover_free(pr);
  mp2g_ctx_destroy(ctx);
  return 0;
}
