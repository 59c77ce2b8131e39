/* libmp2gpu -- C ABI of the MI355X (gfx950) back end for the Plonky2 prover path of
 * Lagrange-Labs/mapreduce-plonky2 (mp2-v1 / recursion-framework).
 *
 * The reference has no FFI for this path: every proof is produced by plonky2's
 * `CircuitData::prove(pw)` called at recursion-framework/src/circuit_builder.rs:308,
 * recursion-framework/src/universal_verifier_gadget/wrap_circuit.rs:143 and
 * verifiable-db/src/api.rs:207, with the hasher chosen by `type C = Poseidon2GoldilocksConfig`
 * (mp2-common/src/lib.rs:37-42). A Rust host keeps those signatures and replaces the bodies of
 * plonky2's PolynomialBatch::{from_values,from_coeffs}, MerkleTree::new, fri_proof and the
 * Hasher impl with the calls below (binding sketch: INTEGRATION.md).
 *
 * Conventions follow the only in-tree C ABI, gnark-utils (gnark-utils/src/lib.rs:13-52,
 * lib/lib.go:40-47,142-161,213-216): plain pointers and sizes, an int status (0 = ok), the
 * message of the last failure via mp2g_last_error(), callee-owned handles freed by the matching
 * *_free. Field elements are canonical u64 (< 2^64 - 2^32 + 1), little-endian in memory.
 * `variant` selects the permutation: 0 = Poseidon2 (default C), 1 = Poseidon (WrapC,
 * verifiable-db/src/api.rs:148). A context is bound to one GPU and one HIP stream; it is
 * thread-compatible, not thread-safe. Pointers named d_* are device pointers on the context's
 * GPU, all others are host pointers. No entry point falls back to the CPU.
 */
#ifndef MP2G_H
#define MP2G_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mp2g_ctx mp2g_ctx;
typedef struct mp2g_tree mp2g_tree;   /* plonky2 MerkleTree   (hash/merkle_tree.rs)  */
typedef struct mp2g_batch mp2g_batch; /* plonky2 PolynomialBatch (fri/oracle.rs)     */

#define MP2G_POSEIDON2 0
#define MP2G_POSEIDON 1

/* Diagnostic: Poseidon / Poseidon2 permutations queued by the Merkle leaf sponge (every commitment of every prove() on every
 * context) since the library was loaded -- a host-side count. Divided into the leaf kernel's time in a kernel trace it is the
 * sponge's rate inside a proving step (bench.py `roofline_alu`). Replaces nothing in the reference. */
uint64_t mp2g_stat_leaf_permutations(void);
/* ---- library / context ------------------------------------------------------------------ */
const char* mp2g_last_error(void);
int mp2g_device_count(void);
/* A context = one device, one HIP stream, ONE host thread proving at a time. Every prover created on a context takes its
 * per-batch working buffers (LDE values, Merkle levels, quotient values, FRI layers ...) from the context's shared scratch,
 * which is safe because their launches are ordered on that one stream: a host that wants several proofs in flight
 * concurrently creates one context per worker thread. Environment: MP2G_SHARE_SCRATCH=0 gives every prover buffers of
 * its own (about three times the device memory of a table build; the same proofs). Fails when no HIP device is visible:
 * there is no CPU path. */
int mp2g_ctx_create(int device, mp2g_ctx** out);
void mp2g_ctx_destroy(mp2g_ctx* ctx);
int mp2g_ctx_sync(mp2g_ctx* ctx);
/* HIP's current device is a property of the calling THREAD (0 until set). mp2g_ctx_create sets it for the creating thread; a worker thread
 * that drives a context of another device (one process per GPU with several proving threads, rank > 0 of a node) calls this once before
 * its first call: allocations and launches follow the thread's current device. */
int mp2g_ctx_make_current(mp2g_ctx* ctx);
/* free / total bytes of the context's device (hipMemGetInfo): what a host sizes its provers' capacities against */
int mp2g_ctx_mem_info(mp2g_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
void* mp2g_ctx_stream(mp2g_ctx* ctx);                 /* hipStream_t the context launches on */
int mp2g_ctx_set_stream(mp2g_ctx* ctx, void* stream); /* adopt a caller-owned hipStream_t     */
int mp2g_dev_alloc(mp2g_ctx* ctx, size_t bytes, void** d_ptr);
int mp2g_dev_free(mp2g_ctx* ctx, void* d_ptr);
int mp2g_h2d(mp2g_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int mp2g_d2h(mp2g_ctx* ctx, void* dst, const void* d_src, size_t bytes);
/* stream-ordered strided device-to-device copy: `rows` pieces of width_bytes, the i-th from d_src + i * src_pitch to
 * d_dst + i * dst_pitch (how a batch of proofs becomes the next witness program's input vectors without leaving the device) */
int mp2g_d2d_2d(mp2g_ctx* ctx, void* d_dst, size_t dst_pitch, const void* d_src, size_t src_pitch, size_t width_bytes, size_t rows);
/* pinned host staging memory and stream-ordered uploads (a host that feeds witness matrices from
 * its own memory overlaps the PCIe copy of batch k+1 with the proving of batch k) */
int mp2g_host_alloc(mp2g_ctx* ctx, size_t bytes, void** ptr);
int mp2g_host_free(mp2g_ctx* ctx, void* ptr);
int mp2g_h2d_async(mp2g_ctx* ctx, void* d_dst, const void* src, size_t bytes);
/* HIP-event stopwatch on the context's stream (used by bench.py) */
int mp2g_timer_start(mp2g_ctx* ctx);
int mp2g_timer_stop(mp2g_ctx* ctx, float* ms);

/* ---- NTT / LDE: replaces plonky2_field fft.rs fft/ifft/coset_fft and the LDE loop of
 *      PolynomialBatch::from_coeffs ------------------------------------------------------ */
/* `batch` transforms of 2^log_n points, in place. inverse=0: coefficients -> values
 * v[i] = P(shift * w^i) (coset_shift 0 = no shift); inverse=1: values -> coefficients.
 * bitrev_out!=0 leaves the output in bit-reversed index order. */
int mp2g_ntt(mp2g_ctx* ctx, uint64_t* data, uint32_t log_n, uint32_t batch, int inverse,
             uint64_t coset_shift, int bitrev_out);
int mp2g_ntt_dev(mp2g_ctx* ctx, const uint64_t* d_in, uint64_t* d_out, uint32_t log_n, uint32_t batch,
                 int inverse, uint64_t coset_shift, int bitrev_out);
/* coeffs [w][n] -> leaves [n << rate_bits][w]: row i = evaluations at g * w_N^bitrev(i)
 * (transpose + reverse_index_bits of from_coeffs). Host layout of plonky2. */
int mp2g_lde_leaves(mp2g_ctx* ctx, const uint64_t* coeffs, uint32_t log_n, uint32_t w, uint32_t rate_bits,
                    uint64_t* leaves);
/* same values, kept polynomial-major on the device: d_values [w][n << rate_bits], index
 * bit-reversed (column i of that matrix is leaf i). */
int mp2g_lde_dev(mp2g_ctx* ctx, const uint64_t* d_coeffs, uint32_t log_n, uint32_t w, uint32_t rate_bits,
                 uint64_t* d_values);

/* ---- hashing / Merkle: replaces Hasher::{hash_no_pad,hash_or_noop,two_to_one} and
 *      MerkleTree::{new,prove} ------------------------------------------------------------- */
/* out[i][0..out_len) = hash_n_to_m_no_pad(in[i][0..in_len)), out_len = 4 (HashOut) or 5
 * (map-to-curve, mp2-common/src/group_hashing/field_to_curve.rs:41-47) */
int mp2g_hash_no_pad_batch(mp2g_ctx* ctx, int variant, const uint64_t* in, uint32_t in_len, uint32_t count,
                           uint32_t out_len, uint64_t* out);
int mp2g_hash_no_pad_batch_dev(mp2g_ctx* ctx, int variant, const uint64_t* d_in, uint32_t in_len,
                               uint32_t count, uint32_t out_len, uint64_t* d_out);
/* MerkleTree::new(leaves, cap_height); leaves [2^log_leaves][leaf_len] */
int mp2g_merkle_build(mp2g_ctx* ctx, int variant, const uint64_t* leaves, uint32_t leaf_len,
                      uint32_t log_leaves, uint32_t cap_height, mp2g_tree** out);
int mp2g_merkle_cap(const mp2g_tree* tree, uint64_t* cap /* [1<<cap_height][4] */);
/* leaves_out [n_idx][leaf_len] (may be NULL), siblings_out [n_idx][log_leaves-cap_height][4] bottom-up */
int mp2g_merkle_open(const mp2g_tree* tree, const uint32_t* idx, uint32_t n_idx, uint64_t* leaves_out,
                     uint64_t* siblings_out);
void mp2g_merkle_free(mp2g_tree* tree);

/* ---- polynomial commitment: replaces PolynomialBatch::{from_values,from_coeffs} ----------- */
/* values [w][n] over the subgroup (natural order): per-poly iFFT, LDE x 2^rate_bits on the
 * coset g<w_N>, Merkle tree with cap. */
int mp2g_commit_from_values(mp2g_ctx* ctx, int variant, const uint64_t* values, uint32_t log_n, uint32_t w,
                            uint32_t rate_bits, uint32_t cap_height, mp2g_batch** out);
int mp2g_commit_from_values_dev(mp2g_ctx* ctx, int variant, const uint64_t* d_values, uint32_t log_n,
                                uint32_t w, uint32_t rate_bits, uint32_t cap_height, mp2g_batch** out);
int mp2g_commit_from_coeffs_dev(mp2g_ctx* ctx, int variant, const uint64_t* d_coeffs, uint32_t log_n,
                                uint32_t w, uint32_t rate_bits, uint32_t cap_height, mp2g_batch** out);
/* re-run the commitment into an existing batch of the same shape (no allocation: the form the
 * batched prover and bench.py use) */
int mp2g_recommit_from_values_dev(mp2g_ctx* ctx, mp2g_batch* batch, const uint64_t* d_values);
/* MerkleTree::new(leaves, cap_height) again over the LDE values the batch already holds ([dep] plonky2 hash/merkle_tree.rs;
 * called by PolynomialBatch::from_coeffs): parts = 1 the leaf sponges only (digests of the 2^(log_n + rate_bits) leaves),
 * 2 the tree levels above them only, 3 both. Same cap as the commitment made; what bench.py times the leaf kernel with. */
int mp2g_batch_rehash_dev(mp2g_ctx* ctx, mp2g_batch* batch, int parts);
int mp2g_batch_cap(const mp2g_batch* batch, uint64_t* cap);
int mp2g_batch_coeffs(const mp2g_batch* batch, uint64_t* coeffs /* [w][n] */);
int mp2g_batch_open(const mp2g_batch* batch, const uint32_t* idx, uint32_t n_idx,
                    uint64_t* leaves_out /* [n_idx][w] */, uint64_t* siblings_out);
void mp2g_batch_free(mp2g_batch* batch);

/* ---- Fiat-Shamir + FRI: replaces iop/challenger.rs, fri/prover.rs fri_proof and
 *      PolynomialBatch::prove_openings ---------------------------------------------------- */
/* FRI / PCS parameters of one circuit shape. standard_recursion_config
 * (mp2-common/src/lib.rs:45-47): rate_bits 3, cap_height 4, pow_bits 16, num_queries 28,
 * reduction ConstantArityBits(4,5); oracles = constants_sigmas, wires, zs_partial_products,
 * quotient; the first zs_count polynomials of oracle zs_oracle are also opened at g*zeta. */
typedef struct mp2g_fri_params {
  uint32_t variant;
  uint32_t log_n;       /* degree_bits */
  uint32_t rate_bits;
  uint32_t cap_height;
  uint32_t pow_bits;
  uint32_t num_queries;
  uint32_t n_layers;    /* len(reduction_arity_bits) */
  uint32_t arity_bits[8];
  uint32_t n_oracles;
  uint32_t oracle_w[8];
  uint32_t zs_oracle;
  uint32_t zs_count;
  /* lookup argument: polynomials per challenge round (0 = none; ceil((num_routed/2) / 7) + 1 = 7 under
   * standard_recursion_config). The last zs_count * num_lookup_polys polynomials of oracle zs_oracle are the
   * lookup polynomials (RE, then the partial Sum/LDC polynomials, per round); they are opened at zeta and at
   * g*zeta and close both FRI batches (plonk/circuit_data.rs fri_all_polys / fri_next_batch_polys). */
  uint32_t num_lookup_polys;
} mp2g_fri_params;
/* fri/reduction_strategies.rs ConstantArityBits(arity_bits, final_poly_bits); returns the count */
uint32_t mp2g_reduction_arity_bits(uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height,
                                   uint32_t arity_bits, uint32_t final_poly_bits, uint32_t* out);
/* Flat FriProof layout in u64 words (the fields of plonky2's FriProof in serde order, without
 * bincode length prefixes):
 *   commit_phase_merkle_caps [n_layers][1<<cap][4]
 *   query_round_proofs [num_queries] { initial_trees_proof: per oracle { leaf[w], siblings[lg-cap][4] };
 *                                      steps: per layer { evals[1<<arity][2], siblings[..][4] } }
 *   final_poly [final_len][2]
 *   pow_witness
 * (the library's own offsets into this layout and into the openings: csrc/layout.h) */
size_t mp2g_fri_proof_words(const mp2g_fri_params* p);
/* sum(oracle_w) + zs_count + zs_count * num_lookup_polys extension values, in FRI batch order
 * (OpeningSet::to_fri_openings): at zeta every polynomial in oracle order except the lookup polynomials, which
 * come last (after the quotient chunks); then at g*zeta the Z polynomials and the lookup polynomials. */
size_t mp2g_fri_n_openings(const mp2g_fri_params* p);

/* Device-resident challengers: `count` independent transcripts stepped in lockstep. */
typedef struct mp2g_challenger mp2g_challenger;
int mp2g_challenger_create(mp2g_ctx* ctx, int variant, uint32_t count, mp2g_challenger** out);
/* transcript t observes elems[t*n .. t*n+n) */
int mp2g_challenger_observe(mp2g_challenger* ch, const uint64_t* elems, uint32_t n);
int mp2g_challenger_get(mp2g_challenger* ch, uint32_t n, uint64_t* out /* [count][n] */);
void mp2g_challenger_free(mp2g_challenger* ch);

/* One FRI layer fold in the value domain. evals [1<<log_m][2]: bit-reversed evaluations on
 * shift*<w_m>; out [(1<<log_m)>>arity_bits][2]: bit-reversed evaluations of the folded polynomial
 * on shift^(2^arity_bits). Equals coeffs.chunks(arity).map(reduce_with_powers(beta)) + coset_fft. */
int mp2g_fri_fold(mp2g_ctx* ctx, const uint64_t* evals, uint32_t log_m, uint32_t arity_bits,
                  const uint64_t beta[2], uint64_t shift, uint64_t* out);
/* fri_proof_of_work: smallest witness w such that permute(state with state[pos] = w)[7] has
 * >= bits leading zeros; `state` = sponge state already overwritten with the pending inputs. */
int mp2g_fri_pow(mp2g_ctx* ctx, int variant, const uint64_t state[12], uint32_t pos, uint32_t bits,
                 uint64_t* witness);

/* Openings of one committed batch at an extension point (plonk/prover.rs eval_commitment):
 * out[p] = [c0, c1] of polynomial p evaluated at point. */
int mp2g_batch_eval_ext(const mp2g_batch* batch, const uint64_t point[2], uint64_t* out /* [w][2] */);
/* PolynomialBatch::prove_openings / fri_proof over committed batches: `oracles` in FRI order
 * (constants_sigmas, wires, zs_partial_products, quotient), zeta the opening point, `ch` a count-1
 * challenger that has already observed the openings; on return it has absorbed the FRI transcript.
 * proof: mp2g_fri_proof_words(params) words, host. This is the call a host makes after computing the
 * quotient polynomials itself. */
int mp2g_fri_prove(mp2g_ctx* ctx, const mp2g_fri_params* params, mp2g_batch* const* oracles, const uint64_t zeta[2],
                   mp2g_challenger* ch, uint64_t* proof);

/* Batched PCS prover: the commitment / Fiat-Shamir / opening / FRI skeleton of plonky2's prove()
 * for `batch` same-shape proofs at once, everything resident on the device. */
typedef struct mp2g_prover mp2g_prover;
int mp2g_prover_create(mp2g_ctx* ctx, const mp2g_fri_params* params, uint32_t batch, mp2g_prover** out);
/* commit oracle 0 (constants_sigmas, [w0][n] subgroup values), shared by every proof */
int mp2g_prover_set_preprocessed_dev(mp2g_prover* pr, const uint64_t* d_values);
/* d_values[o-1] = [batch][w_o][n] subgroup values of oracle o = 1..n_oracles-1;
 * d_circuit_digest [4]; d_pi_hash [batch][4]. Outputs (device): d_caps [batch][n_oracles][1<<cap][4],
 * d_openings [batch][n_openings][2], d_proof [batch][proof_words]. Asynchronous on the stream. */
int mp2g_prover_prove_dev(mp2g_prover* pr, const uint64_t* const* d_values, const uint64_t* d_circuit_digest,
                          const uint64_t* d_pi_hash, uint64_t* d_caps, uint64_t* d_openings, uint64_t* d_proof);
void mp2g_prover_free(mp2g_prover* pr);
/* single proof, host pointers: values[o] = [w_o][n] for o = 0..n_oracles-1 */
int mp2g_pcs_prove(mp2g_ctx* ctx, const mp2g_fri_params* params, const uint64_t* const* values,
                   const uint64_t circuit_digest[4], const uint64_t pi_hash[4], uint64_t* caps,
                   uint64_t* openings, uint64_t* proof);

/* ---- Ecgfp5 multiset digest (off-circuit value side) -------------------------------------- */
/* A point is returned as its canonical 5-limb encoding w = y/x (plonky2_ecgfp5 Point::encode;
 * the form the reference's known-answer test holds, sswu_value.rs:88-118) and/or as the 11-limb
 * short-Weierstrass form [x0..x4, y0..y4, is_inf] of mp2-common/src/group_hashing/mod.rs:163-174.
 * Either output pointer may be NULL. */
/* map_to_curve_point (field_to_curve.rs:36-48) of `count` inputs of in_len limbs each */
int mp2g_map_to_curve_batch(mp2g_ctx* ctx, int variant, const uint64_t* in, uint32_t in_len, uint32_t count,
                            uint64_t* out_w /* [count][5] */, uint64_t* out_weierstrass /* [count][11] */);
/* simple_swu (sswu_value.rs:31-77) of `count` GF(p^5) elements u[count][5] (coefficient i of z^i), without the sponge: what
 * mp2g_map_to_curve_batch does after its hash. Limbs may be any u64 and are read mod p, as GoldilocksField(x) reads them. */
int mp2g_swu_batch(mp2g_ctx* ctx, const uint64_t* u /* [count][5] */, uint32_t count, uint64_t* out_w /* [count][5] */,
                   uint64_t* out_weierstrass /* [count][11] or NULL */);
/* add_curve_point (curve_add.rs:17-22) over `count` encoded points; fails on an invalid encoding.
 * Encodings are canonical: this entry, mp2g_curve_sum_ranges and mp2g_scalar_mul_batch refuse a point with a limb >= p ("point
 * encoding is not canonical"), checked on the host before anything is uploaded; (p,0,0,0,0) is not read as the neutral point. */
int mp2g_curve_sum(mp2g_ctx* ctx, const uint64_t* pts_w /* [count][5] */, uint32_t count, uint64_t out_w[5],
                   uint64_t out_weierstrass[11]);
/* the same sum over n_ranges index ranges [start, end) of one point array at once: the accumulated digest of every node of a
 * tree laid out in order (a subtree = one contiguous range) -- what SplitDigestPoint::accumulate (mp2-common/src/digest.rs:38-47)
 * builds node by node up the cells tree / row tree (verifiable-db/src/cells_tree/full_node.rs:26-28,
 * row_tree/full_node.rs:78-82). An empty range gives the neutral point. */
int mp2g_curve_sum_ranges(mp2g_ctx* ctx, const uint64_t* pts_w /* [count][5] */, uint32_t count, const uint32_t* ranges /* [n_ranges][2] */,
                          uint32_t n_ranges, uint64_t* out_w /* [n_ranges][5] */, uint64_t* out_weierstrass /* [n_ranges][11] */);
/* scalar * point for 128-bit scalars given as 4 little-endian u32 limbs (hash_to_int_value,
 * mp2-common/src/poseidon.rs:120-133) */
int mp2g_scalar_mul_batch(mp2g_ctx* ctx, const uint64_t* pts_w /* [count][5] */, const uint32_t* scalars /* [count][4] */,
                          uint32_t count, uint64_t* out_w /* [count][5] */, uint64_t* out_weierstrass);
/* field_hashed_scalar_mul (group_hashing/mod.rs:220-225): HashToInt(H(inputs)) * base */
int mp2g_field_hashed_scalar_mul(mp2g_ctx* ctx, int variant, const uint64_t* inputs, uint32_t n_inputs,
                                 const uint64_t base_w[5], uint64_t out_w[5], uint64_t out_weierstrass[11]);
/* compute_table_row_digest (mp2-v1/src/values_extraction/mod.rs:527-571):
 *   sum over rows of row_id * sum over columns of D(id_c || value_c), row_id =
 *   HashToInt(H(H(unique column values) || n_cols)).
 * col_ids [n_cols]; values [rows][n_cols][8] and unique [rows][n_unique][8]: each U256 as 8
 * big-endian u32 words, most significant first (mp2-common/src/u256.rs:870-877). */
int mp2g_row_digest_batch(mp2g_ctx* ctx, int variant, const uint64_t* col_ids, uint32_t n_cols,
                          const uint32_t* values, const uint32_t* unique, uint32_t n_unique, uint32_t rows,
                          uint64_t out_w[5], uint64_t out_weierstrass[11]);
/* the per-row terms of that sum, row_id * sum over columns of D(id_c || value_c): the individual digest a row-tree node
 * contributes (verifiable-db/src/row_tree/secondary_index_cell.rs:99-139 with every cell individual) */
int mp2g_row_digests(mp2g_ctx* ctx, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* values,
                     const uint32_t* unique, uint32_t n_unique, uint32_t rows, uint64_t* out_w /* [rows][5] */,
                     uint64_t* out_weierstrass /* [rows][11] */);
/* same with device-resident inputs; d_frac_out [20] receives the sum in fractional coordinates
 * (X:Z:U:T) for further accumulation -- a representative of the point, not a canonical form: compare points through out_w
 * (Point::encode) or out_weierstrass; out_w / out_weierstrass are host pointers (may be NULL) */
int mp2g_row_digest_batch_dev(mp2g_ctx* ctx, int variant, const uint64_t* d_col_ids, uint32_t n_cols,
                              const uint32_t* d_values, const uint32_t* d_unique, uint32_t n_unique, uint32_t rows,
                              uint64_t* d_frac_out, uint64_t out_w[5], uint64_t out_weierstrass[11]);

/* ---- node hashes of a table's trees (off-circuit payload side, csrc/index_hash.hip) -------------------------------------------
 * The hashes a DB host stores for every node and the root proof's first four public inputs must equal: MerkleCell::aggregate
 * (mp2-v1/src/indexing/cell.rs:120-157), RowPayload::aggregate (row.rs:257-317), IndexNode::aggregate (index.rs:61-101), for a
 * whole block at once: one launch per tree level, no host round trip between the launches. Sponge input words are taken as
 * mp2g_hash_no_pad_batch takes them; a missing child hashes as hash_no_pad(&[]) (mp2-common/src/poseidon.rs:44-46, all zero).
 *
 * A tree shape: a binary tree or forest over nodes 0..n-1 given by left[n] / right[n] (-1 = no child). From them come every
 * node's height (0 without children, else 1 + the larger child's: one launch per height), min_idx / max_idx (the node reached by
 * following left / right children to the end: the reference's rule min = left.min if there is a left child, else the node's own
 * value, row.rs:261-285, carried as an index, so no U256 is compared), and the roots (nodes without a parent, ascending).
 * _create refuses, with a message, a child index outside -1..n-1, a node that is its own child, a node with two parents
 * (left[i] == right[i] != -1 included) and a cycle; n = 0 is the valid empty shape. Host work only: no GPU is needed.
 * _sbbst: ryhope's self-balanced BST over the positions 1..n (ryhope/src/tree/sbbst.rs: root :251-257, children :301-333 and
 * :487-503), position k = node k - 1; n <= 2^31 - 1.
 * Ownership: the first hashing call that uses a shape uploads its arrays to that call's context (on its stream); they stay there
 * until mp2g_tree_shape_free, and the shape is refused with any other context. _free waits for the device, so it may be called
 * while hashing calls with the shape are still queued. Free a shape before the context it was used with is destroyed: the shape
 * remembers that context by its address only, and would take a later context at the same address for it. A shape is not to be
 * used from two threads at once. */
typedef struct mp2g_tree_shape mp2g_tree_shape;
int mp2g_tree_shape_create(const int32_t* left, const int32_t* right, uint32_t n, mp2g_tree_shape** out);
int mp2g_tree_shape_sbbst(uint32_t n, mp2g_tree_shape** out);
uint32_t mp2g_tree_shape_size(const mp2g_tree_shape* shape);
uint32_t mp2g_tree_shape_num_levels(const mp2g_tree_shape* shape); /* largest height + 1; 0 for the empty shape */
uint32_t mp2g_tree_shape_num_roots(const mp2g_tree_shape* shape);
/* any output may be NULL; left / right give back the children (what _sbbst made); all [n] but roots [num_roots] */
int mp2g_tree_shape_describe(const mp2g_tree_shape* shape, int32_t* left, int32_t* right, uint32_t* height, uint32_t* min_idx,
                             uint32_t* max_idx, uint32_t* roots);
void mp2g_tree_shape_free(mp2g_tree_shape* shape);
/* ryhope's touched() (ryhope/src/lib.rs:216-222): the given nodes and all their ancestors up to the roots -- what
 * MerkleTreeKvDb::aggregate (:179-209) re-hashes after a block, and what mp2g_row_tree_hashes_update re-hashes. nodes receives them
 * grouped by height (ascending height, ascending node index inside a height: children before parents), *n_nodes their number.
 * Duplicates in touched collapse; n_touched == 0 gives the empty set. nodes == NULL only counts. cap < the number of nodes is an
 * error that still sets *n_nodes. An index >= n is refused with a message that names it. Host work only, no GPU is needed; the cost
 * is that of the closure (plus a sort of it), not of the shape. */
int mp2g_tree_shape_touched(const mp2g_tree_shape* shape, const uint32_t* touched, uint32_t n_touched, uint32_t* nodes /* [cap] or NULL */,
                            uint32_t cap, uint32_t* n_nodes);
/* every row's cells tree (cell.rs:120-157: H(H(left) || H(right) || id || value), 17 limbs): the sbbst over the positions
 * 1..n_cols-1; the cell at position k has the identifier col_ids[k] and the value values[row][k] (column 0 is the secondary index
 * and is not a cell). values [rows][n_cols][8] as mp2g_row_digests takes them (u256.rs:870-877), so one upload serves both.
 * roots [rows][4]; nodes [rows][n_cols-1][4] (position k at index k - 1) or NULL. n_cols == 1: no cells, every root is
 * hash_no_pad(&[]) (row.rs:299-302). Refused before any launch: variant not 0 / 1, n_cols outside 1..256, a col_ids entry >= p
 * (the reference builds them with from_canonical_u64), rows > 2^31. rows == 0 returns 0 and launches nothing.
 * _dev: col_ids stays a host array; d_roots / d_nodes 16-byte aligned; stream ordered, no synchronisation (the context keeps a
 * working buffer of rows * (n_cols-1) * 32 bytes, which grows, with one synchronisation, when a call needs more). */
int mp2g_cells_tree_hashes(mp2g_ctx* ctx, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* values /* [rows][n_cols][8] */,
                           uint32_t rows, uint64_t* roots, uint64_t* nodes);
int mp2g_cells_tree_hashes_dev(mp2g_ctx* ctx, int variant, const uint64_t* col_ids /* host */, uint32_t n_cols, const uint32_t* d_values,
                               uint32_t rows, uint64_t* d_roots, uint64_t* d_nodes);
/* the steady state of a block (MerkleTreeKvDb::aggregate over touched(), ryhope/src/lib.rs:179-222, for the rows' cells trees):
 * the complete cells trees of the rows row_idx[0..n_idx) recomputed from the current table. values is the WHOLE table
 * [rows][n_cols][8]; roots [rows][4] and nodes ([rows][n_cols-1][4] or NULL) are the whole table's too, in and out: only the listed
 * rows' entries are written. Duplicates in row_idx are allowed; n_idx == 0 returns 0 and launches nothing; n_cols == 1 writes
 * hash_no_pad(&[]) for the listed rows. Refused before any launch: what mp2g_cells_tree_hashes refuses, a row index >= rows (named
 * in the message), row_idx NULL with n_idx != 0, and for _dev misaligned d_roots / d_nodes.
 * _dev: col_ids and row_idx stay host arrays (row_idx may be reused or freed as soon as the call returns); stream ordered. The
 * context keeps the working buffer of mp2g_cells_tree_hashes_dev (here n_idx * (n_cols-1) * 32 bytes) and one device buffer for
 * the index lists; either grows, with one synchronisation, when a call needs more. The lists are uploaded from a ring of 4 pinned
 * slots of the context's, so update calls with different lists may be queued back to back without a synchronisation by the caller:
 * a call waits only when the upload of the fourth call before it has not finished yet. */
int mp2g_cells_tree_hashes_rows(mp2g_ctx* ctx, int variant, const uint64_t* col_ids, uint32_t n_cols, const uint32_t* values /* whole table */,
                                uint32_t rows, const uint32_t* row_idx, uint32_t n_idx, uint64_t* roots /* [rows][4] in and out */,
                                uint64_t* nodes /* in and out, or NULL */);
int mp2g_cells_tree_hashes_rows_dev(mp2g_ctx* ctx, int variant, const uint64_t* col_ids /* host */, uint32_t n_cols, const uint32_t* d_values,
                                    uint32_t rows, const uint32_t* row_idx /* host */, uint32_t n_idx, uint64_t* d_roots, uint64_t* d_nodes);
/* every node of a row tree (row.rs:257-317) or index tree (index.rs:61-101) of shape `shape`:
 * H(hL || hR || min || max || id || value || payload), 37 limbs. Node i's value is the 8 big-endian u32 words at
 * values + i * value_stride (value_stride in u32 words, >= 8: pass n_cols * 8 to read column 0 of the table in place); payload
 * [n][4] is the cells root per row (or the row tree's root per block for the index tree), NULL = hash_no_pad(&[]) for every
 * node. hashes [n][4]. A right child without a left one is hashed by the row tree's rule (min = the node's own value); the index
 * tree's caller refuses it beforehand if it wants IndexNode::aggregate's panic. Refused before any launch: variant not 0 / 1,
 * id >= p, value_stride < 8, a size that overflows. An empty shape returns 0 and launches nothing.
 * One launch per level: a degenerate chain of height h costs h launches, which is correct but slow; the reference's trees
 * (sbbst, scapegoat) are logarithmic.
 * _dev: d_payload / d_hashes 16-byte aligned; stream ordered, no synchronisation. */
int mp2g_row_tree_hashes(mp2g_ctx* ctx, int variant, const mp2g_tree_shape* shape, uint64_t id, const uint32_t* values, uint32_t value_stride,
                         const uint64_t* payload, uint64_t* hashes);
int mp2g_row_tree_hashes_dev(mp2g_ctx* ctx, int variant, const mp2g_tree_shape* shape, uint64_t id, const uint32_t* d_values,
                             uint32_t value_stride, const uint64_t* d_payload, uint64_t* d_hashes);
/* the same for the touched nodes and their ancestors only (MerkleTreeKvDb::aggregate, ryhope/src/lib.rs:179-209, re-aggregates
 * touched(), :216-222; the set is mp2g_tree_shape_touched's). On entry hashes [n][4] holds valid hashes for every node outside
 * that set; on return every node of the set holds its hash under the current values, payload and shape, and no word outside the
 * set has been written. The caller lists in touched every node whose value, payload or children differ from what hashes was
 * computed for: after an insertion the shape is a new mp2g_tree_shape, and touched holds the new node and the nodes whose child
 * pointers changed. min / max need no entry of their own: a node's min_idx and max_idx lie in its own subtree (row.rs:261-285), so a
 * change under them puts the node in the set. n_touched == 0 returns 0 and launches nothing. Refused before any launch: what
 * mp2g_row_tree_hashes refuses, a touched index >= n (named in the message), touched NULL with n_touched != 0, and for _dev
 * misaligned d_payload / d_hashes.
 * Poseidon2, while no level of the set has more than mp2g_row_tree_update_fused_width() nodes and the set has at most 256 levels:
 * ONE launch of one workgroup for the whole set (16 lanes per node, a barrier between levels). Everything else (original Poseidon,
 * wider sets, degenerate chains): one launch per level of the set.
 * _dev: touched stays a host array (it may be reused or freed as soon as the call returns); stream ordered; the index lists go
 * through the context's ring of pinned slots as mp2g_cells_tree_hashes_rows_dev describes, so calls with different lists may be
 * queued back to back. */
uint32_t mp2g_row_tree_update_fused_width(void);
int mp2g_row_tree_hashes_update(mp2g_ctx* ctx, int variant, const mp2g_tree_shape* shape, uint64_t id, const uint32_t* values,
                                uint32_t value_stride, const uint64_t* payload, const uint32_t* touched, uint32_t n_touched,
                                uint64_t* hashes /* [n][4] in and out */);
int mp2g_row_tree_hashes_update_dev(mp2g_ctx* ctx, int variant, const mp2g_tree_shape* shape, uint64_t id, const uint32_t* d_values,
                                    uint32_t value_stride, const uint64_t* d_payload, const uint32_t* touched /* host */, uint32_t n_touched,
                                    uint64_t* d_hashes);

/* ---- accumulated digests of a table's trees (off-circuit value side, csrc/tree_digest.hip) --------------------------------------
 * The Ecgfp5 digest every node of a cells tree and of the row tree exposes as public inputs, device resident: one pass over a tree
 * shape with one launch per level, and after a block only the touched nodes and their ancestors. Between the calls a point is the
 * 20 words d_frac holds (fractional coordinates X:Z:U:T, 5 limbs each): a representative of the point, not a canonical form, so no
 * call on the way pays Point::encode's inversion or Point::decode's square root. Compare points through mp2g_curve_emit_dev only. */
/* Point::decode ([dep] plonky2_ecgfp5 curve/curve.rs) of `count` encodings into d_frac [count][20] (device). Refuses a limb >= p on
 * the host before any upload ("point encoding is not canonical"), as mp2g_curve_sum does, and an invalid encoding after the launch
 * (one synchronisation; d_frac then holds the neutral point at the refused entries). count == 0 returns 0 and launches nothing. */
int mp2g_curve_decode_dev(mp2g_ctx* ctx, const uint64_t* pts_w /* host [count][5] */, uint32_t count, uint64_t* d_frac /* [count][20] */);
/* Point::encode / the 11-limb Weierstrass form (group_hashing/mod.rs:163-174) of the points idx[0..count) of d_frac; idx NULL =
 * the points 0..count-1. idx is a host array (free on return; it goes through the context's ring of pinned slots) whose entries the
 * caller keeps inside d_frac: the call does not know that buffer's size. out_w [count][5] and out_weierstrass [count][11] are host
 * arrays and compact (entry j belongs to idx[j]); either may be NULL. One synchronisation. */
int mp2g_curve_emit_dev(mp2g_ctx* ctx, const uint64_t* d_frac, const uint32_t* idx /* host or NULL */, uint32_t count,
                        uint64_t* out_w /* [count][5] */, uint64_t* out_weierstrass /* [count][11] */);
/* acc[i] = own[i] + acc[left[i]] + acc[right[i]] for every node of `shape`: the accumulated digest SplitDigestPoint::accumulate
 * (mp2-common/src/digest.rs:38-47) builds node by node up the cells tree (verifiable-db/src/cells_tree/full_node.rs:26-28) and the
 * row tree (row_tree/full_node.rs:78-82). d_own / d_acc [n][20]. One launch per level of the shape, n - 1 additions in all (the
 * complete addition: equal points, inverse points and the neutral point need no care); a missing child costs none. Any shape:
 * unlike mp2g_curve_sum_ranges it does not need the tree laid out in order. Stream ordered, no synchronisation. Refused before any
 * launch: shape NULL, d_own and d_acc overlapping, a shape first used with another context. An empty shape returns 0 and launches
 * nothing. */
int mp2g_tree_digests_dev(mp2g_ctx* ctx, const mp2g_tree_shape* shape, const uint64_t* d_own /* [n][20] */, uint64_t* d_acc /* [n][20] */);
/* the same from encodings own_w [n][5] and to encodings out_w [n][5] / out_weierstrass [n][11] (either NULL) in host memory: decode,
 * the pass, emit. Refuses what mp2g_curve_decode_dev refuses. */
int mp2g_tree_digests(mp2g_ctx* ctx, const mp2g_tree_shape* shape, const uint64_t* own_w /* [n][5] */, uint64_t* out_w,
                      uint64_t* out_weierstrass);
/* the same for the touched nodes and their ancestors only (MerkleTreeKvDb::aggregate over touched(), ryhope/src/lib.rs:179-222; the
 * set is mp2g_tree_shape_touched's). The contract is mp2g_row_tree_hashes_update_dev's: on entry d_acc holds valid digests for
 * every node outside that set; on return every node of the set holds its digest under the current d_own and shape, and no word
 * outside the set has been written. touched lists every node whose own digest or children differ from what d_acc was computed for;
 * it is a host array, free on return, and the lists go through the context's ring of pinned slots. n_touched == 0 returns 0 and
 * launches nothing. Refused before any launch: what mp2g_tree_digests_dev refuses, a touched index >= n (named in the message),
 * touched NULL with n_touched != 0.
 * While no level of the set has more than mp2g_tree_digests_update_fused_width() nodes and the set has at most 256 levels: ONE
 * launch of one 128-lane workgroup for the whole set (one lane per node, a barrier between levels). Everything else: one launch
 * per level of the set. */
uint32_t mp2g_tree_digests_update_fused_width(void);
int mp2g_tree_digests_update_dev(mp2g_ctx* ctx, const mp2g_tree_shape* shape, const uint64_t* d_own, const uint32_t* touched /* host */,
                                 uint32_t n_touched, uint64_t* d_acc /* in and out */);
/* every node of every row's cells tree: d_nodes[row][k-1] = D(col_ids[k] || values[row][k]) + d_nodes[row][left] +
 * d_nodes[row][right] over the sbbst of the positions 1..n_cols-1, which is Cell::values_digest (verifiable-db/src/cells_tree/
 * mod.rs:65-72) accumulated up the tree (cells_tree/full_node.rs:26-28, partial_node.rs) with every cell individual. n_cols,
 * col_ids, d_values and the node indexing exactly as mp2g_cells_tree_hashes_dev takes them; d_nodes [rows][n_cols-1][20]. One launch
 * per height of the cells tree, one square root per cell. row_idx (host, free on return) NULL with n_idx == 0 = all rows; otherwise
 * only the listed rows' entries are written (duplicates allowed), and a list with n_idx == 0 returns 0 and launches nothing, as
 * rows == 0 does. n_cols == 1: there are no cells and d_nodes is not touched. Refused before any launch: what
 * mp2g_cells_tree_hashes_rows_dev refuses (variant, n_cols outside 1..256, a col_ids entry >= p, a row index >= rows, named in the
 * message, row_idx NULL with n_idx != 0). Stream ordered. */
int mp2g_cells_tree_digests_dev(mp2g_ctx* ctx, int variant, const uint64_t* col_ids /* host */, uint32_t n_cols, const uint32_t* d_values,
                                uint32_t rows, const uint32_t* row_idx /* host or NULL */, uint32_t n_idx,
                                uint64_t* d_nodes /* [rows][n_cols-1][20] */);
/* the per-row terms of mp2g_row_digests (secondary_index_cell.rs:99-139; mp2-v1/src/values_extraction/mod.rs:499-571), device
 * resident: d_own[row] = row_id * sum over columns of D(id_c || value_c). Row r's unique columns are the 8 * n_unique words at
 * d_unique + r * unique_stride (u32 words, >= 8 * n_unique: pass d_values and n_cols * 8 to read column 0 of the table in place).
 * d_cells_nodes NULL = map every column as mp2g_row_digests does; otherwise it is what mp2g_cells_tree_digests_dev wrote, and the
 * sum is D(id_0 || value_0) + d_cells_nodes[row][root of the cells tree]: one square root per row instead of n_cols, the same
 * group element. n_cols == 1 ignores d_cells_nodes. row_idx as above: only the listed rows of d_own [rows][20] are written.
 * Refused before any launch: what mp2g_cells_tree_digests_dev refuses, d_unique NULL with n_unique != 0, unique_stride below
 * 8 * n_unique. Stream ordered. */
int mp2g_row_digests_dev(mp2g_ctx* ctx, int variant, const uint64_t* col_ids /* host */, uint32_t n_cols, const uint32_t* d_values,
                         const uint32_t* d_unique, uint32_t unique_stride, uint32_t n_unique, uint32_t rows,
                         const uint64_t* d_cells_nodes /* or NULL */, const uint32_t* row_idx /* host or NULL */, uint32_t n_idx,
                         uint64_t* d_own /* [rows][20] */);

/* ---- tables in contract storage: MPT storage-leaf digests (off-circuit value side, csrc/extraction.hip) --------------------------
 * What the reference computes for a table that lives in contract storage (mp2-v1/src/values_extraction/mod.rs:298-496): every
 * storage leaf holds one 32-byte EVM word, and the columns of its (slot, evm_word) are bit fields of that word.
 *
 * A column's layout is three u32: byte offset, bit offset (0..8), length in bits (1..256). extract_value (mp2-v1/src/
 * values_extraction/gadgets/column_gadget.rs:326-368) cuts the field out: with k = ceil(length / 8), byte j < k of the result is
 * ((word[b + j] & (2^(8 - bit) - 1)) << bit) + (word[b + j + 1] >> (8 - bit)), word[32] = 0; when m = length % 8 is not zero the
 * last byte is shifted right by 8 - m; the k bytes are left-padded to 32. On the word as a 256-bit big-endian integer V that is
 * ((V << (8 b + bit)) mod 2^256) >> (256 - 8 k), then the low byte shifted right by 8 - m: what the kernels do, on eight registers.
 * Refused before anything is uploaded or launched, with a message that names the argument: length 0 or above 256, bit offset above
 * 8, byte_offset + ceil(length / 8) > 32, more than 32 columns, a required pointer that is NULL, and for _dev a d_words / d_keys
 * that is not 16-byte aligned (a word is read as two 16-byte loads). */
/* the cut alone: out[leaf][col] = extract_value(words[leaf], layout[col]) as 8 big-endian u32 words, the cell format of
 * mp2g_row_digests, mp2g_cells_tree_hashes and mp2g_cells_tree_digests_dev: a storage table reaches those entries without leaving
 * the device. words [count][32] bytes; layout [n_cols][3] (host in both forms); out [count][n_cols][8]. count == 0 or n_cols == 0
 * returns 0 and launches nothing. _dev is stream ordered. */
int mp2g_extract_values(mp2g_ctx* ctx, const uint8_t* words, const uint32_t* layout, uint32_t n_cols, uint32_t count, uint32_t* out);
int mp2g_extract_values_dev(mp2g_ctx* ctx, const uint8_t* d_words, const uint32_t* layout /* host */, uint32_t n_cols, uint32_t count,
                            uint32_t* d_out);
/* compute_leaf_single_values_digest / compute_leaf_mapping_values_digest / compute_leaf_mapping_of_mappings_values_digest
 * (mod.rs:327-341, :374-406, :450-496) of `count` leaves of one (slot, evm_word), n_keys = 0 / 1 / 2:
 *   S      = sum over the extracted columns of D(col_ids[c] || extract_value(word, layout[c]))      (ColumnGadgetData::digest,
 *            column_gadget.rs:301-323), plus D(key_ids[j] || key_j) for every key when evm_word == 0 (mod.rs:389-400, :474-488)
 *   row_id = HashToInt(H(H(key_0 || key_1) || n_table_columns + n_keys))                             (mod.rs:298-314, :499-523)
 *   digest = row_id * S
 * col_ids / layout: the n_extracted columns of this (slot, evm_word) (filter_table_column_identifiers, column_gadget.rs:372-389);
 * n_table_columns = table_info.len(), every column of the table, those of other EVM words included. keys [count][n_keys][32]: each
 * key left_pad32-ed, the outer key before the inner one; key_ids [n_keys]. A leaf without columns and without key digests gives the
 * neutral point (encoding 0, Weierstrass [0 x 10, 1]). col_ids, layout and key_ids are host arrays in both forms and travel in the
 * kernel's arguments.
 * out_w [count][5] / out_weierstrass [count][11]: the leaves' digests; sum_w [5] / sum_weierstrass [11]: their sum, what a branch
 * above all of them accumulates. Each output pointer may be NULL. _dev: d_frac_out [count][20] (or NULL) receives the leaves'
 * digests in fractional coordinates, for mp2g_tree_digests_* and mp2g_curve_emit_dev; the other four outputs are host pointers;
 * stream ordered, one synchronisation when a host output is asked for.
 * Refused like the cut, and further: variant not 0 / 1, n_extracted > 32, n_keys > 2, n_table_columns < n_extracted, a col_ids or
 * key_ids entry >= p. A refused call writes no output. count == 0 launches nothing; its sum is the neutral point. */
int mp2g_leaf_values_digests(mp2g_ctx* ctx, int variant, const uint64_t* col_ids, const uint32_t* layout, uint32_t n_extracted,
                             uint32_t n_table_columns, const uint8_t* words, const uint8_t* keys, const uint64_t* key_ids, uint32_t n_keys,
                             uint32_t evm_word, uint32_t count, uint64_t* out_w, uint64_t* out_weierstrass, uint64_t sum_w[5],
                             uint64_t sum_weierstrass[11]);
int mp2g_leaf_values_digests_dev(mp2g_ctx* ctx, int variant, const uint64_t* col_ids /* host */, const uint32_t* layout /* host */,
                                 uint32_t n_extracted, uint32_t n_table_columns, const uint8_t* d_words, const uint8_t* d_keys,
                                 const uint64_t* key_ids /* host */, uint32_t n_keys, uint32_t evm_word, uint32_t count,
                                 uint64_t* d_frac_out, uint64_t* out_w, uint64_t* out_weierstrass, uint64_t sum_w[5],
                                 uint64_t sum_weierstrass[11]);

/* ---- Keccak-256 on the device: storage slot keys and MPT leaf words (off-circuit value side, csrc/storage.hip) ------------------
 * What lies between an eth_getProof answer and the 32-byte EVM word mp2g_leaf_values_digests starts from. Keccak-256 is Ethereum's
 * keccak256: Keccak-f[1600], rate 136 bytes, domain byte 0x01 (not SHA3-256's 0x06), final bit 0x80. One lane per message / leaf,
 * one shared permutation (csrc/keccak.cuh).
 *
 * out[i] = keccak256(msgs + i * stride, lens ? lens[i] : len): the 32 digest bytes. Read as eight little-endian u32 words they are
 * keccak256(node).pack(Endianness::Little), the H public input of the values-extraction proofs (leaf_single.rs:279,
 * leaf_mapping.rs:340, branch.rs:318, extension.rs:183): no second output is needed. msgs [count][stride] bytes; a message is
 * absorbed with 8-byte loads, so stride is a multiple of 8 and the base is 8-byte aligned. No byte at or past `stride` of a row is
 * read and no byte in [len, stride) influences the result. lens [count] (or NULL: every message has `len` bytes).
 * Refused before anything is uploaded or launched, with a message that names the argument: stride 0, not a multiple of 8 or above
 * 65536; len > stride when lens is NULL; in the host form a lens[i] > stride (the message names i); msgs or out NULL; for _dev a
 * d_msgs or d_out that is not 8-byte aligned (or a d_lens that is not 4-byte aligned). The host cannot see d_lens: in the _dev form
 * a lane clamps its length to stride. Lanes of one wave may run different numbers of rate blocks. A refused call writes no output;
 * count == 0 returns 0 and launches nothing; _dev is stream ordered. */
int mp2g_keccak256_batch(mp2g_ctx* ctx, const uint8_t* msgs, uint32_t stride, const uint32_t* lens, uint32_t len, uint32_t count,
                         uint8_t* out);
int mp2g_keccak256_batch_dev(mp2g_ctx* ctx, const uint8_t* d_msgs, uint32_t stride, const uint32_t* d_lens, uint32_t len, uint32_t count,
                             uint8_t* d_out);
/* StorageSlot::location, mpt_key and mpt_nibbles (mp2-common/src/eth.rs:233-276) of `count` leaves. Per leaf:
 *   loc = parents[i] when parents is given, otherwise `slot` as a 32-byte big-endian integer          (eth.rs:235)
 *   for j = 0 .. n_keys-1, the outer key first: loc = keccak256(keys[i][j] || loc)                    (eth.rs:236-252)
 *   loc += evm_offset, a 256-bit big-endian add                                                       (eth.rs:253-264)
 *   mpt_key = keccak256(loc); nibbles[2 k] = mpt_key[k] >> 4, nibbles[2 k + 1] = mpt_key[k] & 15       (eth.rs:267-276)
 * locations / mpt_keys [count][32], nibbles [count][64] (one nibble per byte: the K public input). keys [count][n_keys][32] are
 * already left_pad32-ed and in the key order of mp2g_leaf_values_digests; n_keys <= 2: deeper nesting, and a mapping below a struct,
 * chain two calls through `parents` [count][32] (the locations of the call before). The reference writes a mapping's slot `as u8`
 * but a simple slot `as u64` (eth.rs:235, :239): slot > 255 with n_keys > 0 and parents NULL is refused, not truncated. The
 * reference's checked_add(..).unwrap() panics when loc + evm_offset leaves 256 bits: here such a leaf gets all three outputs zeroed
 * and is counted in *n_overflow (host in both forms; zeroed by the call). The 64-byte message is built in registers and the leaf's
 * three or four permutations run back to back in one lane: nothing but the outputs touches memory.
 * Each output pointer may be NULL. Refused before any upload or launch: n_keys > 2, the slot above, keys NULL with n_keys != 0, and
 * for _dev any of d_parents / d_keys / d_locations / d_mpt_keys / d_nibbles that is not 8-byte aligned. count == 0 launches nothing
 * and sets *n_overflow to 0. _dev is stream ordered, with one synchronisation when n_overflow is asked for. */
int mp2g_storage_slot_keys(mp2g_ctx* ctx, uint64_t slot, const uint8_t* parents, const uint8_t* keys, uint32_t n_keys,
                           uint32_t evm_offset, uint32_t count, uint8_t* locations, uint8_t* mpt_keys, uint8_t* nibbles,
                           uint32_t* n_overflow);
int mp2g_storage_slot_keys_dev(mp2g_ctx* ctx, uint64_t slot, const uint8_t* d_parents, const uint8_t* d_keys, uint32_t n_keys,
                               uint32_t evm_offset, uint32_t count, uint8_t* d_locations, uint8_t* d_mpt_keys, uint8_t* d_nibbles,
                               uint32_t* n_overflow /* host */);
/* what mp2g_mpt_storage_leaves found in a node */
enum mp2g_mpt_leaf_status {
  MP2G_MPT_LEAF_OK = 0,
  MP2G_MPT_LEAF_MALFORMED = 1,    /* list or item structure, lengths, a header form above 0xf8 */
  MP2G_MPT_LEAF_NOT_A_LEAF = 2,   /* first nibble of the path not 2 or 3: extension nodes included */
  MP2G_MPT_LEAF_BAD_VALUE = 3,    /* item 1 is not the RLP of one string of at most 32 bytes */
  MP2G_MPT_LEAF_KEY_MISMATCH = 4  /* the path is not the tail of mpt_keys[i] */
};
/* MPT storage leaf nodes (mp2-common/src/mpt_sequential/leaf_or_extension.rs:49-87, utils.rs:41-67): nodes [count][stride] bytes,
 * lens [count]. hashes[i] = keccak256(node i), always written, whatever the status. Then the node is opened as an RLP list: the
 * header is 0xc0 + L or 0xf8 L with L >= 56, the payload ends exactly at lens[i], and the list holds exactly two string items.
 * Item 0 is the hex-prefix path (1..33 bytes, at most 64 nibbles): its first nibble is 2 (even) or 3 (odd, the low nibble being the
 * first path nibble); n_nibbles[i] is the path's nibble count, 0..64. The low nibble of an even path's first byte is not judged.
 * Item 1's payload is the RLP of the value: a single byte below 0x80, or 0x80 + n followed by n <= 32 bytes that fill the item
 * exactly. words[i] = left_pad32(value), left_pad_leaf_value's result and the word mp2g_leaf_values_digests takes; the empty string
 * 0x80 gives the zero word. With mpt_keys [count][32] (or NULL) the path's nibbles must equal the last n_nibbles nibbles of
 * mpt_keys[i]. status[i] is an mp2g_mpt_leaf_status, judged in that order: structure, the prefix, the value, the key. On a non-zero
 * status words[i] and n_nibbles[i] are zero. Each of the four outputs may be NULL.
 * The node's bytes are read at offsets that are all below min(lens[i], stride): a hostile length byte cannot read outside the
 * node's row. Refused before any upload or launch: stride as for mp2g_keccak256_batch, nodes or lens NULL, in the host form a
 * lens[i] > stride (named), for _dev a d_nodes / d_hashes / d_words that is not 8-byte aligned (or a d_lens / d_n_nibbles /
 * d_status that is not 4-byte aligned); in the _dev form (every array on the device) a lane clamps its length to stride. count == 0 launches nothing. _dev is stream ordered. */
int mp2g_mpt_storage_leaves(mp2g_ctx* ctx, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, const uint8_t* mpt_keys,
                            uint32_t count, uint8_t* hashes, uint8_t* words, uint32_t* n_nibbles, uint32_t* status);
int mp2g_mpt_storage_leaves_dev(mp2g_ctx* ctx, const uint8_t* d_nodes, uint32_t stride, const uint32_t* d_lens,
                                const uint8_t* d_mpt_keys, uint32_t count, uint8_t* d_hashes, uint8_t* d_words, uint32_t* d_n_nibbles,
                                uint32_t* d_status);

/* ---- MPT inclusion proofs on the device: open nodes, walk paths to the root (csrc/mpt.cuh, csrc/mpt.hip) -------------------------
 * What ProofQuery::verify_storage_proof / verify_state_proof (mp2-common/src/eth.rs:345-399), the walk of
 * mpt_sequential/utils.rs:69-121 and its in-circuit twin Circuit::verify_mpt_proof (mpt_sequential/mod.rs:163-234) compute around
 * a leaf: the leaf is hashed, and for every parent the child's hash is found at the key's nibble in a branch, or after the shared
 * nibbles of an extension, up to the root. Two stages, split the way the data is shared: the proofs of one table share their upper
 * nodes, so every distinct node is hashed and opened once (mp2g_mpt_open_nodes), and the proofs are walked over a table of node
 * indices (mp2g_mpt_verify_paths). Keys have a fixed 64 nibbles (storage and state tries).
 * Out of scope: exclusion proofs (an empty child is a status, not a proof); embedded children, beyond reporting them; receipt and
 * transaction tries, whose keys are not 64 nibbles. The per-node DV / N sums of the reference's branch circuit are the next
 * section's (mp2g_mpt_subtree_digests). */
#define MP2G_MPT_MAX_DEPTH 65 /* 64 branches and a leaf with an empty path */
/* kinds of a node: bits 0-1 of its info word */
#define MP2G_MPT_NODE_INVALID 0
#define MP2G_MPT_NODE_BRANCH 1
#define MP2G_MPT_NODE_EXTENSION 2
#define MP2G_MPT_NODE_LEAF 3
/* why a node is MP2G_MPT_NODE_INVALID: bits 2-4 of its info word */
enum mp2g_mpt_node_reason {
  MP2G_MPT_NODE_MALFORMED = 1,      /* list header, an item's header byte or length, a string of a length its place does not allow */
  MP2G_MPT_NODE_ITEM_COUNT = 2,     /* neither 2 nor 17 items */
  MP2G_MPT_NODE_EMBEDDED_CHILD = 3, /* a child shorter than 32 bytes embedded in its parent: valid Ethereum, not supported here */
  MP2G_MPT_NODE_BRANCH_VALUE = 4,   /* item 16 of a branch is not the empty string */
  MP2G_MPT_NODE_BAD_PREFIX = 5      /* first nibble of the hex-prefix path above 3 */
};
/* how the value of a path's leaf is judged */
#define MP2G_MPT_VALUE_WORD 0    /* storage: the RLP of one string of at most 32 bytes */
#define MP2G_MPT_VALUE_ACCOUNT 1 /* state: the RLP list [nonce, balance, storageHash, codeHash] */
#define MP2G_MPT_VALUE_RAW 2     /* not judged */
/* what mp2g_mpt_verify_paths found on a path */
enum mp2g_mpt_path_status {
  MP2G_MPT_PATH_OK = 0,
  MP2G_MPT_PATH_BAD_PATH = 1,      /* depth outside 1..max_depth, or a node index >= n_nodes */
  MP2G_MPT_PATH_ROOT_MISMATCH = 2, /* the hash of the node at level 0 is not the root */
  MP2G_MPT_PATH_HASH_MISMATCH = 3, /* the hash of a node below level 0 is not what its parent holds for the key */
  MP2G_MPT_PATH_BAD_NODE = 4,      /* a node of kind MP2G_MPT_NODE_INVALID */
  MP2G_MPT_PATH_LEAF_ABOVE = 5,    /* a leaf above the last level */
  MP2G_MPT_PATH_NO_LEAF = 6,       /* a branch or an extension at the last level */
  MP2G_MPT_PATH_KEY_LENGTH = 7,    /* a branch after 64 nibbles, an extension that passes 64, a leaf that does not end at 64 */
  MP2G_MPT_PATH_EMPTY_CHILD = 8,   /* the branch has no child at the key's nibble: an exclusion proof, which this call does not prove */
  MP2G_MPT_PATH_KEY_MISMATCH = 9,  /* the nibbles of an extension or of the leaf are not the key's */
  MP2G_MPT_PATH_BAD_VALUE = 10     /* the leaf's value is not what the mode asks for */
};
/* Stage 1. nodes [n_nodes][stride] bytes and lens [n_nodes], laid out as mp2g_keccak256_batch takes its messages: its stride and
 * alignment rules apply, and a _dev lane clamps its length to the stride. Outputs, each of which may be NULL:
 *   hashes [n_nodes][32]  keccak256(node), written for every node whatever its structure
 *   info [n_nodes]        what the node is, packed so that the walk needs no second scan:
 *     bits 0-1            kind: MP2G_MPT_NODE_INVALID, _BRANCH, _EXTENSION, _LEAF
 *     bits 2-4            an mp2g_mpt_node_reason when the kind is INVALID (every other bit is then 0), else 0
 *     bits 5-6            length of the list header (1, 2 or 3)
 *     bit 7               0
 *     bits 8-23           branch: 16-bit mask of the non-empty children, bit k for nibble k; bits 24-31 are 0
 *     bits 8-14           extension / leaf: nibble count of the path (extension 1..64, leaf 0..64); bit 15 is 0
 *     bits 16-31          extension / leaf: byte offset of item 1's header byte
 * The rules by which a node is judged, in their order:
 * 1. List header. Accepted forms: 0xc0+L (L < 56), 0xf8 L (L >= 56), or 0xf9 hi lo (L >= 256). The payload must end exactly at
 *    lens[i]. Anything else is MALFORMED. (mp2g_mpt_storage_leaves accepts only the first two forms; real 532-byte branch nodes
 *    start f9 02 11.)
 * 2. Items. An item is a string: a single byte below 0x80, 0x80+k with k <= 55, or 0xb8 k with k >= 56. Or it is a short list
 *    0xc0+k, k <= 55. A short list is only recognised, never entered. The items are scanned in order. A header byte outside these
 *    forms is MALFORMED, and so is an item that runs past the payload: the first such item decides. A node has 2 or 17 items that
 *    fill the payload exactly. Any other count is ITEM_COUNT; the scan ends where an 18th item begins, without judging it.
 * 3. 17 items: a branch. Each of items 0..15 is either the empty string 0x80 (mask bit clear) or a 32-byte string 0xa0 ... (mask
 *    bit set). A list item is EMBEDDED_CHILD. A string of any other length is MALFORMED. Item 16 must be the empty string, else
 *    BRANCH_VALUE: the keys have a fixed 64 nibbles, so a branch never holds a value. The first offending item decides. With the
 *    mask, the child at nibble k lies at header_len + k + 32 * popcount(mask & ((1 << k) - 1)) + 1. The walk relies on this.
 * 4. 2 items: the hex-prefix path is item 0, a string of 1..33 bytes, else MALFORMED. Its first nibble selects the kind: 0 or 1 is
 *    an extension, 2 or 3 is a leaf, anything else is BAD_PREFIX; an odd first nibble makes the byte's low nibble the first of the
 *    path, and the low nibble of an even path's first byte is not judged. The nibble count is at most 64; 65 nibbles is MALFORMED.
 *    For an extension: at least 1 nibble, else MALFORMED; item 1 is a 32-byte string; a list as item 1 is EMBEDDED_CHILD; any other
 *    item 1 is MALFORMED. For a leaf, item 1 is any string that ends the list (a list is MALFORMED). Its content is judged by the
 *    walk, per value mode.
 * Every byte is read at an offset below min(lens[i], stride): a hostile length byte cannot read outside the node's row.
 * Refused before any upload or launch, with a message that names the argument: stride as for mp2g_keccak256_batch; nodes or lens
 * NULL; in the host form a lens[i] > stride (named); for _dev a d_nodes / d_hashes that is not 8-byte aligned or a d_lens / d_info
 * that is not 4-byte aligned. A refused call writes nothing; n_nodes == 0 launches nothing; _dev is stream ordered. */
int mp2g_mpt_open_nodes(mp2g_ctx* ctx, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, uint32_t n_nodes, uint8_t* hashes,
                        uint32_t* info);
int mp2g_mpt_open_nodes_dev(mp2g_ctx* ctx, const uint8_t* d_nodes, uint32_t stride, const uint32_t* d_lens, uint32_t n_nodes,
                            uint8_t* d_hashes, uint32_t* d_info);
/* Stage 2, one lane per proof. The node table with stage 1's hashes and info (the host form takes the table alone and runs stage
 * 1 itself); paths [count][max_depth] node indices, root first, as eth_getProof orders them; depths [count]; mpt_keys [count][32];
 * roots with root_stride 0 (one root for all paths) or 32 (one per path), or roots NULL: the root is not checked; a value mode.
 * max_depth is at most MP2G_MPT_MAX_DEPTH.
 * The walk starts with ptr = 0 (nibbles consumed) and expected = root. For level l = 0 .. depth-1:
 * 1. Index. depth outside 1..max_depth, or an index >= n_nodes, is BAD_PATH.
 * 2. Hash. hashes[idx] != expected is ROOT_MISMATCH at level 0 and HASH_MISMATCH below it.
 * 3. Node. Kind 0 is BAD_NODE (so is, in the _dev form, an info word that does not fit its node's length: no bit of it is trusted
 *    for a read).
 * 4. Position. A leaf above the last level is LEAF_ABOVE. A non-leaf at the last level is NO_LEAF.
 * 5. Branch. ptr == 64 is KEY_LENGTH. A clear mask bit for nibble key[ptr] is EMPTY_CHILD. Otherwise expected becomes that child
 *    and ptr becomes ptr + 1.
 * 6. Extension with n nibbles. ptr + n > 64 is KEY_LENGTH. The nibbles are compared with key[ptr .. ptr+n): a difference is
 *    KEY_MISMATCH. expected becomes item 1 and ptr becomes ptr + n.
 * 7. Leaf with n nibbles. ptr + n != 64 is KEY_LENGTH. The nibbles are compared, and a difference is KEY_MISMATCH. Then the value,
 *    item 1's payload, is judged by mode:
 *      MP2G_MPT_VALUE_WORD     the RLP of one string of <= 32 bytes, by exactly the rules of mp2g_mpt_storage_leaves, else BAD_VALUE;
 *                              words[i] = left_pad32(value)
 *      MP2G_MPT_VALUE_ACCOUNT  an RLP list (0xc0+L or 0xf8 L) of exactly four strings that fills the payload, items 2 and 3 of 32
 *                              bytes (nonce, balance, storageHash, codeHash), else BAD_VALUE; words[i] = item 2, the storage root
 *      MP2G_MPT_VALUE_RAW      not judged, and words is not written
 * The first failing level decides; within a level the order is the one above. The words of an ACCOUNT call are, as they lie on the
 * device, the roots (root_stride 32) of a WORD call: state root -> account -> storage root -> leaf word without a download.
 * Outputs, each of which may be NULL: status [count], an mp2g_mpt_path_status; fail_level [count], 0 on success; words [count][32],
 * zero on failure; val_off / val_len [count], item 1's payload inside the leaf node, zero on failure; consumed [count][max_depth]
 * (bytes): the value of ptr on entering each level, which is what the reference's key pointer counts from the other end, 0xff for
 * the levels after the failing one or past depth (all of them when depth itself is refused).
 * Refused before any upload or launch, with a message that names the argument: the table as for mp2g_mpt_open_nodes; NULL paths,
 * depths, mpt_keys, d_hashes or d_info; max_depth 0 or above 65; a root_stride that is neither 0 nor 32; an unknown mode; in the
 * host form the first depths[i] above max_depth (named); for _dev d_nodes / d_hashes / d_roots / d_words not 8-byte aligned, any
 * u32 array not 4-byte aligned. A path index >= n_nodes is a per-proof status, not a refusal. A refused call writes nothing;
 * count == 0 launches nothing; _dev is stream ordered. */
int mp2g_mpt_verify_paths(mp2g_ctx* ctx, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, uint32_t n_nodes,
                          const uint32_t* paths, const uint32_t* depths, uint32_t max_depth, const uint8_t* mpt_keys, uint32_t count,
                          const uint8_t* roots, uint32_t root_stride, uint32_t mode, uint32_t* status, uint32_t* fail_level,
                          uint8_t* words, uint32_t* val_off, uint32_t* val_len, uint8_t* consumed);
int mp2g_mpt_verify_paths_dev(mp2g_ctx* ctx, const uint8_t* d_nodes, uint32_t stride, const uint32_t* d_lens, const uint8_t* d_hashes,
                              const uint32_t* d_info, uint32_t n_nodes, const uint32_t* d_paths, const uint32_t* d_depths,
                              uint32_t max_depth, const uint8_t* d_mpt_keys, uint32_t count, const uint8_t* d_roots,
                              uint32_t root_stride, uint32_t mode, uint32_t* d_status, uint32_t* d_fail_level, uint8_t* d_words,
                              uint32_t* d_val_off, uint32_t* d_val_len, uint8_t* d_consumed);

/* ---- MPT subtree digests on the device: DV and N of every trie node (csrc/mpt_graph.cuh, csrc/mpt_digest.hip) ---------------------
 * What every node of the storage trie exposes in the values-extraction proofs (mp2-v1/src/values_extraction/public_inputs.rs:23-36:
 * H, K, T, DV, DM, N): a branch's DV and N are the sums over its proved children (branch.rs:77-112), an extension passes its
 * child's on (extension.rs:53-61), a leaf has its own digest and N = 1. The trie's shape is taken from the proofs themselves, over
 * the node table, info words, paths and keys of mp2g_mpt_verify_paths; node bytes are not read, and no hash is checked again:
 * d_status [count] is what a walk over the same tables left (NULL: every proof counts as MP2G_MPT_PATH_OK). Whatever the arrays
 * hold, no index is used before it is held against n_nodes.
 *
 * Accepted proofs. Proof i counts when d_status is NULL or d_status[i] is MP2G_MPT_PATH_OK, depths[i] is in 1..max_depth, every
 * index is below n_nodes, every level but the last is a BRANCH or an EXTENSION and the last a LEAF, and ptr (0 at the root, + 1 at a
 * branch, + the info word's nibble count at an extension or leaf) never passes 64 and is 64 after the leaf. Any other proof
 * contributes nothing anywhere and is counted in n_rejected.
 * Occurrences. An accepted proof gives its node x = path[l] the tuple (parent, level, entered, slot): parent = path[l-1], or
 * MP2G_MPT_NO_NODE at level 0; level = l; entered = ptr on entering x; slot = the key's nibble at the parent's `entered` below a
 * branch, 0 below an extension and at level 0. via[x] is the lowest index of an accepted proof through x, and x's reference
 * occurrence the one at the lowest level of proof via[x].
 * Conflicts, in this order: (a) an occurrence of x whose tuple is not the reference occurrence's makes x and that occurrence's own
 * parent MP2G_MPT_SUBTREE_CONFLICT; (b) two different nodes with one (parent, slot) make the parent a CONFLICT (the lower index is
 * kept as the child); (c) a node with a CONFLICT child is a CONFLICT, up to the root. A node table deduplicated by bytes is not a
 * tree: two leaves with equal tails and values below two nibbles of one branch are one entry, their digests differ (the mapping
 * key enters a leaf's digest), and a per-node digest does not exist there. The call says so; it does not sum silently.
 * Several accepted proofs that end at one leaf node with one tuple are one leaf: it counts once, with the digest of proof via[x].
 * Sums. d_leaf_frac [count][20]: the leaves' digests by proof, as mp2g_leaf_values_digests_dev leaves them in d_frac_out. A LEAF
 * takes d_leaf_frac[via[x]] and N = 1; an EXTENSION its child's point and N; a BRANCH the sum (the complete addition) of the
 * children the proofs showed, in nibble order, and the sum of their N: a child no proof showed costs nothing. A CONFLICT or
 * UNREACHED node gets the neutral point and N = 0. Points stay in fractional coordinates: compare them through mp2g_curve_emit_dev.
 * Outputs, each of which may be NULL: d_acc_frac [n_nodes][20] (NULL: no point is read or added, and d_leaf_frac may be NULL);
 * d_n_leaves, d_state (an mp2g_mpt_subtree_state), d_via, d_parent [n_nodes] u32; d_entered [n_nodes] bytes; totals (host):
 * rejected proofs, CONFLICT nodes, levels (1 + the deepest level of a reached node). via, parent and entered are the reference
 * occurrence's, for a CONFLICT node too; an UNREACHED node has via = parent = MP2G_MPT_NO_NODE and entered = 0xff.
 * Four launches over the proofs (minima; the owner of each node writes its tuple; compare and OR; rule (c)), three over the nodes,
 * then one launch per level from the deepest up. Launches are the only ordering, every shared word is an integer minimum or an OR,
 * and no result depends on the schedule. One synchronisation, for the level counts and the totals. The context keeps a working
 * buffer of 100 bytes per node (64 of them the child table) and one per proof, which grows, with one more synchronisation, when
 * a call needs more.
 * Refused before any upload or launch, with a message that names the argument: d_info NULL with n_nodes != 0; d_paths, d_depths or
 * d_mpt_keys NULL with count != 0; d_leaf_frac NULL with d_acc_frac given and count != 0; max_depth 0 or above 65; d_leaf_frac /
 * d_acc_frac not 8-byte aligned, any u32 array not 4-byte aligned; d_leaf_frac and d_acc_frac overlapping. A rejected proof and a
 * conflict are outputs, not refusals. n_nodes == 0 launches nothing (every proof is rejected); count == 0 launches no kernel and
 * fills the outputs with the UNREACHED values. */
#define MP2G_MPT_NO_NODE 0xffffffffu
enum mp2g_mpt_subtree_state { MP2G_MPT_SUBTREE_UNREACHED = 0, MP2G_MPT_SUBTREE_OK = 1, MP2G_MPT_SUBTREE_CONFLICT = 2 };
int mp2g_mpt_subtree_digests_dev(mp2g_ctx* ctx, const uint32_t* d_info, uint32_t n_nodes, const uint32_t* d_paths, const uint32_t* d_depths,
                                 uint32_t max_depth, const uint8_t* d_mpt_keys, const uint32_t* d_status /* or NULL */, uint32_t count,
                                 const uint64_t* d_leaf_frac /* [count][20] */, uint64_t* d_acc_frac /* [n_nodes][20] */,
                                 uint32_t* d_n_leaves, uint32_t* d_state, uint32_t* d_via, uint32_t* d_parent, uint8_t* d_entered,
                                 uint32_t totals[3] /* host: rejected proofs, conflict nodes, levels */);
/* The same from host arrays: the node table, paths, keys, roots and mode as mp2g_mpt_verify_paths takes them, and the leaves'
 * digests as encodings leaf_w [count][5] (by proof). The call runs mp2g_mpt_open_nodes, mp2g_mpt_verify_paths (status [count], or
 * NULL, receives its statuses), mp2g_curve_decode_dev, the pass and mp2g_curve_emit_dev itself. out_w [n_nodes][5] /
 * out_weierstrass [n_nodes][11]: every node's sum; with both NULL no point is decoded or added and leaf_w may be NULL. The other
 * outputs are the _dev form's, in host memory. Refused: what those calls refuse, and leaf_w NULL when a point output is given. */
int mp2g_mpt_subtree_digests(mp2g_ctx* ctx, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, uint32_t n_nodes,
                             const uint32_t* paths, const uint32_t* depths, uint32_t max_depth, const uint8_t* mpt_keys, uint32_t count,
                             const uint8_t* roots, uint32_t root_stride, uint32_t mode, const uint64_t* leaf_w /* [count][5] */,
                             uint32_t* status /* [count], out */, uint64_t* out_w /* [n_nodes][5] */, uint64_t* out_weierstrass /* [n_nodes][11] */,
                             uint32_t* n_leaves, uint32_t* state, uint32_t* via, uint32_t* parent, uint8_t* entered, uint32_t totals[3]);

/* ---- proof wire format between tree levels / GPUs ------------------------------------------ */
/* bincode 1.3 (little-endian fixed-width ints, u64 length prefixes) serialization of plonky2's
 * ProofWithPublicInputs<F, C, 2> exactly as mp2-common/src/proof.rs:84-98 `serialize_proof`
 * produces it, from the prover's flat outputs. `caps` = [n_oracles][1<<cap][4] (oracle 0, the
 * preprocessed one, is not part of a proof and is skipped); `openings` as produced by the prover
 * ([sum w][2] at zeta in oracle order, then [zs_count][2] at g*zeta); the first num_constants
 * polynomials of oracle 0 are `constants`, the rest `plonk_sigmas`; the first zs_count of oracle
 * zs_oracle are `plonk_zs`, then `partial_products`, then (num_lookup_polys > 0) `lookup_zs`, whose values at
 * g*zeta are `lookup_zs_next`.
 * Call with out = NULL to get the size in *out_len. */
int mp2g_proof_serialize(const mp2g_fri_params* params, uint32_t num_constants, const uint64_t* caps,
                         const uint64_t* openings, const uint64_t* fri_proof, const uint64_t* public_inputs,
                         uint32_t n_public_inputs, uint8_t* out, size_t* out_len);
/* inverse of the above; all output arrays sized as the prover's; fails on malformed input */
int mp2g_proof_deserialize(const mp2g_fri_params* params, uint32_t num_constants, const uint8_t* bytes, size_t len,
                           uint64_t* caps, uint64_t* openings, uint64_t* fri_proof, uint64_t* public_inputs,
                           uint32_t n_public_inputs);
/* ProofWithVK::serialize (mp2-common/src/proof.rs:42-52): bincode(proof) followed by the verifier
 * key as a length-prefixed byte blob (plonky2 VerifierOnlyCircuitData::to_bytes: cap HEIGHT as
 * u64, the cap hashes, the circuit digest). vk_cap_len must be a power of two. */
int mp2g_proof_with_vk_serialize(const uint8_t* proof_bytes, size_t proof_len, const uint64_t* vk_cap,
                                 uint32_t vk_cap_len, const uint64_t vk_circuit_digest[4], uint8_t* out, size_t* out_len);
/* ProofWithVK::deserialize (mp2-common/src/proof.rs:54-57), the inverse: the proof's parts as mp2g_proof_deserialize hands
 * them out, then the verifier key -- vk_cap [vk_cap_len][4] (the caller states the cap length it expects: a blob with
 * another cap height is refused) and the circuit digest. What a proof store (mp2-v1/tests/common/proof_storage.rs:139-140
 * `get_proof_exact`) returns is fed to this before the proof enters its parent's witness. */
int mp2g_proof_with_vk_deserialize(const mp2g_fri_params* params, uint32_t num_constants, const uint8_t* bytes, size_t len,
                                   uint64_t* caps, uint64_t* openings, uint64_t* fri_proof, uint64_t* public_inputs,
                                   uint32_t n_public_inputs, uint64_t* vk_cap, uint32_t vk_cap_len,
                                   uint64_t vk_circuit_digest[4]);

/* ---- permutation argument: replaces plonk/prover.rs all_wires_permutation_partial_products ---- */
/* wires [wires_w][n] and sigmas [num_routed][n]: subgroup values (natural order); only the first
 * num_routed wire columns are read. degree = quotient_degree_factor (8 in standard_recursion_config),
 * num_routed % degree == 0. out [nc * num_routed/degree][n] in the order prove() commits:
 * Z of every challenge, then each challenge's num_routed/degree - 1 partial products. */
int mp2g_partial_products_and_zs(mp2g_ctx* ctx, const uint64_t* wires, uint32_t wires_w, const uint64_t* sigmas,
                                 uint32_t log_n, uint32_t num_routed, uint32_t degree, const uint64_t* betas,
                                 const uint64_t* gammas, uint32_t nc, uint64_t* out);
/* Let the batched prover compute oracle 2 itself (d_values[1] of mp2g_prover_prove_dev may then be
 * NULL): the sigmas are the last num_routed polynomials of the preprocessed oracle, betas/gammas
 * the challenges drawn after the wires cap. Call after mp2g_prover_set_preprocessed_dev. */
int mp2g_prover_enable_permutation(mp2g_prover* pr, uint32_t num_routed, uint32_t degree);
/* Also compute oracle 3 (the quotient chunks) on the device, as plonk/prover.rs compute_quotient_polys
 * does: the vanishing terms Z(1) = 1 and the partial-product checks, plus the gate constraints once
 * mp2g_prover_set_gates has given the gate table (without a table: the complete prove() of a circuit whose
 * only constraints are copy constraints). d_values[2] may then be NULL. Needs
 * mp2g_prover_enable_permutation, rate_bits 3 and oracle_w[3] = zs_count * 8. */
int mp2g_prover_enable_quotient(mp2g_prover* pr);

/* PublicInputGate's witness generator on the device: before the wires are committed, every proof's
 * d_pi_hash[b][0..4) is written to wires 0..3 of row `row` (the circuit's PublicInputGate row) of its wire
 * matrix, IN PLACE in d_values[0] of mp2g_prover_prove_dev. A batch of proofs of one circuit that differ only
 * in their public inputs can then share one witness template (the aggregation levels of
 * recursion-framework/tests/integration.rs:138-261). row < 0 turns it off. */
int mp2g_prover_bind_public_inputs(mp2g_prover* pr, int64_t row);

/* plonky2's prove() panics on a witness that violates a constraint (the reference's tests depend on it:
 * recursion-framework/src/framework.rs:694-700). With the check on, every mp2g_prover_prove_dev also
 * evaluates, per proof, the gate constraints on the subgroup (needs mp2g_prover_set_gates) and the
 * wrap-around of the permutation product; mp2g_prover_witness_status synchronises and returns non-zero with
 * a message naming the first offending proof. flags (may be NULL) receives one word per proof: bit 0 a
 * copy constraint, bit 1 a gate constraint, bit 2 the lookup argument (a looked-up pair that is not in its table). The proof itself is still produced (it does not verify). */
int mp2g_prover_enable_witness_check(mp2g_prover* pr, int on);
/* prove only the first n <= batch witnesses from the next call on (every buffer is proof-major, so a prover created for `batch`
 * proofs serves any smaller batch without new allocations: the narrow levels of a tree reuse the wide levels' prover) */
int mp2g_prover_set_active(mp2g_prover* pr, uint32_t n);
int mp2g_prover_witness_status(mp2g_prover* pr, uint32_t* flags);
int mp2g_prover_witness_check_enabled(const mp2g_prover* pr);
/* Replay the prover's launch sequence (several hundred small kernels per call) as a hipGraph: the
 * first call after enabling runs normally (it creates the cached twiddle tables), the second is captured,
 * later calls with the same buffer addresses launch the instantiated graph. A call with different
 * addresses re-captures. Cuts the launch-bound latency of small batches; results are identical. */
int mp2g_prover_enable_graph(mp2g_prover* pr, int on);
/* Stage timing of the batched prover (measurement aid; plonky2 prints the same split through its
 * `timed!` macro inside prove()). With timing on, every mp2g_prover_prove_dev records HIP events on
 * the prover's stream at the phase boundaries; mp2g_prover_stage_ms synchronises and returns the
 * milliseconds of the last call: 0 wires commitment, 1 Z / partial products + commitment, 2 quotient
 * polynomials + commitment, 3 openings, 4 FRI batch composition + commit phase, 5 proof of work,
 * 6 query rounds. */
#define MP2G_N_STAGES 7
int mp2g_prover_enable_timing(mp2g_prover* pr, int on);
int mp2g_prover_stage_ms(mp2g_prover* pr, float out[MP2G_N_STAGES]);

/* ---- gate constraints: the third part of compute_quotient_polys --------------------------------
 * Replaces [dep] plonky2 plonk/vanishing_poly.rs evaluate_gate_constraints_base_batch and the
 * eval_unfiltered_base of the gates below: all 26 entries the reference registers
 * (mp2-common/src/serialization/circuit_data_serialization.rs:236-267). */
enum {
  MP2G_GATE_NOOP = 0,
  MP2G_GATE_CONSTANT = 1,       /* p0 = num_consts */
  MP2G_GATE_PUBLIC_INPUT = 2,
  MP2G_GATE_ARITHMETIC = 3,     /* p0 = num_ops */
  MP2G_GATE_BASE_SUM = 4,       /* p0 = num_limbs, p1 = base (BaseSumGate<B>) */
  MP2G_GATE_ARITHMETIC_EXT = 5, /* p0 = num_ops (D = 2) */
  MP2G_GATE_MUL_EXT = 6,        /* p0 = num_ops */
  MP2G_GATE_POSEIDON2 = 7,
  MP2G_GATE_EXPONENTIATION = 8, /* p0 = num_power_bits */
  MP2G_GATE_REDUCING = 9,       /* p0 = num_coeffs */
  MP2G_GATE_REDUCING_EXT = 10,  /* p0 = num_coeffs */
  MP2G_GATE_RANDOM_ACCESS = 11, /* p0 = bits (<= 6), p1 = num_copies, p2 = num_extra_constants */
  MP2G_GATE_POSEIDON = 12,      /* the original Poseidon permutation gate (wrap circuits) */
  MP2G_GATE_POSEIDON_MDS = 13,
  MP2G_GATE_COSET_INTERPOLATION = 14, /* p0 = subgroup_bits (2..5), p1 = degree (CosetInterpolationGate::degree) */
  /* plonky2-u32 (restated from memory of the published crate, like everything here that is not in the tree) */
  MP2G_GATE_U32_ARITHMETIC = 15,  /* p0 = num_ops */
  MP2G_GATE_U32_RANGE_CHECK = 16, /* p0 = num_input_limbs */
  MP2G_GATE_U32_SUBTRACTION = 17, /* p0 = num_ops */
  MP2G_GATE_U32_ADD_MANY = 18,    /* p0 = num_addends (<= 16), p1 = num_ops */
  MP2G_GATE_COMPARISON = 19,      /* p0 = num_bits, p1 = num_chunks (chunks of at most 4 bits) */
  /* plonky2 gates/lookup.rs, gates/lookup_table.rs: no constraints of their own, the lookup argument of prove()
   * (mp2g_prover_set_lookups) carries them. p0 = num_slots (num_routed / 2, num_routed / 3) */
  MP2G_GATE_LOOKUP = 20,
  MP2G_GATE_LOOKUP_TABLE = 21,
  /* plonky2_crypto u32/gates/{interleave_u32, uninterleave_to_b32, uninterleave_to_u32}.rs (Keccak / SHA in the MPT
   * circuits), restated from memory of the published crate: p0 = num_ops */
  MP2G_GATE_U32_INTERLEAVE = 22,
  MP2G_GATE_UNINTERLEAVE_TO_B32 = 23,
  MP2G_GATE_UNINTERLEAVE_TO_U32 = 24
};
#define MP2G_MAX_GATES 32
#define MP2G_MAX_GATE_CONSTRAINTS 160
/* One entry per gate of CommonCircuitData::gates, in that order (sorted by degree). The selector
 * fields restate SelectorsInfo (gates/selectors.rs): the gate's filter is
 * prod_{r in [group_start, group_end), r != index} (r - s) * (num_selectors > 1 ? (u32::MAX - s) : 1)
 * with s = local_constants[selector_index]. */
typedef struct {
  uint32_t kind, p0, p1, p2;
  uint32_t selector_index, group_start, group_end;
} mp2g_gate;
/* Gate::num_constraints / Gate::degree of a descriptor; 0 for an unknown kind and for a malformed descriptor: a parameter outside
 * the range documented above, an operation / slot / limb / coefficient count of 0 where the gate needs one, or a wire or
 * constraint count that does not fit 32 bits */
uint32_t mp2g_gate_num_constraints(const mp2g_gate* g);
uint32_t mp2g_gate_degree(const mp2g_gate* g);
/* Give the batched prover the gate table: the quotient then carries the gate constraint terms after
 * the permutation terms (eval_vanishing_poly_base_batch order), i.e. the complete prove() of a circuit
 * built from the gates above. Constants are the first oracle_w[0] - num_routed polynomials of the
 * preprocessed oracle (selectors first, then the gate constants); the public-inputs hash is the
 * d_pi_hash of mp2g_prover_prove_dev. Needs mp2g_prover_enable_quotient. n_gates = 0 removes it. */
int mp2g_prover_set_gates(mp2g_prover* pr, const mp2g_gate* gates, uint32_t n_gates, uint32_t num_selectors);
/* One lookup table of the circuit: plonky2's LookupWire (the rows CircuitBuilder::add_all_lookups appended for it:
 * LookupGate rows [last_lu_row, last_lut_row), LookupTableGate rows [last_lut_row, first_lut_row] with the table
 * running DOWN from first_lut_row, then a Noop row) and the table itself (CommonCircuitData::luts). */
typedef struct {
  uint32_t last_lu_row, last_lut_row, first_lut_row;
  uint32_t table_len;
  const uint16_t* table; /* [table_len][2] = (input, output), host pointer */
} mp2g_lookup;
#define MP2G_MAX_LUTS 16
/* The lookup argument of prove() ([dep] plonk/prover.rs compute_lookup_polys, vanishing_poly.rs
 * check_lookup_constraints): after the wires cap the transcript also yields the lookup challenges (deltas = betas,
 * gammas and 2 * num_challenges more), the RE / Sum / LDC polynomials are computed on the device into the tail of
 * oracle 2, and their constraints enter the quotient between the partial-product and the gate terms. The constants
 * of the preprocessed oracle are then: selectors, the 4 + n_luts lookup selectors (gates/selectors.rs
 * selectors_lookup, selector_ends_lookups), gate constants. Needs mp2g_prover_set_gates (with the LookupGate /
 * LookupTableGate entries), params.num_lookup_polys = ceil((num_routed/2) / (degree-1)) + 1 and
 * oracle_w[2] = zs_count * (num_routed/degree + num_lookup_polys). The multiplicity wires are part of the witness:
 * mp2g_prover_lookup_wires_dev fills them on the device, as do the witness tape's replays for a program that has the
 * tables (mp2g_witness_program_set_lookups). n_luts = 0 removes the argument. */
int mp2g_prover_set_lookups(mp2g_prover* pr, const mp2g_lookup* luts, uint32_t n_luts);
/* prove()'s set_lookup_wires ([dep] plonk/prover.rs) for a batch, in place, stream ordered on the prover's context; needs
 * mp2g_prover_set_lookups. For hosts that keep plonky2's generators and use only the prover. Per table t: lookup j < n_lookups[t]
 * sits at row last_lu_row + j / 40, wires 2 (j % 40), + 1 and is READ; every later slot of the table's LookupGate rows is
 * padding and receives the table's first pair; entry e of the table goes to row first_lut_row - e / 26, wires 3 (e % 26) .. + 2 =
 * input, output, multiplicity = the number of LookupGate slots of the table (padding included) that hold the entry's pair; the
 * LookupTableGate slots past the table's end get zeros. No other wire is touched. A slot whose pair is in no entry is not
 * counted and nothing fails here: that proof fails the lookup argument (witness-check flag 4). Refused: n_lookups[t] above
 * the table's 40 x rows slots; a table that holds an input twice (set_lookups itself accepts such a table). */
int mp2g_prover_lookup_wires_dev(mp2g_prover* pr, const uint32_t* n_lookups /* [n_luts] */, uint64_t* d_wires /* [batch][wires_w][n] */, uint32_t batch);

/* The filtered constraints C_j = sum_gates filter_g c_{g,j} at npts arbitrary points (host pointers):
 * consts [num_constants][npts], wires [wires_w][npts], out [max_j][npts] with max_j the largest
 * num_constraints of the table. On the subgroup H a satisfied witness gives all zeros -- the check
 * behind plonky2's "invalid witness" panic in prove(). */
int mp2g_eval_gate_constraints(mp2g_ctx* ctx, const mp2g_gate* gates, uint32_t n_gates, uint32_t num_selectors,
                               const uint64_t* consts, uint32_t num_constants, const uint64_t* wires, uint32_t wires_w,
                               uint64_t npts, const uint64_t pi_hash[4], uint64_t* out);
/* The quotient-side sibling: the alpha-reduced gate term of prove()'s quotient, sum_j alpha_{b,a}^j C_j, for B proofs at
 * N = 2^log_points points each (1 <= log_points <= 24), computed by the launchers prove() itself runs on the LDE (the per-kind
 * kernels, the fused launch of the light gates, one alpha-power table per batch). Host pointers: consts [num_constants][N]
 * shared by the batch -- selectors, then num_lookup_selectors rows the gates never read, then the gate constants --,
 * wires [B][wires_w][N], alphas [B][nc] with nc = 1 or 2, pi_hash [B][4], out [B][nc][N].
 * POINT ORDER: column p of consts / wires is memory column p of the prover's bit-reversed LDE matrices; its result lands at
 * out[b][a][bitrev(p, log_points)], the natural order the quotient is divided and committed in.
 * Refused before anything is launched, with `out` untouched: a word >= p in consts, wires, alphas or pi_hash (the kernels take
 * canonical words only), nc outside 1..2, B = 0, a gate table mp2g_prover_set_gates would refuse. A table without constraints
 * (Noops, lookup gates) is valid and gives zeros. */
int mp2g_eval_gate_constraints_lde(mp2g_ctx* ctx, const mp2g_gate* gates, uint32_t n_gates, uint32_t num_selectors,
                                   uint32_t num_lookup_selectors, const uint64_t* consts, uint32_t num_constants,
                                   const uint64_t* wires, uint32_t wires_w, uint32_t log_points, uint32_t B, const uint64_t* alphas,
                                   uint32_t nc, const uint64_t* pi_hash, uint64_t* out);

/* ---- batched proof verification on the device (csrc/verifier.hip) --------------------------------
 * Replaces [dep] plonky2 plonk/verifier.rs verify / verify_with_challenges and fri/verifier.rs verify_fri_proof -- the other half
 * of every proving call: VerifierCircuitData::verify as reached from mp2-common/src/utils.rs:47-59 (verify_proof_tuple),
 * verifiable-db/src/api.rs:448-452 and ProofWithVK::verify (mp2-common/src/proof.rs) -- for `count` proofs of ONE circuit per call.
 * Everything runs on the context's stream; one synchronisation at the end reads the statuses. No CPU path.
 *
 * A verifier holds the VerifierCircuitData of one circuit: VerifierOnlyCircuitData (constants_sigmas cap [1 << cap_height][4], circuit
 * digest) and what verify() reads of CommonCircuitData (FRI parameters, num_routed, the quotient degree factor `degree`, the gate
 * table with its selector groups, the lookup tables). n_public_inputs = MP2G_PI_HASH_GIVEN: part 0 of a proof is the 4-word
 * public-inputs hash itself instead of the list verify() hashes first. `capacity` = the most proofs one call takes.
 * Create fails for a gate table the prover would refuse, lookup tables that do not match params->num_lookup_polys, or a table whose
 * filtered constraints would need more than 32 line points (mp2g_gate_table_line_points).
 *
 * STATUS, one word per proof, the first failing check in this order (the codes of the CPU oracle's verifier, so that the two compare
 * for equality): 20 a word >= p somewhere in the proof (checked first; such a proof takes no further part); 10 + a the PLONK
 * identity vanishing(zeta) = Z_H(zeta) * sum_i zeta^(n i) t_i(zeta) fails for challenge round a; 1 proof of work; then the FIRST
 * failing check of the LOWEST failing query round: 2 a Merkle path of an initial oracle, 3 a FRI layer's evaluation does not
 * continue the previous layer, 4 a FRI layer's Merkle path, 5 the final polynomial. 0 = accept. A rejected proof never affects
 * another proof of the batch. The functions return 0 when the call ran, whatever the statuses. */
typedef struct mp2g_verifier mp2g_verifier;
#define MP2G_PI_HASH_GIVEN 0xFFFFFFFFu
int mp2g_verifier_create(mp2g_ctx* ctx, const mp2g_fri_params* params, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                         uint32_t num_routed, uint32_t degree, const mp2g_gate* gates, uint32_t n_gates, uint32_t num_selectors,
                         const mp2g_lookup* luts, uint32_t n_luts, uint32_t n_public_inputs, uint32_t capacity, mp2g_verifier** out);
/* words of one proof = the lengths of its four parts, in a parent's input order: public inputs (n_public_inputs, or 4 for the hash),
 * caps of oracles 1 .. n_oracles - 1, openings (2 * mp2g_fri_n_openings), FRI words (mp2g_fri_proof_words). part_words (may be NULL)
 * receives the four lengths. */
size_t mp2g_verifier_proof_words(const mp2g_verifier* v, uint32_t part_words[4]);
/* Proofs where the prover / chain left them: four device parts per proof, each a base pointer and a stride in words between
 * consecutive proofs -- mp2g_prover_prove_dev's outputs (d_pi_hash; d_caps + one cap, stride n_oracles caps; d_openings; d_proof) and
 * mp2g_chain_step_buffers fit as they are. status [count]: host memory. */
int mp2g_verifier_verify_dev(mp2g_verifier* v, const uint64_t* const d_parts[4], const uint64_t strides[4], uint32_t count, uint32_t* status);
/* contiguous proofs of mp2g_verifier_proof_words words each, in a parent's input order (what mp2g_forest_proof returns), host memory */
int mp2g_verifier_verify(mp2g_verifier* v, const uint64_t* words, uint32_t count, uint32_t* status);
/* The challenges the last call derived, per proof (so that a transcript mismatch is found by comparing a few words and not by
 * bisecting a rejected proof): betas [2], gammas [2], alphas [2], zeta [2], the 8 lookup challenges of the two rounds (betas,
 * gammas and 4 more; zero without lookup tables), FRI alpha [2], FRI betas [n_layers][2], the proof-of-work response, the
 * num_queries query indices (already reduced mod the LDE size). out (may be NULL) [count of the last call][*words_per_proof]. */
int mp2g_verifier_challenges(mp2g_verifier* v, uint64_t* out, size_t* words_per_proof);
void mp2g_verifier_free(mp2g_verifier* v);
/* The number T of base-field points the verifier evaluates the gate constraints at (see DESIGN.md "Verifier"): 1 + the largest
 * degree of a filtered constraint = 1 + max over gates of degree + (selector group size - 1) + (num_selectors > 1). Pure host
 * arithmetic: needs no GPU. 0 for an unknown gate kind, a malformed descriptor (as for mp2g_gate_degree) or an empty selector group. */
uint32_t mp2g_gate_table_line_points(const mp2g_gate* gates, uint32_t n_gates, uint32_t num_selectors);

/* ---- witness generation: the witness tape ------------------------------------------------------------------
 * Replaces [dep] plonky2 iop/generator.rs generate_partial_witness -- the first line of prove() at
 * recursion-framework/src/circuit_builder.rs:308 and universal_verifier_gadget/wrap_circuit.rs:143 -- for circuits whose
 * generator graph does not depend on the witness (every circuit of the recursion framework and of the table build: the
 * set of generators and the wires they read and write are fixed when the circuit is built). plonky2 walks a dependency
 * graph of the generators of mp2-common/src/serialization/circuit_data_serialization.rs:186-231 per proof; here the host
 * records them ONCE, in an order in which every value is produced before it is used, as a flat array of u64 words -- the
 * TAPE -- and the library replays it per proof, on host threads (mp2g_witness_program_run) or on the device for a whole batch
 * (mp2g_witness_program_run_dev: one block per proof, the instructions grouped by dependency level). INTEGRATION.md
 * section 6 maps every generator of the reference's registry to its opcode.
 *
 * VALUES live in SLOTS: n_slots u64 cells per proof, indexed by the tape. A slot plays the part of a plonky2 Target's
 * value; copy constraints need no instruction (two wires that are copies of each other are written from the same slot).
 * Before the tape runs, slot const_slots[2 i] holds the canonical field element const_slots[2 i + 1] and slot input_sids[j]
 * holds the proof's j-th input word; every other slot holds 0 until an instruction writes it.
 * WIRES: wire (col, row) of the 135 x 2^log_n matrix prove() commits to (standard_recursion_config: 135 wires, the first
 * 80 routed). The matrix is zero-filled per proof; an instruction writes the wires of ITS generator's gate (listed below),
 * MP2G_OP_WIRE writes a single one.
 *
 * INSTRUCTION = one opcode word followed by its operands. Operand kinds below: `row` a gate row (< 2^log_n); `i`, `col`,
 * counts: small integers as stated; `k...` a canonical field element (< p); `s...` a slot that is READ; `d...` a slot
 * that is WRITTEN; x[n] = n consecutive operand words; an extension element takes two slots (c0, c1).
 *
 * RULES. (1) Host replay executes the tape in order. (2) The device replay re-orders: an instruction's level is one more
 * than the highest level of the slots it reads (inputs and constants are level 0), and a level's instructions run
 * concurrently; it therefore needs single assignment -- no slot written twice, no slot written after an earlier
 * instruction read it. mp2g_witness_program_run_dev refuses a tape that breaks this (the host replay still accepts it).
 * (3) Two instructions must not write the same wire with different values (they may run in either order on the device).
 * (4) MP2G_OP_PAR brackets sections that neither read each other's written slots nor write the same slots or wires.
 *
 * OPCODES come in four blocks: the base set [1, MP2G_OP_END) of enum mp2g_witness_op, the GF(p^5) set [32, MP2G_OP_GF5_END)
 * of enum mp2g_witness_op_gf5, the lookup set [40, MP2G_OP_LUT_END) of enum mp2g_witness_op_lut and the wide set
 * [48, MP2G_OP_WIDE_END) of enum mp2g_witness_op_wide; every other value (0, MP2G_OP_END .. 31, MP2G_OP_GF5_END .. 39,
 * MP2G_OP_LUT_END .. 47, MP2G_OP_WIDE_END and above) is refused.
 *
 * What mp2g_witness_program_create VALIDATES (a tape that fails is refused with a message, nothing is run): every opcode
 * is known, no instruction is truncated, every row < 2^log_n, every column < 135, gate-operation indices, limb counts and
 * other counts are in the ranges given below, constants are canonical, every slot operand, input slot and constant slot is < n_slots,
 * parallel regions do not nest and their section lengths end on instruction boundaries. It does NOT check that the
 * values satisfy the circuit: that is prove()'s witness check (mp2g_prover_enable_witness_check), which fails the proof
 * the way plonky2's prove() panics on an unsatisfied witness. */
enum mp2g_witness_op {
  /* ArithmeticGate (20 operations a row) / ArithmeticBaseGenerator: out = k_c0 m0 m1 + k_c1 addend.
   * operands: row, i (< 20), k_c0, k_c1, s_m0, s_m1, s_addend, d_out.   wires 4i .. 4i+3 = m0, m1, addend, out.
   * k_c0, k_c1 must be the row's two gate constants (the caller's preprocessed constants hold them). */
  MP2G_OP_ARITH = 1,
  /* ArithmeticExtensionGate (10 operations a row) / ArithmeticExtensionGenerator, over the quadratic extension.
   * operands: row, i (< 10), k_c0, k_c1, s_m0[2], s_m1[2], s_addend[2], d_out[2].   wires 8i .. 8i+7 in that order. */
  MP2G_OP_ARITH_EXT = 2,
  /* Poseidon2Gate / Poseidon2Generator: one permutation, with the swap of the first two 4-limb chunks.
   * operands: row, s_in[12], s_swap (0 or 1), d_out[12].   wires 0..11 inputs, 12..23 outputs, 24 swap, 25..28 the swap
   * deltas, 29..64 / 65..86 / 87..134 the S-box inputs of the first full rounds 1..3, the 22 partial rounds, the last 4 full rounds. */
  MP2G_OP_P2 = 3,
  /* BaseSumGate<2> with 63 limbs / BaseSplitGenerator<2>: the bits of a value below 2^63, little endian.
   * operands: row, s_x, d_bit[63].   wire 0 = x, wires 1..63 = bits.  (other bases / limb counts: MP2G_OP_BASE_SPLIT) */
  MP2G_OP_BASE_SUM = 4,
  /* RandomAccessGate (bits = 4, 4 copies a row, 2 extra constants) / RandomAccessGenerator: out = value[index].
   * operands: row, copy (< 4), s_index (< 16), s_value[16], d_out.   wires 18 copy + 0 = index, + 1 = out, + 2..17 = values;
   * the 4 bits of the index at wires 74 + 4 copy .. (not routed).  (wires 72, 73: the row's extra constants, MP2G_OP_WIRE) */
  MP2G_OP_RA = 5,
  /* ReducingGate with 43 coefficients / ReducingGenerator: acc <- acc alpha + coeff_j for j = 0..42, base-field coefficients.
   * operands: row, s_alpha[2], s_old_acc[2], s_coeff[43], d_out[2].   wires 0,1 out; 2,3 alpha; 4,5 old acc; 6..48 coefficients;
   * 49.. the 42 intermediate accumulators. */
  MP2G_OP_REDUCING = 6,
  /* ReducingExtensionGate with 32 coefficients / ReducingExtensionGenerator: the same with extension coefficients.
   * operands: row, s_alpha[2], s_old_acc[2], s_coeff[32][2], d_out[2].   wires 0,1 out; 2,3 alpha; 4,5 old acc; 6..69 coefficients; 70.. accumulators. */
  MP2G_OP_REDUCING_EXT = 7,
  /* CosetInterpolationGate::with_max_degree(bits, 8) / InterpolationGenerator: the polynomial through 2^bits values on the coset
   * shift <w> evaluated at a point.   operands: row, bits (2..5), s_shift, s_value[2^bits][2], s_point[2], d_out[2].
   * wires 0 shift, 1.. values, then point, out, intermediate (eval, prod) pairs, shifted point (the gate's own layout). */
  MP2G_OP_COSET = 8,
  /* one wire from a slot: ConstantGenerator (ConstantGate wire j = the row's constant j), the PublicInputGate's four
   * public-inputs-hash wires, RandomAccessGate's extra constants, CopyGenerator targets that no other instruction writes.
   * operands: row, col (< 135), s_value. */
  MP2G_OP_WIRE = 9,
  /* QuotientGeneratorExtension: q = num / den in the extension (0 when den = 0: also EqualityGenerator's / NonzeroTestGenerator's
   * "inverse or zero" with num = (1, 0)).   operands: s_num[2], s_den[2], d_q[2].   no wires. */
  MP2G_OP_HINT_DIV_EXT = 10,
  /* the two halves of split_le of a full field element: d = s & (2^63 - 1) / d = s >> 63.   operands: s, d.   no wires. */
  MP2G_OP_HINT_LO63 = 11,
  MP2G_OP_HINT_HI = 12,
  /* LowHighGenerator / SplitToU32Generator (bit = 32): low = s & (2^bit - 1), high = s >> bit.
   * operands: s, bit (1..63), d_low, d_high.   no wires. */
  MP2G_OP_HINT_SPLIT = 13,
  /* a parallel region (rule 4): operands: n_sections (<= 4096), length[n_sections] in words; the sections follow back to back.
   * Host replay with fewer proofs than threads runs the sections on spare threads; the device replay ignores the marker. */
  MP2G_OP_PAR = 14,
  /* PoseidonGate / PoseidonGenerator (the original permutation, WrapC): operands and wires as MP2G_OP_P2. */
  MP2G_OP_POSEIDON = 15,
  /* U32ArithmeticGate with `ops` operations a row / U32ArithmeticGenerator: m0 m1 + addend = low + 2^32 high, all u32.
   * operands: row, i (< ops), ops (1..3), s_m0, s_m1, s_addend, d_low, d_high.   wires 6i .. 6i+5 = m0, m1, addend, low, high,
   * (2^32 - 1 - high)^-1 or 0; the 32 two-bit limbs of the 64-bit result at wires 6 ops + 32 i .. */
  MP2G_OP_U32_ARITH = 16,
  /* U32SubtractionGate / U32SubtractionGenerator: x - y - borrow_in = result - 2^32 borrow_out.
   * operands: row, i (< ops), ops (1..6), s_x, s_y, s_borrow_in, d_result, d_borrow_out.   wires 5i .. 5i+4 in that order; the 16
   * two-bit limbs of result at wires 5 ops + 16 i .. */
  MP2G_OP_U32_SUB = 17,
  /* U32AddManyGate(num_addends, ops) / U32AddManyGenerator: sum of the addends + carry_in = result + 2^32 carry_out.
   * operands: row, i (< ops), ops, n (addends, 1..16), s_addend[n], s_carry_in, d_result, d_carry_out.   wires (n + 3) i .. =
   * addends, carry_in, result, carry_out; 18 two-bit limbs (16 of result, 2 of carry_out) at wires (n + 3) ops + 18 i .. */
  MP2G_OP_U32_ADD_MANY = 18,
  /* U32RangeCheckGate(k) / U32RangeCheckGenerator: x < 2^32.   operands: row, i (< k), k (1..7), s_x.
   * wire i = x, its 16 two-bit limbs at wires k + 16 i .. ; no slot is written. */
  MP2G_OP_U32_RANGE_CHECK = 19,
  /* ComparisonGate(num_bits, num_chunks) / ComparisonGenerator: result = (first <= second), both below 2^num_bits.
   * operands: row, num_bits (1..63), num_chunks (1..16, chunks of ceil(num_bits / num_chunks) bits), s_first, s_second, d_result.
   * wires 0 first, 1 second, 2 result, 3 most significant difference, then per chunk: first chunks, second chunks, equality
   * dummies, chunks-equal flags, intermediate values, then the chunk_bits + 1 bits of 2^chunk_bits + most significant difference. */
  MP2G_OP_COMPARISON = 20,
  /* BaseSumGate<B> with n limbs, B = 2^base_bits / BaseSplitGenerator<B>: the base-B digits of x, little endian.
   * operands: row, base_bits (1 or 2), n (1..63, n base_bits <= 63), s_x, d_limb[n].   wire 0 = x, wires 1..n = limbs. */
  MP2G_OP_BASE_SPLIT = 21,
  /* MulExtensionGate (13 operations a row) / MulExtensionGenerator: out = k_c0 m0 m1 over the extension.
   * operands: row, i (< 13), k_c0, s_m0[2], s_m1[2], d_out[2].   wires 6i .. 6i+5 in that order. */
  MP2G_OP_MUL_EXT = 22,
  /* ExponentiationGate(n) / ExponentiationGenerator: out = base^(sum bit_j 2^j).
   * operands: row, n (1..66), s_base, s_bit[n] (little endian), d_out.   wire 0 base, wires 1..n bits, wire n + 1 out, wires n + 2 ..
   * the n intermediate values (most significant bit first). */
  MP2G_OP_EXP = 23,
  MP2G_OP_END = 24 /* one past the last opcode of the base set */
};
/* The Ecgfp5 base field GF(p^5) = GF(p)[z] / (z^5 - 3). An element takes 5 slots, coefficient i of z^i first (the layout of
 * plonky2_ecgfp5's QuinticExtensionTarget, of mp2g_swu_batch's inputs and of the hash output mp2g_map_to_curve_batch maps).
 * Neither opcode writes a wire: a tape puts the results on wires with MP2G_OP_WIRE. Neither fails the replay: a value that cannot
 * satisfy the circuit's constraints (no root, a zero divisor) fails that proof in prove()'s witness check, as MP2G_OP_HINT_DIV_EXT
 * does. */
enum mp2g_witness_op_gf5 {
  /* QuinticSqrtGenerator (try_any_sqrt_quintic_ext / any_sqrt_quintic_ext, mp2-common/src/group_hashing/sswu_gadget.rs).
   * x a square: root^2 = x and is_sqrt = 1, where root is THE root with sgn0(root) = 0 (the first non-zero coefficient is even;
   * x = 0 gives root = 0). x not a square: root = 0 and is_sqrt = 0. The sgn0 rule fixes the root for every replay (host,
   * device, a client's own); which root [dep] plonky2_ecgfp5's generator picks, and whether its is_sqrt flag comes from the
   * generator or from an in-circuit equality, is not pinned here -- the gadget's constraint root^2 = x holds for either root.
   * operands: s_x[5], d_root[5], d_is_sqrt. */
  MP2G_OP_QUINTIC_SQRT = 32,
  /* QuinticQuotientGenerator (div_quintic_ext / inverse_quintic_ext): q = a / b, 0 when b = 0.
   * operands: s_a[5], s_b[5], d_q[5]. */
  MP2G_OP_QUINTIC_QUOTIENT = 33,
  MP2G_OP_GF5_END = 34 /* one past the last opcode of the GF(p^5) set */
};
/* Lookups into the circuit's tables (CircuitBuilder::add_lookup_from_index). A program that holds the opcode needs its tables
 * (mp2g_witness_program_set_lookups) before it runs. */
enum mp2g_witness_op_lut {
  /* LookupGate (40 slots a row) / LookupGenerator: out = the table's output for the input; 0 when the table has no such input
   * (the pair is then in no table entry: that proof fails the lookup argument in prove(), witness-check flag 4, nothing fails in
   * the replay).   operands: row (one of the table's LookupGate rows), i (< 40), lut (table index), s_inp, d_out.
   * wires 2i, 2i+1 = input, output. */
  MP2G_OP_LOOKUP = 40,
  MP2G_OP_LUT_END = 41 /* one past the last opcode of the lookup set */
};
/* The wide block: the bit-interleaving gates of [dep] plonky2_crypto (u32/gates/interleave_u32.rs, uninterleave_to_b32.rs,
 * uninterleave_to_u32.rs: what its xor / and of u32 words are built from), the multi-limb division hints (UInt256DivGenerator,
 * mp2-common/src/u256.rs:920-952; [dep] plonky2_ecdsa BigUintDivRemGenerator) and PoseidonMdsGate's generator. Bit wires are
 * most significant first. A multi-limb integer is a run of u32 limbs, least significant first, one slot each; a limb operand is
 * read as the low 32 bits of its slot (a circuit's range checks catch a wider value). None of these instructions fails a replay:
 * a value that cannot satisfy the circuit fails that proof in prove()'s witness check, as with the hints above. */
enum mp2g_witness_op_wide {
  /* U32InterleaveGate with `ops` operations a row / U32InterleaveGenerator: x_interleaved = sum_k b_k 4^k, b_k = bit k of the low
   * 32 bits of x.   operands: row, i (< ops), ops (1..3), s_x, d_x_interleaved.   wires 2i, 2i+1 = x, x_interleaved; wire
   * 2 ops + 32 i + j = b_(31-j). */
  MP2G_OP_U32_INTERLEAVE = 48,
  /* UninterleaveToB32Gate / UninterleaveToB32Generator: evens = sum_b bit(2b) 4^b, odds = sum_b bit(2b+1) 4^b over the 64 bits of
   * x_interleaved, b = 0..31.   operands: row, i (< ops), ops (1..2), s_x_interleaved, d_evens, d_odds.   wires 3i, 3i+1, 3i+2 =
   * x_interleaved, evens, odds; wire 3 ops + 64 i + j = bit (63-j). */
  MP2G_OP_UNINTERLEAVE_TO_B32 = 49,
  /* UninterleaveToU32Gate / UninterleaveToU32Generator: as MP2G_OP_UNINTERLEAVE_TO_B32 with weights 2^b instead of 4^b (the even
   * bits and the odd bits as two u32 words: of the sum of two interleaved words, the xor and the and). */
  MP2G_OP_UNINTERLEAVE_TO_U32 = 50,
  /* UInt256DivGenerator::run_once, branch by branch. is_div != 0 and divisor != 0: (quotient, remainder) = divmod(dividend,
   * divisor). is_div != 0 and divisor = 0: (0, dividend). is_div = 0: quotient = 1 and remainder = dividend - dividend divisor
   * mod 2^256 (so that quotient' divisor + remainder = dividend holds for quotient' = dividend, as mul_div_u256 then checks).
   * operands: s_dividend[8], s_divisor[8], s_is_div, d_quotient[8], d_remainder[8].   no wires. */
  MP2G_OP_U256_DIV = 51,
  /* BigUintDivRemGenerator: (div, rem) = divmod(a, b) over na and nb limbs; b = 0 gives (0, a truncated to nb limbs) -- this
   * library's choice: [dep] plonky2_ecdsa's generator panics on a zero divisor. rem < b fits nb limbs, div <= a fits na.
   * operands: na (1..32), nb (1..32), s_a[na], s_b[nb], d_div[na], d_rem[nb].   no wires. */
  MP2G_OP_BIGUINT_DIV_REM = 52,
  /* PoseidonMdsGate / PoseidonMdsGenerator: Poseidon's MDS layer applied to 12 extension elements, component by component.
   * operands: row, s_in[12][2], d_out[12][2].   wires 2i, 2i+1 = input i; wires 24 + 2i, 24 + 2i + 1 = output i. */
  MP2G_OP_POSEIDON_MDS = 53,
  MP2G_OP_WIDE_END = 54 /* one past the last opcode of the wide set */
};
/* create: the tape is copied. input_sids [n_inputs]: the slots the caller provides per proof, in the order of the proof's input
 * words (a framework circuit: the circuit-set digest, then per verified child its verifier data, public inputs, caps, openings, FRI
 * proof words and set-membership path, then the circuit's own inputs -- recursion.py universal_inputs); const_slots [n_consts][2]:
 * (slot, value) pairs. */
typedef struct mp2g_witness_program mp2g_witness_program;
int mp2g_witness_program_create(const uint64_t* tape, size_t tape_len, uint32_t n_slots, uint32_t log_n, const uint32_t* input_sids,
                                uint32_t n_inputs, const uint64_t* const_slots, uint32_t n_consts, mp2g_witness_program** out);
uint32_t mp2g_witness_program_num_inputs(const mp2g_witness_program* p);
/* The circuit's lookup tables, for a tape with MP2G_OP_LOOKUP (tables and rows as mp2g_prover_set_lookups takes them; copied; call
 * before the first device run, which uploads them with the program's other data). After the tape, every replay (run, run_rows,
 * run_dev) then also does prove()'s set_lookup_wires -- the padding of the LookupGate rows, the LookupTableGate rows, the
 * multiplicities: see mp2g_prover_lookup_wires_dev -- so the wire matrix is complete. run_dev uses that kernel, the host replays a
 * plain C++ twin of it (bit-identical, no GPU). n_lookups of a table = the number of its MP2G_OP_LOOKUP instructions.
 * Refused: an instruction that names a table >= n_luts or a row outside that table's LookupGate rows; a table's instructions not
 * taking the slots 0 .. n_t - 1 of its rows (slot = 40 (row - last_lu_row) + i) exactly once; LookupTableGate rows that are not
 * ceil(table_len / 26); tables that share rows; a table that holds an input twice. A program with the opcode and no tables is
 * refused at run. */
int mp2g_witness_program_set_lookups(mp2g_witness_program* p, const mp2g_lookup* luts, uint32_t n_luts);
/* The same replay ON THE DEVICE, for a batch of proofs of one circuit, stream ordered on ctx's stream and without a host copy of
 * anything: one block per proof walks the program's dependency levels (csrc/witness_dev.hip). d_inputs [batch][n_inputs] and
 * d_wires [batch][135][2^log_n] (zero-filled here, then written: what mp2g_prover_prove_dev takes as d_values[0]) are device
 * pointers; d_probe_out [batch][n_probe] receives the slots registered with set_probe (the public-inputs hash and the public inputs,
 * which prove() and the parent's witness need), set once before the first device run. Bit-identical to the host replay. */
uint32_t mp2g_witness_program_num_levels(const mp2g_witness_program* p);
int mp2g_witness_program_set_probe(mp2g_witness_program* p, const uint32_t* probe_sids, uint32_t n_probe);
int mp2g_witness_program_run_dev(mp2g_witness_program* p, mp2g_ctx* ctx, const uint64_t* d_inputs, uint32_t batch, uint64_t* d_wires,
                                 uint64_t* d_probe_out);
/* inputs [batch][n_inputs] canonical field elements -> wires [batch][135][2^log_n] (host memory, the layout of
 * mp2g_prover_prove_dev's d_values[0]); `threads` host threads (0 = all), one proof per thread at a time.
 * probe_sids (may be NULL): slots whose final values are also returned, probe_out [batch][n_probe] -- the circuit's
 * public inputs and their hash, which prove() needs next to the wires. */
int mp2g_witness_program_run(const mp2g_witness_program* p, const uint64_t* inputs, uint32_t batch, uint32_t threads, uint64_t* wires,
                             const uint32_t* probe_sids, uint32_t n_probe, uint64_t* probe_out);
/* The same with one contiguous row of 135 wires per gate row: rows [batch][2^log_n][135]. This is what the host writes fastest (a
 * Poseidon2Gate row is 135 consecutive words instead of 135 cache lines: -25 % per witness); mp2g_wires_from_rows_dev turns the uploaded
 * rows into the prover's [batch][135][2^log_n] on the device. */
int mp2g_witness_program_run_rows(const mp2g_witness_program* p, const uint64_t* inputs, uint32_t batch, uint32_t threads, uint64_t* rows,
                                  const uint32_t* probe_sids, uint32_t n_probe, uint64_t* probe_out);
int mp2g_wires_from_rows_dev(mp2g_ctx* ctx, const uint64_t* d_rows, uint64_t* d_wires, uint32_t log_n, uint32_t num_wires, uint32_t batch);
void mp2g_witness_program_free(mp2g_witness_program* p);

/* ---- generate_proof for a batch of nodes of one framework circuit, on the device (csrc/chain.hip) ------------------------------
 * Replaces the bodies of CircuitWithUniversalVerifier::generate_proof (recursion-framework/src/circuit_builder.rs:286-311) and
 * WrapCircuit::wrap_proof (universal_verifier_gadget/wrap_circuit.rs:122-148): step 0 = the base circuit, steps 1.. = its wrap
 * circuits, each given as its prover (mp2g_prover with the circuit's preprocessed polynomials, gate table, permutation / quotient /
 * witness check switched on), its witness program (probe set: public-inputs hash, then the public inputs), its FRI parameters and
 * its circuit digest (device pointer, 4 words). `capacity` = the widest batch; every narrower one runs in the same buffers.
 * mp2g_chain_run: inputs [batch][n_inputs of step 0] (host) = the base circuit's witness inputs (circuit-set digest, per child the
 * verifier data, the proof, the membership proof; the circuit's own inputs); patches copy child proofs that already live on the
 * device into them in place. Per step: witness replay, prove(), gather of the next step's inputs -- all queued on the context's
 * stream, one synchronisation at the end. Outputs (host, may be NULL): the LAST step's caps [batch][4][cap words], openings
 * [batch][n_openings][2], FRI proof [batch][proof_words], public inputs [batch][n_pi]. A witness that violates a constraint makes
 * the call fail when the provers' witness check is on, as plonky2's prove() panics. */
typedef struct mp2g_chain mp2g_chain;
typedef struct { uint32_t job; uint32_t offset; uint32_t n_words; uint32_t pad_; const uint64_t* d_src; } mp2g_chain_patch;
int mp2g_chain_create(mp2g_ctx* ctx, uint32_t n_steps, mp2g_prover* const* provers, mp2g_witness_program* const* programs,
                      const mp2g_fri_params* params, const uint64_t* const* d_circuit_digests, uint32_t capacity, mp2g_chain** out);
int mp2g_chain_run(mp2g_chain* chain, const uint64_t* inputs, uint32_t batch, const mp2g_chain_patch* patches, uint32_t n_patches,
                   uint64_t* caps, uint64_t* openings, uint64_t* proof, uint64_t* public_inputs);
/* the device buffers of a step after a run (a checker downloads the wires it re-proves; any pointer may be NULL) */
int mp2g_chain_step_buffers(const mp2g_chain* chain, uint32_t step, uint64_t** d_wires, uint64_t** d_probe, uint64_t** d_caps,
                            uint64_t** d_openings, uint64_t** d_proof);
/* proof b of the last run where the chain left it: address and length (words) of its public inputs, its three proof caps, its openings
 * and its FRI proof words -- what a parent's mp2g_chain_patch entries (or a send to another rank) take; valid until the next run */
int mp2g_chain_device_proof(const mp2g_chain* chain, uint32_t b, const uint64_t* d_parts[4], uint32_t n_words[4]);
void mp2g_chain_free(mp2g_chain* chain);

/* ---- a forest of framework proofs: the native scheduler of a tree build (csrc/forest.hip) -------------------------------------
 * Replaces the harness loops that prove every node of a tree children-before-parents, one RecursiveCircuits::generate_proof per
 * node over its children's proofs (mp2-v1/tests/common/celltree.rs:54-189, rowtree.rs:78-337; recursion-framework/src/framework.rs)
 * for a host that hands whole blocks of rows to one GPU. Circuits are described once: the words of the base circuit's witness
 * inputs, how many child proofs a node takes and where each child's proof words lie in the inputs (a child's range = public inputs,
 * the three proof caps, openings, FRI words: what mp2g_chain_device_proof lists), and n_const = the remaining words (circuit-set
 * digest, the children's verifier data and membership proofs, the circuit's own inputs) in input order with the child ranges cut
 * out. chains[worker * n_circuits + circuit]: one mp2g_chain per circuit on every worker's context (NULL = this worker never gets
 * that circuit). Final proofs live in a device pool of `pool_slots` slots of `slot_words` words; a node's slot is returned when its
 * parent is proved unless the node was registered with keep != 0, or on mp2g_forest_release.
 * mp2g_forest_prove: units[u] = unit_nodes[unit_offsets[u] .. unit_offsets[u+1]) are proved by the workers in parallel, each unit
 * level by level (levels counted inside the unit), every level's nodes of one circuit in batches of the chain's capacity. The units
 * of ONE call must not depend on each other (the items of one wave of an update plan do not); children outside a unit must have
 * been proved by an earlier call or put into the pool by mp2g_forest_put_proofs (below: a stored proof as a child). A witness that
 * violates a constraint fails the call as plonky2's prove() panics. */
typedef struct mp2g_forest mp2g_forest;
typedef struct {
  uint32_t n_inputs;         /* witness inputs of the base circuit (chain step 0), in words */
  uint32_t n_children;       /* child proofs of a node, <= 4 */
  uint32_t child_offset[4];  /* word offset of each child's proof inside the inputs, increasing */
  uint32_t n_const;          /* the node's own words: everything outside the children's ranges */
} mp2g_forest_circuit;
int mp2g_forest_create(uint32_t n_workers, mp2g_ctx* const* ctxs, uint32_t n_circuits, const mp2g_forest_circuit* circuits,
                       mp2g_chain* const* chains, uint32_t slot_words, uint32_t pool_slots, mp2g_forest** out);
int mp2g_forest_add_nodes(mp2g_forest* f, uint32_t circuit, uint32_t count, const uint64_t* ids, const uint64_t* child_ids /* [count][n_children] */,
                          const uint64_t* consts /* [count][n_const] */, const uint8_t* keep /* [count] or NULL */);
/* How mp2g_forest_prove_plan cuts one wave of Ready items into units (a host that drives mp2g_forest_prove itself can use the same
 * cut): the items in order and whole, units of about group_nodes plan nodes (item i counts item_sizes[i]), at least as many units as
 * workers, shrinking towards the end of the wave (half of what is left per worker, never below group_nodes / 6) so that the last
 * units do not run beside idle workers. unit u = items [unit_first_item[u], unit_first_item[u + 1]); unit_first_item has room for
 * n_items + 1 entries. Pure host arithmetic: needs no GPU. */
int mp2g_forest_group_units(const uint32_t* item_sizes, uint32_t n_items, uint32_t n_workers, uint32_t group_nodes,
                            uint32_t* unit_first_item, uint32_t* n_units);
/* (one mp2g_forest_prove / mp2g_forest_prove_plan call at a time per forest: the call starts the forest's worker threads itself.
 * Inside it a worker keeps up to two batches queued behind the running one; a node counts as proved, and its children's pool
 * slots return, when its batch has been CONFIRMED -- witness flags read, one batch late; a failure rolls the queued batches back.
 * A worker that finds the pool empty waits for slots and fails only when every worker of the call waits. A node is PUBLISHED --
 * visible to mp2g_forest_proof and usable as a child by another unit -- only when its batch is confirmed; inside its own unit it
 * is usable as soon as it is queued (same stream). The units of one call must therefore not name each other's nodes as children
 * (the waves of an update plan never do). After a failed call the nodes of the confirmed batches stay proved: resubmit the unit
 * without them -- a unit that names a proved node is refused.) */
int mp2g_forest_prove(mp2g_forest* f, const uint64_t* unit_nodes, const uint32_t* unit_offsets /* [n_units + 1] */, uint32_t n_units);
/* the harness loop over an update plan (declared below), inside the library: drain the Ready items of a wave, group them into units of
 * about group_nodes plan nodes (never fewer units than workers), prove, mark done, until the plan is finished. A plan node k stands for
 * forest node k and its n_satellites satellite nodes ((j + 1) << satellite_shift) | k (a row and that row's cells-tree nodes).
 * waves / items_per_wave[max_waves] (may be NULL) receive the number of waves and the items of each. */
struct mp2g_update_plan;
int mp2g_forest_prove_plan(mp2g_forest* f, struct mp2g_update_plan* plan, uint32_t group_nodes, uint32_t n_satellites, uint32_t satellite_shift,
                           uint32_t* waves, uint32_t* items_per_wave, uint32_t max_waves);
/* a proved node's final proof: its words in a parent's input order (public inputs, caps of oracles 1..3, openings, FRI words) on the
 * host (words may be NULL to ask for the length) or where they lie on the device (valid until the slot is returned) */
int mp2g_forest_proof(mp2g_forest* f, uint64_t id, uint64_t* words, uint32_t* n_words);
int mp2g_forest_device_proof(mp2g_forest* f, uint64_t id, const uint64_t** d_words, uint32_t* n_words);
int mp2g_forest_release(mp2g_forest* f, uint64_t id);
/* verify published nodes of ONE circuit where they lie in the device pool (v = the verifier of that circuit's last chain step,
 * created on the forest's first context with n_public_inputs = the node's public inputs): status [n_ids], host. An id that is
 * unknown, not proved or already released fails the call before anything is verified; no status is written then. */
int mp2g_forest_verify(mp2g_forest* f, mp2g_verifier* v, const uint64_t* ids, uint32_t n_ids, uint32_t* status);
/* Stored proofs as children: what the reference's harness does for every block after the first, where it proves the touched nodes
 * of an UpdateTree only and takes each untouched sibling out of its proof store (get_proof_exact; celltree.rs:77-152,
 * rowtree.rs:78-337 over ryhope/src/lib.rs:179-222 touched()). put_proofs registers `count` EXTERNAL nodes: no circuit, no
 * children, no constant words in this forest, only a proof -- n_words[i] words at words + i * stride (host), in a parent's input
 * order, i.e. what mp2g_forest_proof hands out. Each takes one pool slot; the words go up through pinned staging in chunks of at
 * most mp2g_forest_staging_words() words on the forest's first context, one kernel per chunk scatters them into the slots and in
 * the same pass checks every word for canonicity (< p). The call synchronises: on return the nodes are PUBLISHED -- usable as
 * children by any worker, visible to mp2g_forest_proof / _proofs / _device_proof / _verify (the proof itself is NOT verified here:
 * mp2g_forest_verify with its circuit's verifier does that where it lies) -- and a node's slot returns when its parent is proved
 * unless keep[i] != 0, or on mp2g_forest_release. Refused, with nothing registered and every slot back: an id the forest knows
 * (or listed twice); n_words[i] = 0 or > slot_words; stride < n_words[i]; fewer free slots than count (the message says how many
 * are needed and how many are free); a word >= p (the message names the first such id); a call while mp2g_forest_prove runs (and
 * mp2g_forest_prove refuses to start while this call runs). A unit that lists an external node is refused like any proved node;
 * mp2g_forest_proved does not count external nodes. */
int mp2g_forest_put_proofs(mp2g_forest* f, uint32_t count, const uint64_t* ids, const uint64_t* words /* host, [count][stride] */,
                           size_t stride, const uint32_t* n_words /* [count] */, const uint8_t* keep /* [count] or NULL */);
/* mp2g_forest_proof for many published nodes at once: per chunk of at most mp2g_forest_staging_words() words one gather kernel from
 * the slots into a device staging buffer, one device-to-host copy and one synchronisation. words [n_ids][stride] (host; NULL asks
 * for the lengths only) and n_words [n_ids] receive what mp2g_forest_proof returns for each id. An id that is unknown, not proved
 * or already released -- or a proof longer than stride -- fails the call before anything is written. */
int mp2g_forest_proofs(mp2g_forest* f, const uint64_t* ids, uint32_t n_ids, uint64_t* words /* host, [n_ids][stride] */, size_t stride,
                       uint32_t* n_words /* [n_ids] */);
uint32_t mp2g_forest_staging_words(void);
uint64_t mp2g_forest_proved(const mp2g_forest* f);
uint32_t mp2g_forest_free_slots(mp2g_forest* f);
void mp2g_forest_free(mp2g_forest* f);

/* ---- work plan: the reference's only scheduler --------------------------------------
 * Host-side, no GPU involved. Replaces ryhope/src/storage/updatetree.rs: UpdateTree (:19-242, arena
 * of nodes, node 0 = root, children ordered by arena index) and UpdatePlan (:422-541). Keys are u64
 * (row / cell / block keys); a path runs root -> node. An item handed out by the plan is the unit one
 * GPU proves locally: a single node (subtree_size == 1) or a spun-off subtree whose root proof is the
 * only thing returned. */
typedef struct mp2g_update_tree mp2g_update_tree;
typedef struct mp2g_update_plan mp2g_update_plan;
/* UpdateTree::from_paths (:80-92): paths concatenated in `keys`, path i has path_lens[i] keys.
 * n_paths == 0 gives the empty tree. Fails where the reference panics: an empty path, a key that
 * occurs twice at different positions, a path whose first key is not the root. */
int mp2g_update_tree_from_paths(const uint64_t* keys, const uint32_t* path_lens, uint32_t n_paths, int64_t epoch,
                                mp2g_update_tree** out);
/* UpdateTree::from_map (:296-331): the hierarchy described by a map key -> NodeContext {left, right} (arrays of n
 * entries; has_left / has_right say whether the option is Some), walked pre-order from root. Child keys missing
 * from the map are skipped; is_path_end = NodeContext::is_leaf. A key reached twice is the reference's panic. */
int mp2g_update_tree_from_map(const uint64_t* keys, const uint64_t* left, const uint64_t* right, const uint8_t* has_left,
                              const uint8_t* has_right, uint32_t n, uint64_t root, int64_t epoch, mp2g_update_tree** out);
/* UpdateTree::extend_with_path (:145-151) */
int mp2g_update_tree_extend_with_path(mp2g_update_tree* t, const uint64_t* path, uint32_t len);
uint32_t mp2g_update_tree_size(const mp2g_update_tree* t);
int64_t mp2g_update_tree_epoch(const mp2g_update_tree* t);
int mp2g_update_tree_contains_key(const mp2g_update_tree* t, uint64_t k);
/* arena dump: keys[size], parents[size] (-1 for a root), is_path_end[size]; any pointer may be NULL */
int mp2g_update_tree_nodes(const mp2g_update_tree* t, uint64_t* keys, int32_t* parents, uint8_t* is_path_end);
/* UpdateTree::subtree_size_i (:171-179) by key */
int mp2g_update_tree_subtree_size(const mp2g_update_tree* t, uint64_t k, uint32_t* out);
void mp2g_update_tree_free(mp2g_update_tree* t);
/* into_workplan (subtree_size 1) / into_batched_workplan (:154-163); the tree is consumed (the
 * handle stays valid only for mp2g_update_tree_free, which the plan performs). */
int mp2g_update_plan_create(mp2g_update_tree* t, uint32_t subtree_size, mp2g_update_plan** out);
#define MP2G_PLAN_FINISHED 0 /* Iterator::next() == None           */
#define MP2G_PLAN_READY 1    /* Some(Next::Ready(item))            */
#define MP2G_PLAN_NOT_YET 2  /* Some(Next::NotYet)                 */
/* Iterator::next (:517-531). On READY *k is the item's key; with subtree_size == 1 the item is
 * WorkplanItem::Node and *is_path_end is set (*subtree = NULL); otherwise it is
 * WorkplanItem::Subtree and *subtree receives the spun-off tree (caller frees). Returns one of
 * the MP2G_PLAN_* states, or -1 on invalid arguments. */
int mp2g_update_plan_next(mp2g_update_plan* p, uint64_t* k, int* is_path_end, mp2g_update_tree** subtree);
/* UpdatePlan::done (:449-467); unknown key -> error (RyhopeError::KeyNotFound) */
int mp2g_update_plan_done(mp2g_update_plan* p, uint64_t k);
int mp2g_update_plan_completed(const mp2g_update_plan* p);
void mp2g_update_plan_free(mp2g_update_plan* p);

#ifdef __cplusplus
}
#endif
#endif
