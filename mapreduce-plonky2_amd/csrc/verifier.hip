// Batched proof verification on the device: plonky2 plonk/verifier.rs verify_with_challenges + fri/verifier.rs
// verify_fri_proof for `count` proofs of one circuit, stream-ordered, one synchronisation at the end (the statuses).
// Call sites in the reference: mp2-common/src/utils.rs:47-59 (verify_proof_tuple), verifiable-db/src/api.rs:448-452,
// mp2-common/src/proof.rs ProofWithVK::verify.
//
// Stages (kernel names are stable for kernel traces):
//   verifier_canon_kernel      a word >= p anywhere in a proof -> status 20, the proof takes no further part
//   verifier_pi_hash_kernel    hash_no_pad(public inputs) with the circuit's hasher (or the given hash)
//   challenger_step (fri.hip)  the transcript replayed in lock-step over the batch, read straight from the proof words
//   verifier_line_kernel       the opened constants / wires a_j + X b_j at the T base points a_j + t b_j, t < T
//   gate_constraints_points_batch_kernel (gates.hip)   the filtered gate constraints at those points: the SAME evaluators the
//                              witness check and the quotient use
//   verifier_identity_kernel   Z(1) = 1 terms, partial products, lookup terms over gl2, the gate terms interpolated in t and
//                              reduced mod t^2 - 7, alpha-reduced against Z_H(zeta) sum_i zeta^(n i) t_i(zeta): status 10 + a
//   verifier_pow_kernel        proof-of-work response (status 1) and the precomputed reduced openings
//   verifier_paths_kernel      one Merkle path per thread: count * num_queries * (n_oracles + n_layers) hashing tasks
//   verifier_fold_kernel       one query per thread: fri_combine_initial, layer consistency, compute_evaluation, final polynomial
//   verifier_status_kernel     the first failing check of the lowest failing query (a minimum over (query, check) keys)
// Why the line: every filtered constraint is a polynomial with base-field coefficients in the opened constants and wires, so
// c(a + X b) is the polynomial P(t) = c(a + t b), of degree < T, taken at t = X. gates.hip stays the only set of gate evaluators.
#include "verifier.h"
#include "fri.h"
#include "gates.h"
#include "lookup.h"
#include "poseidon.cuh"
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

using namespace mp2g;


#define V_MAX_LINE_POINTS 32
#define V_NO_FAIL 0xFFFFFFFFu

namespace {
// the four parts of the batch's proofs: public inputs | caps of oracles 1.. | openings | FRI words
struct Parts {
  const u64* p[4];
  u64 s[4];
  u32 n[4];
};
// what the kernels need of the circuit beside the layouts (layout.h), by value: the FRI scalars and the PLONK-identity numbers
struct VShape {
  u32 log_n, n_oracles, n_layers, num_queries, pow_bits;
  u32 arity_bits[8];
  u32 nc, nlp;
  u32 num_routed, degree, num_constants, num_selectors, max_j, T;
};

__device__ __forceinline__ gl2 open_at(const u64* op, u32 i) { return gl2_make(op[2 * i], op[2 * i + 1]); }
__device__ __forceinline__ bool gl2_same(gl2 x, gl2 y) { return x.a == y.a && x.b == y.b; }
__device__ __forceinline__ gl2 gl2_from(u64 a) { return gl2_make(a, 0); }

// ---- canonicity --------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) verifier_canon_kernel(Parts pt, u32* __restrict__ status) {
  const u32 b = blockIdx.y;
  bool bad = false;
  for (u32 k = 0; k < 4; k++) {
    const u64* w = pt.p[k] + b * pt.s[k];
    for (u32 i = blockIdx.x * 256 + threadIdx.x; i < pt.n[k]; i += gridDim.x * 256) bad |= w[i] >= GL_P;
  }
  if (bad) status[b] = 20;  // every writer writes the same value
}

// ---- public-inputs hash ---------------------------------------------------------------------------
template <int V>
__global__ void verifier_pi_hash_kernel(Parts pt, u32 n_pi, int given, u32 B, const u32* __restrict__ status, u64* __restrict__ pih) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  u64* out = pih + 4 * b;
  if (status[b]) { out[0] = out[1] = out[2] = out[3] = 0; return; }
  const u64* in = pt.p[0] + b * pt.s[0];
  if (given) { for (int i = 0; i < 4; i++) out[i] = in[i]; return; }
  u64 s[12];
  for (int i = 0; i < 12; i++) s[i] = 0;
  for (u32 i = 0; i < n_pi; i += 8) {
    const u32 k = n_pi - i < 8 ? n_pi - i : 8;
    for (u32 j = 0; j < k; j++) s[j] = in[i + j];
    perm<V>(s);
  }
  for (int i = 0; i < 4; i++) out[i] = s[i];
}

// ---- PLONK identity ---------------------------------------------------------------------------------
// lc [B][num_constants][T], lw [B][wires_w][T]: opening a + X b at the base points a + t b
__global__ void __launch_bounds__(256) verifier_line_kernel(VShape sh, OpeningLayout ol, Parts pt, u32 B, const u32* __restrict__ status,
                                                            u64* __restrict__ lc, u64* __restrict__ lw) {
  const u32 wires_w = ol.oracle[1].len, per = (sh.num_constants + wires_w) * sh.T;
  const u32 idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * per) return;
  const u32 b = idx / per, r = idx % per, j = r / sh.T, t = r % sh.T;
  u64 v = 0;
  if (!status[b]) {
    const u64* op = pt.p[2] + b * pt.s[2];
    const u32 o = j < sh.num_constants ? ol.constants + j : ol.oracle[1].off + (j - sh.num_constants);
    v = gl_mul_add(op[2 * o + 1], t, op[2 * o]);
  }
  if (j < sh.num_constants) lc[((u64)b * sh.num_constants + j) * sh.T + t] = v;
  else lw[((u64)b * wires_w + (j - sh.num_constants)) * sh.T + t] = v;
}

// One proof per thread: every term of the vanishing polynomial at zeta in the order of eval_vanishing_poly, accumulated into
// sum_i term_i alpha_a^i for both challenges at once (the alphas are base-field elements).
__global__ void __launch_bounds__(64) verifier_identity_kernel(VShape sh, OpeningLayout ol, LookupGeometry lu, Parts pt, u32 B,
                                                               const u64* __restrict__ bg,
                                                               const u64* __restrict__ alphas, const u64* __restrict__ zetas,
                                                               const u64* __restrict__ lut_eval, const u64* __restrict__ gate_vals,
                                                               const u64* __restrict__ interp, u32* __restrict__ status) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || status[b]) return;
  const u64* op = pt.p[2] + b * pt.s[2];
  const u32 nc = sh.nc, chunks = sh.num_routed / sh.degree, num_prods = chunks - 1;
  const u64* betas = bg + 8 * b;
  const u64* gammas = betas + nc;
  const gl2 zeta = gl2_make(zetas[2 * b], zetas[2 * b + 1]);
  gl2 zn = zeta;
  for (u32 i = 0; i < sh.log_n; i++) zn = gl2_mul(zn, zn);
  const gl2 zh = gl2_sub(zn, gl2_from(1));
  const gl2 l0 = gl2_mul(zh, gl2_inv(gl2_scale(gl2_sub(zeta, gl2_from(1)), ((u64)1 << sh.log_n) % GL_P)));
  u64 al[2] = {alphas[2 * b], nc > 1 ? alphas[2 * b + 1] : 0}, apow[2] = {1, 1};
  gl2 van[2] = {gl2_from(0), gl2_from(0)};
  auto term = [&](gl2 v) {
#pragma unroll
    for (int a = 0; a < 2; a++) {
      van[a] = gl2_add(van[a], gl2_scale(v, apow[a]));
      apow[a] = gl_mul(apow[a], al[a]);
    }
  };
  for (u32 c = 0; c < nc; c++) term(gl2_mul(l0, gl2_sub(open_at(op, ol.zs + c), gl2_from(1))));
  for (u32 c = 0; c < nc; c++) {
    u64 kj = 1;
    for (u32 ch = 0; ch < chunks; ch++) {
      gl2 num = gl2_from(1), den = gl2_from(1);
      for (u32 j = ch * sh.degree; j < (ch + 1) * sh.degree; j++) {
        const gl2 wv = open_at(op, ol.wires + j);
        num = gl2_mul(num, gl2_add(gl2_add(wv, gl2_scale(zeta, gl_mul(betas[c], kj))), gl2_from(gammas[c])));
        den = gl2_mul(den, gl2_add(gl2_add(wv, gl2_scale(open_at(op, ol.sigmas + j), betas[c])), gl2_from(gammas[c])));
        kj = gl_mul(kj, GL_MULT_GEN);
      }
      const gl2 prev = ch == 0 ? open_at(op, ol.zs + c) : open_at(op, ol.partial_products + c * num_prods + ch - 1);
      const gl2 next = ch == chunks - 1 ? open_at(op, ol.zs_next + c) : open_at(op, ol.partial_products + c * num_prods + ch);
      term(gl2_sub(gl2_mul(prev, num), gl2_mul(next, den)));
    }
  }
  if (lu.n_luts) {
    // vanishing_poly.rs check_lookup_constraints per round: sel = TransSre, TransLdc, InitSre, LastLdc, ends per table; zs[0] = RE,
    // zs[1..] the partial Sum / LDC polynomials; deltas = A, B, alpha, delta
    const u32 ns = lu.num_sldc, nlp = sh.nlp;
    auto sel = [&](u32 i) { return open_at(op, sh.num_selectors + i); };
    auto wire = [&](u32 i) { return open_at(op, ol.wires + i); };
    for (u32 c = 0; c < nc; c++) {
      const u64* d = bg + 8 * b + 4 * c;
      const u64 dA = d[0], dB = d[1], dAl = d[2], dDe = d[3];
      auto zs = [&](u32 q) { return open_at(op, ol.lookup + c * nlp + q); };
      auto zsn = [&](u32 q) { return open_at(op, ol.lookup_next + c * nlp + q); };
      auto combo = [&](u32 i, u32 stride) {  // alpha - (inp + A out)
        const gl2 x = gl2_add(wire(stride * i), gl2_scale(wire(stride * i + 1), dA));
        return gl2_make(gl_sub(dAl, x.a), gl_neg(x.b));
      };
      term(gl2_mul(sel(3), zs(ns)));
      term(gl2_mul(sel(2), zs(1)));
      term(gl2_mul(sel(2), zs(0)));
      for (u32 r = 0; r < lu.n_luts; r++)
        term(gl2_mul(sel(4 + r), gl2_sub(zs(0), gl2_from(lut_eval[((u64)b * nc + c) * MP2G_MAX_LUTS + r]))));
      gl2 cur = zsn(0);
      for (u32 s = 0; s < lu.num_lut_slots; s++)
        cur = gl2_add(gl2_scale(cur, dDe), gl2_add(wire(3 * s), gl2_scale(wire(3 * s + 1), dB)));
      term(gl2_mul(sel(0), gl2_sub(zs(0), cur)));
      for (u32 poly = 0; poly < ns; poly++) {
        u32 t0 = poly * lu.lut_degree, t1 = t0 + lu.lut_degree < lu.num_lut_slots ? t0 + lu.lut_degree : lu.num_lut_slots;
        const u32 u0 = poly * lu.lu_degree, u1 = u0 + lu.lu_degree < lu.num_lu_slots ? u0 + lu.lu_degree : lu.num_lu_slots;
        if (t0 > lu.num_lut_slots) t0 = t1 = lu.num_lut_slots;
        gl2 lut_prod = gl2_from(1), lut_sum = gl2_from(0), lu_prod = gl2_from(1), lu_sum = gl2_from(0);
        for (u32 i = t0; i < t1; i++) lut_prod = gl2_mul(lut_prod, combo(i, 3));
        for (u32 i = t0; i < t1; i++) {
          gl2 pr = gl2_from(1);
          for (u32 j = t0; j < t1; j++)
            if (j != i) pr = gl2_mul(pr, combo(j, 3));
          lut_sum = gl2_add(lut_sum, gl2_mul(wire(3 * i + 2), pr));
        }
        for (u32 i = u0; i < u1; i++) lu_prod = gl2_mul(lu_prod, combo(i, 2));
        for (u32 i = u0; i < u1; i++) {
          gl2 pr = gl2_from(1);
          for (u32 j = u0; j < u1; j++)
            if (j != i) pr = gl2_mul(pr, combo(j, 2));
          lu_sum = gl2_add(lu_sum, pr);
        }
        const gl2 prev = poly == 0 ? zsn(ns) : zs(poly);
        const gl2 diff = gl2_sub(zs(1 + poly), prev);
        term(gl2_mul(sel(0), gl2_sub(gl2_mul(lut_prod, diff), lut_sum)));  // Sum transition
        term(gl2_mul(sel(1), gl2_add(gl2_mul(lu_prod, diff), lu_sum)));    // LDC transition
      }
    }
  }
  // gate terms: P_j(t) at t = 0 .. T - 1 -> P_j(X) mod X^2 - 7, as two dot products with the interpolation rows
  const u64* gv = gate_vals + (u64)b * sh.max_j * sh.T;
  for (u32 j = 0; j < sh.max_j; j++) {
    gl_cols c0, c1;
    for (u32 t = 0; t < sh.T; t++) {
      const u64 v = gv[j * sh.T + t];
      c0.add(v, interp[t]);
      c1.add(v, interp[V_MAX_LINE_POINTS + t]);
    }
    term(gl2_make(c0.value(), c1.value()));
  }
  for (u32 a = 0; a < nc; a++) {
    gl2 tz = gl2_from(0);
    for (u32 i = 8; i-- > 0;) tz = gl2_add(gl2_mul(tz, zn), open_at(op, ol.quotient + a * 8 + i));
    if (!gl2_same(van[a], gl2_mul(zh, tz))) { status[b] = 10 + a; return; }
  }
}

// ---- proof of work, reduced openings ---------------------------------------------------------------
__global__ void __launch_bounds__(64) verifier_pow_kernel(VShape sh, OpeningLayout ol, Parts pt, u32 B, const u64* __restrict__ pow_resp,
                                                          const u64* __restrict__ fri_alpha, u32* __restrict__ status,
                                                          u64* __restrict__ red) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || status[b]) return;
  if (sh.pow_bits && (pow_resp[b] >> (64 - sh.pow_bits)) != 0) { status[b] = 1; return; }
  const u64* op = pt.p[2] + b * pt.s[2];
  const gl2 alpha = gl2_make(fri_alpha[2 * b], fri_alpha[2 * b + 1]);
  gl2 acc = gl2_from(0);
  for (u32 i = ol.n_zeta; i-- > 0;) acc = gl2_add(gl2_mul(acc, alpha), open_at(op, i));
  red[4 * b] = acc.a; red[4 * b + 1] = acc.b;
  acc = gl2_from(0);
  for (u32 i = ol.n_open; i-- > ol.n_zeta;) acc = gl2_add(gl2_mul(acc, alpha), open_at(op, i));
  red[4 * b + 2] = acc.a; red[4 * b + 3] = acc.b;
}

// ---- queries -----------------------------------------------------------------------------------------
// failure key of a query's check: (query, position of the check in the verifier's order, code); the minimum is the first failing
// check of the lowest failing query. positions: 0 initial paths; 1 + 2 li consistency of layer li; 2 + 2 li its path; then the final
// polynomial
__device__ __forceinline__ void query_fail(u32* qstat, u32 b, u32 q, u32 pos, u32 code) { atomicMin(&qstat[b], (q << 16) | (pos << 8) | code); }

// One Merkle path per thread (merkle_proofs.rs verify_merkle_proof_to_cap; the leaf through hash_or_noop). Threads are ordered path-
// kind major so that a wave's lanes hash leaves of one width and climb paths of one length.
template <int V>
__global__ void __launch_bounds__(256) verifier_paths_kernel(FriProofLayout L, VShape sh, Parts pt, u32 B, const u64* __restrict__ cap0,
                                                             const u64* __restrict__ qchal, const u32* __restrict__ status,
                                                             u32* __restrict__ qstat) {
  const u32 idx = blockIdx.x * 256 + threadIdx.x, per = B * sh.num_queries;
  if (idx >= per * L.n_paths) return;
  const u32 p = idx / per, r = idx % per, b = r / sh.num_queries, q = r % sh.num_queries;
  if (status[b]) return;
  const u64* proof = pt.p[3] + b * pt.s[3];
  const u64* leaf = proof + L.q_off + (u64)q * L.q_words + L.leaf_off[p];
  const u32 len = L.leaf_len[p];
  const u64* sib = leaf + len;
  u32 x = (u32)(qchal[(u64)b * sh.num_queries + q] & (((u64)1 << L.lg) - 1)) >> L.x_shift[p];
  const u64* cap = p == 0 ? cap0 : p < sh.n_oracles ? pt.p[1] + b * pt.s[1] + (u64)(p - 1) * L.capw : proof + (u64)(p - sh.n_oracles) * L.capw;
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = 0;
  if (len <= 4) {
    for (u32 i = 0; i < len; i++) s[i] = leaf[i];
  } else {
    for (u32 i = 0; i < len; i += 8) {
      const u32 k = len - i < 8 ? len - i : 8;
      if (k == 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = leaf[i + j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
          if ((u32)j < k) s[j] = leaf[i + j];
      }
      perm<V>(s);
    }
  }
  for (u32 i = 0; i < L.n_sib[p]; i++) {
    const u64* sb = sib + 4 * i;
    const bool right = x & 1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u64 c = s[j], o = sb[j];
      s[j] = right ? o : c;
      s[4 + j] = right ? c : o;
      s[8 + j] = 0;
    }
    perm<V>(s);
    x >>= 1;
  }
  const u64* want = cap + 4 * x;
  if (s[0] != want[0] || s[1] != want[1] || s[2] != want[2] || s[3] != want[3]) {
    if (p < sh.n_oracles) query_fail(qstat, b, q, 0, 2);
    else query_fail(qstat, b, q, 2 + 2 * (p - sh.n_oracles), 4);
  }
}

// One query per thread: the field arithmetic of fri_verifier_query_round (no hashing here)
__global__ void __launch_bounds__(64) verifier_fold_kernel(VShape sh, FriShape fs, FriProofLayout L, Parts pt, u32 B, const u64* __restrict__ qchal,
                                                           const u64* __restrict__ zetas, const u64* __restrict__ fri_alpha,
                                                           const u64* __restrict__ fri_betas, const u64* __restrict__ red,
                                                           const u32* __restrict__ status, u32* __restrict__ qstat) {
  const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * sh.num_queries) return;
  const u32 b = idx / sh.num_queries, q = idx % sh.num_queries;
  if (status[b]) return;
  const u64* proof = pt.p[3] + b * pt.s[3];
  const u64* qw = proof + L.q_off + (u64)q * L.q_words;
  const u32 lg = fs.log_n + fs.rate_bits;
  u32 x = (u32)(qchal[(u64)b * sh.num_queries + q] & (((u64)1 << lg) - 1));
  const gl2 alpha = gl2_make(fri_alpha[2 * b], fri_alpha[2 * b + 1]);
  const gl2 zeta = gl2_make(zetas[2 * b], zetas[2 * b + 1]);
  const gl2 g_zeta = gl2_scale(zeta, gl_root_of_unity(fs.log_n));
  u64 sx = gl_mul(GL_MULT_GEN, gl_pow(gl_root_of_unity(lg), bitrev32(x, lg)));
  // fri_combine_initial
  gl2 sum = gl2_from(0);
  for (u32 batch = 0; batch < 2; batch++) {
    const u32 count = fri_batch_len(fs, batch);
    gl2 acc = gl2_from(0);
    for (u32 j = count; j-- > 0;) {
      u32 o, p;
      fri_batch_poly(fs, batch, j, o, p);
      acc = gl2_mul(acc, alpha);
      acc.a = gl_add(acc.a, qw[L.leaf_off[o] + p]);
    }
    const gl2 num = gl2_sub(acc, gl2_make(red[4 * b + 2 * batch], red[4 * b + 2 * batch + 1]));
    const gl2 den = gl2_sub(gl2_from(sx), batch == 0 ? zeta : g_zeta);
    sum = gl2_mul(sum, gl2_pow(alpha, count));
    sum = gl2_add(sum, gl2_mul(num, gl2_inv(den)));
  }
  gl2 old_eval = sum;
  for (u32 li = 0; li < sh.n_layers; li++) {
    const u32 ab = sh.arity_bits[li], arity = 1u << ab;
    const u32 coset = x >> ab, within = x & (arity - 1);
    const u64* ev = qw + L.leaf_off[fs.n_oracles + li];
    if (ev[2 * within] != old_eval.a || ev[2 * within + 1] != old_eval.b) query_fail(qstat, b, q, 1 + 2 * li, 3);
    // compute_evaluation: the polynomial through (start g^i, ev[bitrev(i)]) at beta. The points are the roots of X^arity - S,
    // S = start^arity, so prod_{j != i} (x_i - x_j) = arity x_i^(arity - 1) = arity S / x_i: one inversion per layer.
    const gl2 beta = gl2_make(fri_betas[16 * b + 2 * li], fri_betas[16 * b + 2 * li + 1]);
    const u64 g = gl_root_of_unity(ab);
    const u64 start = gl_mul(sx, gl_pow(g, arity - bitrev32(within, ab)));
    u64 S = start;
    for (u32 i = 0; i < ab; i++) S = gl_sqr(S);
    const u64 inv_as = gl_inv(gl_mul(S, arity));
    gl2 res = gl2_from(0);
    u64 xi = start;
    for (u32 i = 0; i < arity; i++) {
      const u32 src = bitrev32(i, ab);
      gl2 numr = gl2_from(1);
      u64 xj = start;
      for (u32 j = 0; j < arity; j++) {
        if (j != i) numr = gl2_mul(numr, gl2_make(gl_sub(beta.a, xj), beta.b));
        xj = gl_mul(xj, g);
      }
      res = gl2_add(res, gl2_mul(gl2_make(ev[2 * src], ev[2 * src + 1]), gl2_scale(numr, gl_mul(xi, inv_as))));
      xi = gl_mul(xi, g);
    }
    old_eval = res;
    for (u32 i = 0; i < ab; i++) sx = gl_sqr(sx);
    x = coset;
  }
  const u64* fin = proof + L.final_off;
  gl2 fe = gl2_from(0);
  for (u32 i = L.final_len; i-- > 0;) fe = gl2_add(gl2_scale(fe, sx), gl2_make(fin[2 * i], fin[2 * i + 1]));
  if (!gl2_same(fe, old_eval)) query_fail(qstat, b, q, 1 + 2 * sh.n_layers, 5);
}

__global__ void verifier_status_kernel(u32 B, const u32* __restrict__ qstat, u32* __restrict__ status) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (!status[b] && qstat[b] != V_NO_FAIL) status[b] = qstat[b] & 0xFF;
}

// out[b] = betas[2], gammas[2], alphas[2], zeta[2], lookup challenges[8], FRI alpha[2], FRI betas[n_layers][2], PoW response, indices
__global__ void verifier_challenges_kernel(VShape sh, u32 lg, u32 has_lookup, u32 B, const u64* bg, const u64* alphas, const u64* zetas, const u64* fri_alpha,
                                           const u64* fri_betas, const u64* pow_resp, const u64* qchal, u64* out, u32 wpp) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  u64* o = out + (u64)b * wpp;
  for (u32 i = 0; i < 2; i++) {
    o[i] = i < sh.nc ? bg[8 * b + i] : 0;
    o[2 + i] = i < sh.nc ? bg[8 * b + sh.nc + i] : 0;
    o[4 + i] = i < sh.nc ? alphas[2 * b + i] : 0;
    o[6 + i] = zetas[2 * b + i];
    o[16 + i] = fri_alpha[2 * b + i];
  }
  for (u32 i = 0; i < 8; i++) o[8 + i] = has_lookup && i < 4 * sh.nc ? bg[8 * b + i] : 0;
  for (u32 i = 0; i < 2 * sh.n_layers; i++) o[18 + i] = fri_betas[16 * b + i];
  o[18 + 2 * sh.n_layers] = pow_resp[b];
  for (u32 i = 0; i < sh.num_queries; i++) o[19 + 2 * sh.n_layers + i] = qchal[(u64)b * sh.num_queries + i] & (((u64)1 << lg) - 1);
}

// rows of the map "values of P at t = 0 .. T - 1" -> P(X) mod X^2 - 7: out[t] and out[V_MAX_LINE_POINTS + t]
void interpolation_rows(u32 T, u64* out) {
  std::vector<u64> basis(T), next(T);
  for (u32 t = 0; t < T; t++) {
    // L_t = prod_{s != t} (X - s) / (t - s)
    std::fill(basis.begin(), basis.end(), 0);
    basis[0] = 1;
    u64 den = 1;
    u32 deg = 0;
    for (u32 s = 0; s < T; s++) {
      if (s == t) continue;
      std::fill(next.begin(), next.end(), 0);
      for (u32 k = 0; k <= deg; k++) {
        next[k + 1] = gl_add(next[k + 1], basis[k]);
        next[k] = gl_sub(next[k], gl_mul(basis[k], s));
      }
      basis.swap(next);
      deg++;
      den = gl_mul(den, gl_sub(t, s));
    }
    const u64 di = gl_inv(den);
    u64 r0 = 0, r1 = 0, p7 = 1;
    for (u32 k = 0; k < T; k++) {
      const u64 c = gl_mul(gl_mul(basis[k], di), p7);
      if (k & 1) { r1 = gl_add(r1, c); p7 = gl_mul(p7, 7); } else r0 = gl_add(r0, c);
    }
    out[t] = r0;
    out[V_MAX_LINE_POINTS + t] = r1;
  }
}
}  // namespace

struct mp2g_verifier {
  mp2g_ctx* ctx = nullptr;
  mp2g_fri_params P{};
  uint32_t capacity = 0, n_pi = 0, last_count = 0, wpp = 0;
  bool pi_given = false;
  ProofParts parts{};  // a proof as the verifier takes it: the part lengths, and the offsets in a contiguous proof
  FriProofLayout fl{};
  OpeningLayout ol{};
  VShape sh{};
  FriShape fs{};
  GateTable gates{};
  LookupDev lookups{};
  DevBuf lut_tables, lut_eval;
  DevBuf cap0, digest, interp;
  DevBuf ch, pih, chal, bg, alphas, zeta, fri_alpha, fri_betas, pow_resp, qchal, red;
  DevBuf lc, lw, gate_vals;
  DevBuf status, qstat, staging, chal_out;
};

namespace mp2g {
mp2g_ctx* verifier_ctx(const mp2g_verifier* v) { return v ? v->ctx : nullptr; }
uint32_t verifier_capacity(const mp2g_verifier* v) { return v ? v->capacity : 0; }
}  // namespace mp2g

// `count` contiguous proofs at d_words (device)
static Parts contiguous_parts(const mp2g_verifier* v, const u64* d_words) {
  Parts pt{};
  for (int k = 0; k < 4; k++) { pt.p[k] = d_words + v->parts.off[k]; pt.s[k] = v->parts.words; pt.n[k] = v->parts.n[k]; }
  return pt;
}

static int verify_parts(mp2g_verifier* v, const Parts& pt, uint32_t B, uint32_t* status) {
  mp2g_ctx* c = v->ctx;
  hipStream_t s = c->stream;
  const mp2g_fri_params& P = v->P;
  const VShape& sh = v->sh;
  const FriProofLayout& L = v->fl;
  const bool has_lookup = v->lookups.n_luts != 0;
  const int V = (int)P.variant;
  ChState* st = (ChState*)v->ch.p;
  u32* d_status = (u32*)v->status.p;
  u32* d_qstat = (u32*)v->qstat.p;
  u64* chal = v->chal.p;
  const u32 nch = sh.nc, capw = L.capw;
  v->last_count = 0;
  CK(hipMemsetAsync(d_status, 0, B * sizeof(u32), s));
  CK(hipMemsetAsync(d_qstat, 0xFF, B * sizeof(u32), s));
  hipLaunchKernelGGL(verifier_canon_kernel, dim3(16, B), dim3(256), 0, s, pt, d_status);
  if (V == MP2G_POSEIDON2)
    hipLaunchKernelGGL((verifier_pi_hash_kernel<MP2G_POSEIDON2>), dim3((B + 63) / 64), dim3(64), 0, s, pt, v->n_pi, (int)v->pi_given, B, d_status, v->pih.p);
  else
    hipLaunchKernelGGL((verifier_pi_hash_kernel<MP2G_POSEIDON>), dim3((B + 63) / 64), dim3(64), 0, s, pt, v->n_pi, (int)v->pi_given, B, d_status, v->pih.p);
  CK(hipGetLastError());
  // transcript: plonk/get_challenges.rs get_challenges + fri_challenges
  CK(challenger_init(s, st, B));
  CK(challenger_step(s, V, st, B, v->digest.p, 0, 4, chal, 8, 0));
  CK(challenger_step(s, V, st, B, v->pih.p, 4, 4, chal, 8, 0));
  for (u32 o = 1; o < P.n_oracles; o++) {
    u64* dst = o == 1 ? v->bg.p : o == 2 ? v->alphas.p : chal;
    const u64 dst_stride = o == 2 ? 2 : 8;
    CK(challenger_step(s, V, st, B, pt.p[1] + (u64)(o - 1) * capw, pt.s[1], capw, dst, dst_stride, plonk_challenges_after_cap(o, nch, has_lookup)));
  }
  CK(challenger_step(s, V, st, B, chal, 0, 0, v->zeta.p, 2, 2));
  CK(challenger_step(s, V, st, B, pt.p[2], pt.s[2], pt.n[2], chal, 8, 0));
  CK(challenger_step(s, V, st, B, chal, 0, 0, v->fri_alpha.p, 2, 2));
  for (u32 li = 0; li < P.n_layers; li++)
    CK(challenger_step(s, V, st, B, pt.p[3] + (u64)li * capw, pt.s[3], capw, v->fri_betas.p + 2 * li, 16, 2));
  CK(challenger_step(s, V, st, B, pt.p[3] + L.final_off, pt.s[3], 2 * L.final_len, chal, 8, 0));
  CK(challenger_step(s, V, st, B, pt.p[3] + L.pow_off, pt.s[3], 1, v->pow_resp.p, 1, 1));
  if (P.num_queries) CK(challenger_step(s, V, st, B, chal, 0, 0, v->qchal.p, P.num_queries, P.num_queries));
  // PLONK identity at zeta
  if (has_lookup) CK(lookup_table_polys(s, B, v->lookups, v->bg.p, 8, nch, v->lut_eval.p));
  if (sh.max_j) {
    const u32 total = B * (sh.num_constants + P.oracle_w[1]) * sh.T;
    hipLaunchKernelGGL(verifier_line_kernel, dim3((total + 255) / 256), dim3(256), 0, s, sh, v->ol, pt, B, d_status, v->lc.p, v->lw.p);
    CK(hipGetLastError());
    CK(gate_constraints_points_batch(s, B, v->gates, v->lc.p, (u64)sh.num_constants * sh.T, v->lw.p, (u64)P.oracle_w[1] * sh.T, sh.T,
                                     sh.max_j, v->pih.p, v->gate_vals.p));
  }
  hipLaunchKernelGGL(verifier_identity_kernel, dim3((B + 63) / 64), dim3(64), 0, s, sh, v->ol, (LookupGeometry)v->lookups, pt, B, v->bg.p, v->alphas.p,
                     v->zeta.p, v->lut_eval.p, v->gate_vals.p, v->interp.p, d_status);
  hipLaunchKernelGGL(verifier_pow_kernel, dim3((B + 63) / 64), dim3(64), 0, s, sh, v->ol, pt, B, v->pow_resp.p, v->fri_alpha.p, d_status, v->red.p);
  CK(hipGetLastError());
  if (P.num_queries) {
    const u32 n_tasks = B * P.num_queries * L.n_paths;
    if (V == MP2G_POSEIDON2)
      hipLaunchKernelGGL((verifier_paths_kernel<MP2G_POSEIDON2>), dim3((n_tasks + 255) / 256), dim3(256), 0, s, L, sh, pt, B, v->cap0.p, v->qchal.p, d_status, d_qstat);
    else
      hipLaunchKernelGGL((verifier_paths_kernel<MP2G_POSEIDON>), dim3((n_tasks + 255) / 256), dim3(256), 0, s, L, sh, pt, B, v->cap0.p, v->qchal.p, d_status, d_qstat);
    hipLaunchKernelGGL(verifier_fold_kernel, dim3((B * P.num_queries + 63) / 64), dim3(64), 0, s, sh, v->fs, L, pt, B, v->qchal.p, v->zeta.p,
                       v->fri_alpha.p, v->fri_betas.p, v->red.p, d_status, d_qstat);
    hipLaunchKernelGGL(verifier_status_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, d_qstat, d_status);
    CK(hipGetLastError());
  }
  CK(hipMemcpyAsync(status, d_status, B * sizeof(u32), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  v->last_count = B;
  return 0;
}

namespace mp2g {
int verifier_verify_gathered(mp2g_verifier* v, const u64* const* d_srcs, uint32_t count, uint32_t* status) {
  NEED(v && d_srcs && status, "verifier / sources / status");
  NEED(count >= 1 && count <= v->capacity, "1 <= count <= the verifier's capacity");
  if (!v->staging.p) CK(v->staging.alloc((size_t)v->capacity * v->parts.words * sizeof(u64)));
  for (uint32_t i = 0; i < count; i++)
    CK(hipMemcpyAsync(v->staging.p + (size_t)i * v->parts.words, d_srcs[i], v->parts.words * sizeof(u64), hipMemcpyDeviceToDevice, v->ctx->stream));
  return verify_parts(v, contiguous_parts(v, v->staging.p), count, status);
}
}  // namespace mp2g

extern "C" {

uint32_t mp2g_gate_table_line_points(const mp2g_gate* gates, uint32_t n_gates, uint32_t num_selectors) {
  if (!gates && n_gates) return 0;
  uint64_t deg = 0;
  for (uint32_t i = 0; i < n_gates; i++) {
    const mp2g_gate& g = gates[i];
    if (gate_shape(g).err || g.group_end <= g.group_start) return 0;
    deg = std::max(deg, gate_filtered_degree(g, num_selectors));
  }
  return deg < 0xFFFFFFFFull ? (uint32_t)deg + 1 : 0;
}

int mp2g_verifier_create(mp2g_ctx* c, const mp2g_fri_params* params, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                         uint32_t num_routed, uint32_t degree, const mp2g_gate* gates, uint32_t n_gates, uint32_t num_selectors,
                         const mp2g_lookup* luts, uint32_t n_luts, uint32_t n_public_inputs, uint32_t capacity, mp2g_verifier** out) {
  NEED(c && params && constants_sigmas_cap && circuit_digest && out, "ctx / params / cap / digest / out");
  if (params_check(params)) return 1;
  const mp2g_fri_params& P = *params;
  NEED(capacity >= 1 && capacity <= (1u << 20), "1 <= capacity <= 2^20");
  NEED(P.n_oracles == 4 && P.zs_oracle == 2, "plonky2's four oracles (constants_sigmas, wires, zs_partial_products, quotient)");
  NEED(P.zs_count >= 1 && P.zs_count <= 2, "1 or 2 challenge rounds");
  NEED(P.log_n + P.rate_bits <= 31, "log_n + rate_bits <= 31");
  NEED(P.n_oracles + P.n_layers <= MP2G_MAX_PATHS, "n_oracles + n_layers");
  NEED(degree >= 2 && num_routed >= degree && num_routed % degree == 0 && num_routed <= 256, "num_routed / degree");
  NEED(P.oracle_w[0] > num_routed && P.oracle_w[1] >= num_routed, "oracle widths against num_routed");
  NEED(P.oracle_w[2] == P.zs_count * (num_routed / degree + P.num_lookup_polys), "oracle_w[2] = rounds * (num_routed / degree + num_lookup_polys)");
  NEED(P.oracle_w[3] == P.zs_count * 8, "oracle_w[3] = rounds * 8 quotient chunks");
  NEED(n_gates <= MP2G_MAX_GATES && (gates || !n_gates), "gate table");
  NEED(n_luts <= MP2G_MAX_LUTS && (luts || !n_luts), "lookup tables");
  NEED((n_luts != 0) == (P.num_lookup_polys != 0), "lookup tables and params.num_lookup_polys go together");
  NEED(n_public_inputs == MP2G_PI_HASH_GIVEN || n_public_inputs <= (1u << 16), "n_public_inputs");
  const uint32_t num_constants = P.oracle_w[0] - num_routed;
  mp2g_verifier* v = new (std::nothrow) mp2g_verifier();
  if (!v) return fail("out of memory");
  struct Guard { mp2g_verifier* v; ~Guard() { delete v; } } guard{v};
  v->ctx = c; v->P = P; v->capacity = capacity;
  v->pi_given = n_public_inputs == MP2G_PI_HASH_GIVEN;
  v->n_pi = v->pi_given ? 4 : n_public_inputs;
  VShape& sh = v->sh;
  const char* msg = gate_table_make(gates, n_gates, num_selectors, n_luts ? 4 + n_luts : 0, num_constants, P.oracle_w[1], v->gates, &sh.max_j);
  if (msg) return fail("invalid gate table: %s", msg);
  if (n_gates) {
    sh.T = mp2g_gate_table_line_points(gates, n_gates, num_selectors);
    NEED(sh.T >= 1 && sh.T <= V_MAX_LINE_POINTS, "the filtered constraints need more than 32 line points");
  }
  sh.log_n = P.log_n; sh.n_oracles = P.n_oracles; sh.n_layers = P.n_layers; sh.num_queries = P.num_queries; sh.pow_bits = P.pow_bits;
  for (int i = 0; i < 8; i++) sh.arity_bits[i] = P.arity_bits[i];
  sh.nc = P.zs_count; sh.nlp = P.num_lookup_polys;
  sh.num_routed = num_routed; sh.degree = degree; sh.num_constants = num_constants; sh.num_selectors = num_selectors;
  NEED(num_selectors + v->gates.num_lookup_selectors <= num_constants, "the constants must hold the selectors and the lookup selectors");
  v->fl = fri_proof_layout(P);
  NEED(v->fl.proof_words <= 0xFFFFFFFFull, "the FRI proof must be shorter than 2^32 words");
  v->ol = opening_layout(P, num_constants);
  v->fs = fri_shape(P);
  v->parts = proof_parts(P, v->n_pi);
  v->wpp = 19 + 2 * P.n_layers + P.num_queries;
  hipStream_t s = c->stream;
  if (n_luts) {
    LookupDev& L = v->lookups;
    lookup_geometry(num_routed, degree, L);
    NEED(L.num_lut_slots >= 1, "lookup slot geometry");
    NEED(P.num_lookup_polys == L.num_sldc + 1, "params.num_lookup_polys must be ceil((num_routed/2) / (degree-1)) + 1");
    NEED(P.oracle_w[1] >= 3 * L.num_lut_slots && P.oracle_w[1] >= 2 * L.num_lu_slots, "wires against the lookup slots");
    for (uint32_t r = 0; r < n_luts; r++)
      NEED(luts[r].table && luts[r].table_len >= 1 && luts[r].table_len <= 65536, "lookup table");
    { int rc = lookup_upload(s, luts, n_luts, v->lut_tables, L); if (rc) return rc; }
    CK(v->lut_eval.alloc((size_t)capacity * P.zs_count * MP2G_MAX_LUTS * sizeof(u64)));
  } else {
    CK(v->lut_eval.alloc(8));
  }
  std::vector<u64> rows(2 * V_MAX_LINE_POINTS, 0);
  if (sh.T) interpolation_rows(sh.T, rows.data());
  CK(v->interp.alloc(rows.size() * sizeof(u64)));
  CK(hipMemcpyAsync(v->interp.p, rows.data(), rows.size() * sizeof(u64), hipMemcpyHostToDevice, s));
  CK(v->cap0.alloc(v->fl.capw * sizeof(u64)));
  CK(hipMemcpyAsync(v->cap0.p, constants_sigmas_cap, v->fl.capw * sizeof(u64), hipMemcpyHostToDevice, s));
  CK(v->digest.alloc(4 * sizeof(u64)));
  CK(hipMemcpyAsync(v->digest.p, circuit_digest, 4 * sizeof(u64), hipMemcpyHostToDevice, s));
  CK(hipStreamSynchronize(s));  // the caller's memory may go away
  const size_t B = capacity;
  CK(v->ch.alloc(B * sizeof(ChState)));
  CK(v->pih.alloc(B * 4 * sizeof(u64)));
  CK(v->chal.alloc(B * 8 * sizeof(u64)));
  CK(v->bg.alloc(B * 8 * sizeof(u64)));
  CK(v->alphas.alloc(B * 2 * sizeof(u64)));
  CK(v->zeta.alloc(B * 2 * sizeof(u64)));
  CK(v->fri_alpha.alloc(B * 2 * sizeof(u64)));
  CK(v->fri_betas.alloc(B * 16 * sizeof(u64)));
  CK(v->pow_resp.alloc(B * sizeof(u64)));
  CK(v->qchal.alloc(B * std::max(1u, P.num_queries) * sizeof(u64)));
  CK(v->red.alloc(B * 4 * sizeof(u64)));
  CK(v->lc.alloc(B * num_constants * std::max(1u, sh.T) * sizeof(u64)));
  CK(v->lw.alloc(B * P.oracle_w[1] * std::max(1u, sh.T) * sizeof(u64)));
  CK(v->gate_vals.alloc(B * std::max(1u, sh.max_j * sh.T) * sizeof(u64)));
  CK(v->status.alloc(B * sizeof(u32)));
  CK(v->qstat.alloc(B * sizeof(u32)));
  CK(hipMemsetAsync(v->bg.p, 0, B * 8 * sizeof(u64), s));
  CK(hipMemsetAsync(v->alphas.p, 0, B * 2 * sizeof(u64), s));
  CK(hipMemsetAsync(v->fri_betas.p, 0, B * 16 * sizeof(u64), s));
  guard.v = nullptr;
  *out = v;
  return 0;
}

size_t mp2g_verifier_proof_words(const mp2g_verifier* v, uint32_t part_words[4]) {
  if (!v) return 0;
  if (part_words) for (int k = 0; k < 4; k++) part_words[k] = v->parts.n[k];
  return v->parts.words;
}

int mp2g_verifier_verify_dev(mp2g_verifier* v, const uint64_t* const d_parts[4], const uint64_t strides[4], uint32_t count, uint32_t* status) {
  NEED(v && d_parts && strides && status, "verifier / parts / strides / status");
  NEED(count >= 1 && count <= v->capacity, "1 <= count <= the verifier's capacity");
  Parts pt{};
  for (int k = 0; k < 4; k++) {
    pt.n[k] = v->parts.n[k];
    NEED(d_parts[k] || !pt.n[k], "a part is missing");
    NEED(count == 1 || strides[k] >= pt.n[k], "a stride is shorter than its part");
    pt.p[k] = d_parts[k] ? d_parts[k] : v->chal.p;
    pt.s[k] = strides[k];
  }
  return verify_parts(v, pt, count, status);
}

int mp2g_verifier_verify(mp2g_verifier* v, const uint64_t* words, uint32_t count, uint32_t* status) {
  NEED(v && words && status, "verifier / words / status");
  NEED(count >= 1 && count <= v->capacity, "1 <= count <= the verifier's capacity");
  if (!v->staging.p) CK(v->staging.alloc((size_t)v->capacity * v->parts.words * sizeof(u64)));
  CK(hipMemcpyAsync(v->staging.p, words, (size_t)count * v->parts.words * sizeof(u64), hipMemcpyHostToDevice, v->ctx->stream));
  return verify_parts(v, contiguous_parts(v, v->staging.p), count, status);
}

int mp2g_verifier_challenges(mp2g_verifier* v, uint64_t* out, size_t* words_per_proof) {
  NEED(v && words_per_proof, "verifier / words_per_proof");
  *words_per_proof = v->wpp;
  if (!out) return 0;
  NEED(v->last_count, "no completed verify call to report the challenges of");
  const u32 B = v->last_count;
  hipStream_t s = v->ctx->stream;
  if (!v->chal_out.p) CK(v->chal_out.alloc((size_t)v->capacity * v->wpp * sizeof(u64)));
  hipLaunchKernelGGL(verifier_challenges_kernel, dim3((B + 63) / 64), dim3(64), 0, s, v->sh, v->fl.lg, v->lookups.n_luts != 0, B, v->bg.p, v->alphas.p, v->zeta.p, v->fri_alpha.p,
                     v->fri_betas.p, v->pow_resp.p, v->qchal.p, v->chal_out.p, v->wpp);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, v->chal_out.p, (size_t)B * v->wpp * sizeof(u64), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return 0;
}

void mp2g_verifier_free(mp2g_verifier* v) {
  if (!v) return;
  (void)hipStreamSynchronize(v->ctx->stream);
  delete v;
}

}  // extern "C"
