// Ecgfp5 points for gfx950 device code: the group law, decode / encode, scalar multiplication and simple_swu / map_to_curve,
// shared by the multiset-digest kernels (ecgfp5.hip) and the SWU entry (ec_swu.hip). See ecgfp5.hip for what they replace.
#pragma once
#include "poseidon.cuh"
#include "gl5.cuh"

namespace mp2g {

// large bodies are real functions: the SWU / scalar-mul kernels call them hundreds of times
#define GLN __device__ __noinline__

// ---- group ------------------------------------------------------------------------------------
struct pt { gl5 X, Z, U, T; };
#define EC_B1 263u
GLD pt pt_neutral() { pt p; p.X = gl5_zero(); p.Z = gl5_from(1); p.U = gl5_zero(); p.T = gl5_from(1); return p; }
GLN pt pt_add(const pt& p, const pt& q) {
  gl5 t1 = gl5_mul(p.X, q.X), t2 = gl5_mul(p.Z, q.Z), t3 = gl5_mul(p.U, q.U), t4 = gl5_mul(p.T, q.T);
  gl5 t5 = gl5_sub(gl5_sub(gl5_mul(gl5_add(p.X, p.Z), gl5_add(q.X, q.Z)), t1), t2);
  gl5 t6 = gl5_sub(gl5_sub(gl5_mul(gl5_add(p.U, p.T), gl5_add(q.U, q.T)), t3), t4);
  gl5 t7 = gl5_add(t1, gl5_mul_kz(t2, EC_B1));
  gl5 t8 = gl5_mul(t4, t7);
  gl5 t9 = gl5_mul(t3, gl5_add(gl5_mul_kz(t5, 2 * EC_B1), gl5_dbl(t7)));
  gl5 t10 = gl5_mul(gl5_add(t4, gl5_dbl(t3)), gl5_add(t5, t7));
  pt r;
  r.X = gl5_mul_kz(gl5_sub(t10, t8), EC_B1);
  r.Z = gl5_sub(t8, t9);
  r.U = gl5_mul(t6, gl5_sub(gl5_mul_kz(t2, EC_B1), t1));
  r.T = gl5_add(t8, t9);
  return r;
}
GLN pt pt_dbl(const pt& p) {
  gl5 t1 = gl5_mul(p.Z, p.T), t2 = gl5_mul(t1, p.T);
  gl5 X1 = gl5_sqr(t2), Z1 = gl5_mul(t1, p.U), t3 = gl5_sqr(p.U);
  gl5 W1 = gl5_sub(t2, gl5_mul(gl5_dbl(gl5_add(p.X, p.Z)), t3));
  gl5 t4 = gl5_sqr(Z1);
  pt r;
  r.X = gl5_mul_kz(t4, 4 * EC_B1);
  r.Z = gl5_sqr(W1);
  r.U = gl5_sub(gl5_sub(gl5_sqr(gl5_add(W1, Z1)), t4), r.Z);
  r.T = gl5_sub(gl5_sub(gl5_dbl(X1), gl5_small(t4, 4)), r.Z);
  return r;
}
// Four successive doublings (one window of pt_mul128). The first leaves the fractional coordinates for Jacobian ones, x = X / Z^2 and
// w = 1 / u = W / Z, in which doubling is 1M + 7S:  D = W^2 - 2X - 2Z^2,  X' = 16 b (WZ)^4,  W' = 2 W^4 - 4 (WZ)^2 - D^2,  Z' = 2 D W Z
// (the same map as pt_dbl, x' = 4 b w^2 / D_a^2 and w' = (2 w^4 - 4 w^2 - D_a^2) / (2 w D_a) with D_a = w^2 - 2x - 2, on those
// coordinates); (X : Z^2 : Z : W) are fractional coordinates again. 4M + 6S, then 3 x (1M + 7S), then 1S: 595 base products against
// 4 x (4M + 5S) = 700. The neutral element has Z = 0 in the Jacobian form and is put back by hand.
GLN pt pt_dbl4(const pt& p) {
  gl5 X, W, Z;
  {
    gl5 t1 = gl5_mul(p.Z, p.T), t2 = gl5_mul(t1, p.T);
    gl5 X1 = gl5_sqr(t2), Z1 = gl5_mul(t1, p.U), t3 = gl5_sqr(p.U);
    gl5 W1 = gl5_sub(t2, gl5_mul(gl5_dbl(gl5_add(p.X, p.Z)), t3));
    gl5 z2 = gl5_sqr(Z1), w2 = gl5_sqr(W1);
    Z = gl5_sub(gl5_sub(gl5_sqr(gl5_add(W1, Z1)), z2), w2);    // 2 W1 Z1
    X = gl5_mul_kz(gl5_sqr(z2), 16 * EC_B1);                    // 16 b Z1^4
    W = gl5_sub(gl5_sub(gl5_dbl(X1), gl5_small(z2, 4)), w2);    // 2 X1 - 4 Z1^2 - W1^2
  }
#pragma unroll 1
  for (int i = 0; i < 3; i++) {
    gl5 w2 = gl5_sqr(W), z2 = gl5_sqr(Z);
    gl5 wz2 = gl5_sub(gl5_sub(gl5_sqr(gl5_add(W, Z)), w2), z2);  // 2 W Z
    gl5 D = gl5_sub(gl5_sub(w2, gl5_dbl(X)), gl5_dbl(z2));
    gl5 a = gl5_sqr(wz2);                                         // 4 (WZ)^2
    X = gl5_mul_kz(gl5_sqr(a), EC_B1);
    W = gl5_sub(gl5_sub(gl5_dbl(gl5_sqr(w2)), a), gl5_sqr(D));
    Z = gl5_mul(D, wz2);
  }
  if (gl5_is_zero(Z)) return pt_neutral();
  pt r;
  r.X = X; r.Z = gl5_sqr(Z); r.U = Z; r.T = W;
  return r;
}
GLD gl5 pt_encode(const pt& p) { return gl5_mul(p.T, gl5_inv(p.U)); }  // neutral -> 0
// decode(w): x^2 - (w^2 - a) x + b = 0, keep the non-square root; (x, 1, 1, w)
GLN bool pt_decode(gl5 w, pt& out) {
  gl5 e = gl5_sub(gl5_sqr(w), gl5_from(2));
  gl5 b4 = gl5_zero(); b4.c[1] = 4 * EC_B1;
  gl5 delta = gl5_sub(gl5_sqr(e), b4);
  gl5 r;
  if (!gl5_sqrt(delta, r)) { out = pt_neutral(); return gl5_is_zero(w); }
  const u64 half = 0x7FFFFFFF80000001ULL;  // (p+1)/2
  gl5 x1 = gl5_scale(gl5_add(e, r), half), x2 = gl5_scale(gl5_sub(e, r), half);
  gl5 x = gl5_is_square(x1) ? x2 : x1;
  out.X = x; out.Z = gl5_from(1); out.U = gl5_from(1); out.T = w;
  return true;
}
// [x0..x4, y0..y4, is_inf] of the short Weierstrass image (mod.rs:163-174): X = x + 2/3, Y = -w x
GLD void pt_to_weierstrass(const pt& p, u64 out[11]) {
  gl5 w = pt_encode(p);
  gl5 x = gl5_mul(p.X, gl5_inv(p.Z));
  if (gl5_is_zero(x)) {
#pragma unroll
    for (int i = 0; i < 10; i++) out[i] = 0;
    out[10] = 1;
    return;
  }
  gl5 y = gl5_neg(gl5_mul(w, x));
  x.c[0] = gl_add(x.c[0], 6148914689804861441ULL);
#pragma unroll
  for (int i = 0; i < 5; i++) { out[i] = x.c[i]; out[5 + i] = y.c[i]; }
  out[10] = 0;
}
// k * p, k = 128-bit little-endian (k[0] least significant).
// Signed 4-bit windows: the scalar recoded into 33 digits in [-8, 8], {0..8} * p in the lane's scratch, four doublings (pt_dbl4:
// a run in Jacobian coordinates) and one complete addition (of +-table[|digit|]; -P = (X : Z : -U : T)) per digit: 128 doublings +
// 32 additions + 7 for the table. The
// bit-serial double-and-add this replaces paid close to 128 additions: a wave takes the "bit set" branch
// whenever any of its 64 lanes has the bit. The projective representative differs from the bit-serial one; every consumer reads
// points through the canonical encodings (pt_emit / pt_to_weierstrass) or adds them.
GLD pt pt_mul128(const pt& p, const u32 k[4]) {
  pt tab[9];
  tab[0] = pt_neutral(); tab[1] = p; tab[2] = pt_dbl(p); tab[3] = pt_add(tab[2], p); tab[4] = pt_dbl(tab[2]);
  tab[5] = pt_add(tab[4], p); tab[6] = pt_dbl(tab[3]); tab[7] = pt_add(tab[6], p); tab[8] = pt_dbl(tab[4]);
  u32 mag[4] = {0, 0, 0, 0}, neg[4] = {0, 0, 0, 0}, carry = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    const u32 d = ((k[i >> 3] >> ((i & 7) * 4)) & 15) + carry;  // 0..16
    carry = d > 8;
    mag[i >> 3] |= (carry ? 16 - d : d) << ((i & 7) * 4);
    neg[i >> 3] |= carry << (i & 7);
  }
  pt acc = tab[carry];  // the 33rd digit
#pragma unroll
  for (int w = 3; w >= 0; w--) {
#pragma unroll 1
    for (int i = 7; i >= 0; i--) {
      acc = pt_dbl4(acc);
      pt q = tab[(mag[w] >> (i * 4)) & 15];
      if ((neg[w] >> i) & 1) q.U = gl5_neg(q.U);
      acc = pt_add(acc, q);
    }
  }
  return acc;
}

// sswu_value.rs:31-77
GLN pt simple_swu(gl5 u) {
  const gl5 two_thirds = gl5_from(6148914689804861441ULL);
  const gl5 a_sw = gl5_make(6148914689804861439ULL, 263, 0, 0, 0);
  const gl5 b_sw = gl5_make(15713893096167979237ULL, 6148914689804861265ULL, 0, 0, 0);
  const gl5 z_sw = gl5_make(GL_P - 4, GL_P - 1, 0, 0, 0);
  const gl5 neg_z_inv = gl5_make(4795794222525505369ULL, 3412737461722269738ULL, 8370187669276724726ULL,
                                 7130825117388110979ULL, 12052351772713910496ULL);
  const gl5 neg_b_div_a = gl5_make(6585749426319121644ULL, 16990361517133133838ULL, 3264760655763595284ULL,
                                   16784740989273302855ULL, 13434657726302040770ULL);
  gl5 denom_part = gl5_mul(z_sw, gl5_sqr(u));
  gl5 denom = gl5_add(gl5_sqr(denom_part), denom_part);
  gl5 tv1 = gl5_inv(denom);
  gl5 x1 = gl5_mul(gl5_is_zero(tv1) ? neg_z_inv : gl5_add(tv1, gl5_from(1)), neg_b_div_a);
  gl5 x2 = gl5_mul(denom_part, x1);
  gl5 gx1 = gl5_add(gl5_add(gl5_mul(x1, gl5_sqr(x1)), gl5_mul(a_sw, x1)), b_sw);
  gl5 x_sw = x1, y_pos;
  // which candidate has a square g(x) is a Legendre symbol (a norm to GF(p) and 63 base-field squarings), an eighth of the square
  // root whose failure would say the same. Every lane computes g(x2) (three products) and the wave takes ONE square root, of the
  // lane's own choice: branching on the symbol would send a wave through gl5_sqrt twice, its lanes split over the two candidates.
  {
    const bool first = gl5_is_square(gx1);
    const gl5 gx2 = gl5_add(gl5_add(gl5_mul(x2, gl5_sqr(x2)), gl5_mul(a_sw, x2)), b_sw);
    gl5 g;
#pragma unroll
    for (int i = 0; i < 5; i++) { g.c[i] = first ? gx1.c[i] : gx2.c[i]; x_sw.c[i] = first ? x1.c[i] : x2.c[i]; }
    gl5_sqrt(g, y_pos);
  }
  gl5 x_cand = gl5_sub(x_sw, two_thirds);
  gl5 y_cand = gl5_sgn0(u) == gl5_sgn0(y_pos) ? y_pos : gl5_neg(y_pos);
  pt p;
  // Point::decode(w), w = y / x, without its square root: (x_cand, y_cand) is on y^2 = x (x^2 + a x + b), so w^2 - a = x + b / x and
  // the two roots of decode's quadratic x^2 - (w^2 - a) x + b are x_cand and b / x_cand; decode keeps the non-square one (their
  // product b = 263 z is a non-square, so exactly one is). The general path stays for the degenerate encodings.
  const gl5 xi = gl5_inv(x_cand);
  const gl5 w = gl5_mul(y_cand, xi);
  if (gl5_is_zero(w) || gl5_is_zero(x_cand)) {
    pt_decode(w, p);
  } else {
    p.X = gl5_is_square(x_cand) ? gl5_mul_kz(xi, EC_B1) : x_cand;
    p.Z = gl5_from(1); p.U = gl5_from(1); p.T = w;
  }
  return p;
}
template <int V>
GLD pt map_to_curve(const u64* in, u32 n) {
  u64 s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  for (u32 p = 0; p < n; p += 8) {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (p + k < n) s[k] = in[p + k];
    perm<V>(s);
  }
  return simple_swu(gl5_make(s[0], s[1], s[2], s[3], s[4]));
}
GLD void pt_store(u64* d, const pt& p) {
#pragma unroll
  for (int i = 0; i < 5; i++) { d[i] = p.X.c[i]; d[5 + i] = p.Z.c[i]; d[10 + i] = p.U.c[i]; d[15 + i] = p.T.c[i]; }
}
GLD pt pt_load(const u64* d) {
  pt p;
#pragma unroll
  for (int i = 0; i < 5; i++) { p.X.c[i] = d[i]; p.Z.c[i] = d[5 + i]; p.U.c[i] = d[10 + i]; p.T.c[i] = d[15 + i]; }
  return p;
}
GLD void pt_emit(const pt& p, u64* w, u64* wei) {
  if (w) { gl5 e = pt_encode(p); for (int i = 0; i < 5; i++) w[i] = e.c[i]; }
  if (wei) pt_to_weierstrass(p, wei);
}
}  // namespace mp2g
