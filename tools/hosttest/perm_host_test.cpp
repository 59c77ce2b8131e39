// Host-side check of the device arithmetic headers (the GLHD functions): the portable (#else) bodies.
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -DMP2G_DEVCONST="static const" \
//        -I../../mapreduce-plonky2_amd/csrc perm_host_test.cpp -x none ../../oracle/liboracle.so -o perm_host_test
// Without arguments: the permutations against the C oracle and the primitives against unsigned __int128, on its own random inputs.
// With `perm_host_test REQUEST RESULT`: table mode for tests/test_field_host.py -- runs ONE named routine on the operand table in
// REQUEST and writes its raw outputs to RESULT; the test compares them with the reference of tests/field_cases.py, the same table
// and reference that the device bodies face in tests/test_gpu_field_device.py. Nothing is judged here in that mode.
#include "gl5.cuh"
#include "poseidon.cuh"
#include "../../tests/devfield/field_ops.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace mp2g;
extern "C" void orc_perm(int variant, uint64_t s[12]);
static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// ---- table mode -----------------------------------------------------------------------------------------------------------------
// REQUEST: u64 shape (0 scalar, 1 gl_cols, 2 vector), n, p0, p1, then char name[32], then the operands:
//   scalar: a[n] b[n] c[n] -> o0[n] o1[n]        (weak-output routines: o1 = gl_canon(o0))
//   gl_cols: p0 = terms, p1 = f; a[n][terms] b[n][terms] -> out[n]
//   vector: p0 = k, p1 = 0 no second operand / 1 y[n][w] / 2 twelve shared round constants; x[n][w] -> out[n][w] flag[n]
static bool read_words(FILE* f, std::vector<u64>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), 8, n, f) == n;
}
static int vec_width(const char* name) { return !strncmp(name, "gl2_", 4) ? 2 : (!strncmp(name, "gl5_", 4) ? 5 : 12); }

static int table_mode(const char* request, const char* result) {
  FILE* f = fopen(request, "rb");
  u64 h[4];
  char name[32];
  if (!f || fread(h, 8, 4, f) != 4 || fread(name, 1, 32, f) != 32 || name[31] != 0) { fprintf(stderr, "bad request\n"); return 2; }
  const u64 shape = h[0], n = h[1];
  std::vector<u64> a, b, c, out, out1;
  if (shape == 0) {
    if (!read_words(f, a, n) || !read_words(f, b, n) || !read_words(f, c, n)) return 2;
    out.assign(n, 0);
    out1.assign(n, 0);
    bool known = false;
    const u64 *pa = a.data(), *pb = b.data(), *pc = c.data();
#define X(op, body)                                                                   \
  if (!strcmp(name, #op)) {                                                           \
    known = true;                                                                     \
    for (u64 i = 0; i < n; i++) {                                                     \
      const u64 a = pa[i], b = pb[i], c = pc[i];                                      \
      u64 o0 = 0, o1 = 0;                                                             \
      (void)a; (void)b; (void)c;                                                      \
      body;                                                                           \
      out[i] = o0; out1[i] = o1;                                                      \
    }                                                                                 \
  }
    SCALAR_OPS_HD(X)
#undef X
    if (!known) { fprintf(stderr, "no host body for %s\n", name); return 2; }
  } else if (shape == 1) {
    const u64 terms = h[2], fac = h[3];
    if (!read_words(f, a, n * terms) || !read_words(f, b, n * terms)) return 2;
    out.assign(n, 0);
    for (u64 i = 0; i < n; i++) {
      gl_cols acc;
      for (u64 k = 0; k < terms; k++) {
        if (fac == 0) acc.add(a[i * terms + k], b[i * terms + k]); else acc.add_scaled(a[i * terms + k], b[i * terms + k], (u32)fac);
      }
      out[i] = acc.value();
    }
  } else if (shape == 2) {
    const u32 k = (u32)h[2];
    const u64 w = vec_width(name);
    if (!read_words(f, a, n * w) || !read_words(f, b, h[3] == 1 ? n * w : (h[3] == 2 ? 12 : 0))) return 2;
    out.assign(n * w, 0);
    out1.assign(n, 0);
    const u64* rc = h[3] == 2 ? b.data() : nullptr;
    for (u64 i = 0; i < n; i++) {
      const u64* x = &a[i * w];
      const u64* y = h[3] == 1 ? &b[i * w] : nullptr;
      u64* o = &out[i * w];
      if (w == 2) {
        gl2 r;
        if (!strcmp(name, "gl2_mul") && y) r = gl2_mul(gl2_make(x[0], x[1]), gl2_make(y[0], y[1]));
        else if (!strcmp(name, "gl2_inv")) r = gl2_inv(gl2_make(x[0], x[1]));
        else if (!strcmp(name, "gl2_scale") && y) r = gl2_scale(gl2_make(x[0], x[1]), y[0]);
        else return 2;
        o[0] = r.a; o[1] = r.b;
      } else if (w == 5) {
        const gl5 v = gl5_make(x[0], x[1], x[2], x[3], x[4]);
        gl5 r = gl5_zero();
        if (!strcmp(name, "gl5_mul") && y) r = gl5_mul(v, gl5_make(y[0], y[1], y[2], y[3], y[4]));
        else if (!strcmp(name, "gl5_sqr")) r = gl5_sqr(v);
        else if (!strcmp(name, "gl5_small")) r = gl5_small(v, k);
        else if (!strcmp(name, "gl5_mul_kz")) r = gl5_mul_kz(v, k);
        else if (!strcmp(name, "gl5_frob1")) r = gl5_frob1(v);
        else if (!strcmp(name, "gl5_frob2")) r = gl5_frob2(v);
        else if (!strcmp(name, "gl5_inv")) r = gl5_inv(v);
        else if (!strcmp(name, "gl5_norm")) r.c[0] = gl5_norm(v);
        else if (!strcmp(name, "gl5_sqrt")) out1[i] = gl5_sqrt(v, r) ? 1 : 0;
        else if (!strcmp(name, "gl5_is_square")) out1[i] = gl5_is_square(v) ? 1 : 0;
        else if (!strcmp(name, "gl5_sgn0")) out1[i] = gl5_sgn0(v) ? 1 : 0;
        else return 2;
        memcpy(o, r.c, 40);
      } else {
        u64 s[12];
        memcpy(s, x, 96);
        if (!strcmp(name, "p2_external")) p2_external_rc<false>(s, nullptr);
        else if (!strcmp(name, "p2_external_rc") && (rc || k < 8)) p2_external_rc<true>(s, rc ? rc : c_p2_ext + 12 * k);
        else if (!strcmp(name, "p2_internal")) p2_internal(s);
        else if (!strcmp(name, "poseidon_mds")) poseidon_mds_rc<false>(s, nullptr);
        else if (!strcmp(name, "poseidon_mds_rc") && (rc || k < 30)) poseidon_mds_rc<true>(s, rc ? rc : c_p_rc + 12 * k);
        else if (!strcmp(name, "poseidon2_perm")) poseidon2_perm(s);
        else if (!strcmp(name, "poseidon_perm")) poseidon_perm(s);
        else { fprintf(stderr, "no host body for %s\n", name); return 2; }
        memcpy(o, s, 96);
      }
    }
  } else {
    return 2;
  }
  fclose(f);
  FILE* g = fopen(result, "wb");
  if (!g || fwrite(out.data(), 8, out.size(), g) != out.size() || fwrite(out1.data(), 8, out1.size(), g) != out1.size() || fclose(g)) return 2;
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3) return table_mode(argv[1], argv[2]);
  const uint64_t edge[] = {0, 1, GL_P - 1, GL_P - 2, 0xFFFFFFFFull, 0xFFFFFFFF00000000ull, 0x100000000ull, GL_P >> 1};
  long bad = 0;
  for (int variant = 0; variant < 2; variant++)
    for (int it = 0; it < 20000; it++) {
      uint64_t a[12], b[12];
      for (int i = 0; i < 12; i++) {
        uint64_t v = (it < 4000 && (rnd() & 3)) ? edge[rnd() % 8] : rnd() % GL_P;
        a[i] = b[i] = v;
      }
      if (variant == 0) poseidon2_perm(a); else poseidon_perm(a);
      orc_perm(variant, b);
      for (int i = 0; i < 12; i++) if (a[i] != b[i]) bad++;
    }
  // weak primitives on adversarial non-canonical inputs
  for (int it = 0; it < 2000000; it++) {
    uint64_t x = (rnd() & 1) ? ~0ull - (rnd() & 0xFFFFFFFFull) : rnd();
    uint64_t y = (rnd() & 1) ? ~0ull - (rnd() & 0xFFFFFFFFull) : rnd();
    unsigned __int128 pr = (unsigned __int128)x * y;
    uint64_t want = (uint64_t)(pr % GL_P);
    if (gl_canon(gl_mulw(x, y)) != want) bad++;
    uint64_t yc = y % GL_P;
    if (gl_canon(gl_addw(x, yc)) != (uint64_t)(((unsigned __int128)x + yc) % GL_P)) bad++;
  }
  // canonical primitives on edge and random canonical inputs
  for (int it = 0; it < 2000000; it++) {
    uint64_t x = (it < 4096) ? edge[it & 7] : rnd() % GL_P, y = (it < 4096) ? edge[(it >> 3) & 7] : rnd() % GL_P;
    if (gl_add(x, y) != (uint64_t)(((unsigned __int128)x + y) % GL_P)) bad++;
    if (gl_sub(x, y) != (uint64_t)(((unsigned __int128)x + GL_P - y) % GL_P)) bad++;
    if (gl_mul(x, y) != (uint64_t)(((unsigned __int128)x * y) % GL_P)) bad++;
    uint32_t c = (uint32_t)rnd();
    if (gl_mul_small(x, c) != (uint64_t)(((unsigned __int128)x * c) % GL_P)) bad++;
    uint64_t any = rnd() | ((it & 1) ? 0xFFFFFFFF00000000ull : 0);
    if (gl_canon(any) != any % GL_P) bad++;
  }
  printf(bad ? "FAIL %ld\n" : "host arithmetic ok\n", bad);
  return bad != 0;
}
