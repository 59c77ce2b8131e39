// Host-side run of csrc/mpt_graph.cuh: the passes that build a trie's shape from its proofs and the sum of a node over its
// children, the same text the kernels of mpt_digest.hip compile, for the host alone and with the plain policy (no atomics).
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -I../../mapreduce-plonky2_amd/csrc -I../../include mpt_graph_host_test.cpp -o mpt_graph_host_test
// (tests/test_mpt_graph_host.py, which also builds it with -fsanitize=address,undefined).
// `mpt_graph_host_test REQUEST RESULT`. REQUEST is u32 n_nodes, count, max_depth, has_status, backwards; u32 info[n_nodes]; u32
// paths[count][max_depth]; u32 depths[count]; u8 keys[count][32]; with has_status u32 status[count]; u64 leaf[count][20]: the
// arguments of mp2g_mpt_subtree_digests_dev. RESULT receives u64 acc[n_nodes][20], u32 n_leaves / state / via / parent [n_nodes],
// u8 entered[n_nodes], u32 totals[3]. With `backwards` every pass takes the proofs from the last to the first: the result must not
// depend on the order. A point is an opaque token of 20 words here and the sum is word by word, so what comes out says which
// leaves fed which node, not what the curve does. Nothing is judged here.
// Every array lives in a heap block of exactly its size: a read or write outside is a heap overflow that a sanitizer build
// reports, not luck.
#include "mpt_graph.cuh"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace mp2g;

struct Plain {
  static void min64(u64* p, u64 v) { if (v < *p) *p = v; }
  static void min32(u32* p, u32 v) { if (v < *p) *p = v; }
  static void or32(u32* p, u32 v) { *p |= v; }
};
struct Tokens {
  struct point { u64 w[20]; };
  static point neutral() { point p; memset(p.w, 0, sizeof(p.w)); return p; }
  static point load(const u64* d) { point p; memcpy(p.w, d, sizeof(p.w)); return p; }
  static point add(const point& a, const point& b) { point p; for (int k = 0; k < 20; k++) p.w[k] = a.w[k] + b.w[k]; return p; }
  static void store(u64* d, const point& p) { memcpy(d, p.w, sizeof(p.w)); }
};

// a heap block of exactly n elements (one byte when n is 0, so that the pointer is still a block's)
template <class T>
static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }
template <class T>
static T* block_from(FILE* f, size_t n, bool* ok) {
  T* p = block<T>(n);
  if (fread(p, sizeof(T), n, f) != n) *ok = false;
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: mpt_graph_host_test REQUEST RESULT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  u32 h[5];
  if (!f || fread(h, 4, 5, f) != 5) { fprintf(stderr, "bad request\n"); return 2; }
  const u32 n_nodes = h[0], count = h[1], max_depth = h[2], has_status = h[3], backwards = h[4];
  if (!max_depth || max_depth > MP2G_MPT_MAX_DEPTH) { fprintf(stderr, "a max_depth the library would refuse\n"); return 2; }
  bool ok = true;
  u32* info = block_from<u32>(f, n_nodes, &ok);
  u32* paths = block_from<u32>(f, (size_t)count * max_depth, &ok);
  u32* depths = block_from<u32>(f, count, &ok);
  uint8_t* keys = block_from<uint8_t>(f, (size_t)count * 32, &ok);
  u32* status = has_status ? block_from<u32>(f, count, &ok) : nullptr;
  u64* leaf = block_from<u64>(f, (size_t)count * 20, &ok);
  if (!ok) { fprintf(stderr, "short request\n"); return 2; }
  fclose(f);
  const size_t n = n_nodes;
  u64* ref = block<u64>(n);
  u32 *child = block<u32>(16 * n), *direct = block<u32>(n), *above = block<u32>(n), *parent = block<u32>(n), *les = block<u32>(n);
  uint8_t* taken = block<uint8_t>(count);
  memset(ref, 0xff, 8 * n);
  memset(child, 0xff, 64 * n);
  memset(direct, 0, 4 * n);
  memset(above, 0, 4 * n);
  // every proof's path row and key in blocks of their own, as the kernels see one row each
  std::vector<u32*> path(count);
  std::vector<uint8_t*> key(count);
  for (u32 i = 0; i < count; i++) {
    path[i] = block<u32>(max_depth);
    key[i] = block<uint8_t>(32);
    memcpy(path[i], paths + (size_t)i * max_depth, 4 * (size_t)max_depth);
    memcpy(key[i], keys + 32 * (size_t)i, 32);
  }
  u32 totals[3] = {0, 0, 0};
  auto each = [&](auto&& pass) {
    for (u32 t = 0; t < count; t++) pass(backwards ? count - 1 - t : t);
  };
  each([&](u32 i) {
    taken[i] = mpt_graph_minima<Plain>(info, n_nodes, path[i], depths[i], max_depth, key[i], status, i, ref, child);
    totals[0] += !taken[i];
  });
  each([&](u32 i) { if (taken[i]) mpt_graph_own(info, path[i], depths[i], key[i], i, ref, parent, les); });
  each([&](u32 i) { if (taken[i]) mpt_graph_compare<Plain>(info, path[i], depths[i], key[i], parent, les, child, direct); });
  each([&](u32 i) { if (taken[i]) mpt_graph_above<Plain>(path[i], depths[i], direct, above); });
  // the nodes: the outputs, and the OK nodes by level
  u64* acc = block<u64>(20 * n);
  u32 *n_leaves = block<u32>(n), *state = block<u32>(n), *via = block<u32>(n), *out_parent = block<u32>(n);
  uint8_t* entered = block<uint8_t>(n);
  std::vector<std::vector<u32>> levels(MP2G_MPT_MAX_DEPTH);
  for (u32 x = 0; x < n_nodes; x++) {
    const MptNodeShape s = mpt_graph_node(x, ref, parent, les, direct, above);
    state[x] = s.state; via[x] = s.via; out_parent[x] = s.parent; entered[x] = (uint8_t)s.entered;
    if (s.state != MP2G_MPT_SUBTREE_UNREACHED && s.level + 1 > totals[2]) totals[2] = s.level + 1;
    totals[1] += s.state == MP2G_MPT_SUBTREE_CONFLICT;
    if (s.state == MP2G_MPT_SUBTREE_OK) { levels[s.level].push_back(x); continue; }
    n_leaves[x] = 0;
    Tokens::store(acc + 20 * (size_t)x, Tokens::neutral());
  }
  for (u32 lv = MP2G_MPT_MAX_DEPTH; lv-- > 0;)
    for (u32 x : levels[lv]) mpt_graph_sum<Tokens>(x, info, child, ref, leaf, acc, n_leaves);
  f = fopen(argv[2], "wb");
  ok = f && fwrite(acc, 8, 20 * n, f) == 20 * n && fwrite(n_leaves, 4, n, f) == n && fwrite(state, 4, n, f) == n && fwrite(via, 4, n, f) == n &&
       fwrite(out_parent, 4, n, f) == n && fwrite(entered, 1, n, f) == n && fwrite(totals, 4, 3, f) == 3;
  if (!ok) { fprintf(stderr, "cannot write the result\n"); return 2; }
  fclose(f);
  for (u32 i = 0; i < count; i++) { free(path[i]); free(key[i]); }
  for (void* p : {(void*)info, (void*)paths, (void*)depths, (void*)keys, (void*)status, (void*)leaf, (void*)ref, (void*)child, (void*)direct,
                  (void*)above, (void*)parent, (void*)les, (void*)taken, (void*)acc, (void*)n_leaves, (void*)state, (void*)via, (void*)out_parent,
                  (void*)entered})
    free(p);
  return 0;
}
