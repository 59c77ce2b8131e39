// Host-side run of csrc/mpt.cuh: the node opener and the walk of one path, the same text the kernels of mpt.hip compile, for the
// host alone.
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -I../../mapreduce-plonky2_amd/csrc -I../../include mpt_host_test.cpp -o mpt_host_test
// (tests/test_mpt_host.py, which also builds it with -fsanitize=address,undefined).
// `mpt_host_test REQUEST RESULT`. REQUEST is u32 n_nodes, stride, count, max_depth, root_stride, mode, has_roots, has_info; u32
// lens[n_nodes]; u8 rows[n_nodes][stride]; u32 paths[count][max_depth]; u32 depths[count]; u8 keys[count][32]; then, with
// has_roots, u8 roots[root_stride ? count : 1][32]: the arguments of mp2g_mpt_verify_paths; then, with has_info, u32
// info[n_nodes] that the walk is given in place of stage 1's (words that are not the nodes'). RESULT receives hashes[n_nodes][32],
// u32 info[n_nodes], u32 status[count], u32 fail_level[count], u8 words[count][32], u32 val_off[count], u32 val_len[count],
// u8 consumed[count][max_depth]. Nothing is judged here.
// Every node is copied into a heap block of its own of min(len, stride) bytes rounded up to 8, every path, key and consumed row
// into one of exactly its size: a read or write outside is a heap overflow that a sanitizer build reports, not luck.
#include "mpt.cuh"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace mp2g;

struct HostNodes {
  std::vector<uint8_t*> blocks;
  std::vector<u32> lens;
  u32 stride;
  const uint8_t* node(u32 idx) const { return blocks[idx]; }
  u32 len(u32 idx) const { return lens[idx] > stride ? stride : lens[idx]; }
};

template <class T>
static bool read_all(FILE* f, std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T>
static bool write_all(FILE* f, const std::vector<T>& v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: mpt_host_test REQUEST RESULT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  u32 h[8];
  if (!f || fread(h, 4, 8, f) != 8) { fprintf(stderr, "bad request\n"); return 2; }
  const u32 n_nodes = h[0], stride = h[1], count = h[2], max_depth = h[3], root_stride = h[4], mode = h[5], has_roots = h[6], has_info = h[7];
  if (!stride || stride % 8 || !max_depth || max_depth > MP2G_MPT_MAX_DEPTH || (root_stride != 0 && root_stride != 32)) {
    fprintf(stderr, "a stride, max_depth or root_stride the library would refuse\n");
    return 2;
  }
  HostNodes nodes;
  nodes.stride = stride;
  nodes.lens.resize(n_nodes);
  std::vector<uint8_t> rows((size_t)n_nodes * stride), keys((size_t)count * 32), roots(has_roots ? (size_t)(root_stride ? count : 1) * 32 : 0);
  std::vector<u32> paths((size_t)count * max_depth), depths(count), foreign_info(has_info ? n_nodes : 0);
  if (!read_all(f, nodes.lens) || !read_all(f, rows) || !read_all(f, paths) || !read_all(f, depths) || !read_all(f, keys) || !read_all(f, roots) ||
      !read_all(f, foreign_info)) {
    fprintf(stderr, "short request\n");
    return 2;
  }
  fclose(f);
  // stage 1
  std::vector<u64> hashes((size_t)n_nodes * 4);
  std::vector<u32> info(n_nodes);
  for (u32 i = 0; i < n_nodes; i++) {
    const u32 n = nodes.len(i), room = (n + 7) / 8 * 8;
    uint8_t* block = (uint8_t*)malloc(room ? room : 1);
    memcpy(block, rows.data() + (size_t)i * stride, room);
    nodes.blocks.push_back(block);
    keccak256_lanes((const u64*)block, n, &hashes[4 * (size_t)i]);
    info[i] = mpt_open_node(block, n);
  }
  // stage 2
  std::vector<u32> status(count), fail_level(count), val_off(count), val_len(count);
  std::vector<u64> words((size_t)count * 4, 0), root_lanes(roots.size() / 8);
  std::vector<uint8_t> consumed((size_t)count * max_depth);
  if (!roots.empty()) memcpy(root_lanes.data(), roots.data(), roots.size());
  for (u32 i = 0; i < count; i++) {
    u32* path = (u32*)malloc(4 * (size_t)max_depth);
    uint8_t* key = (uint8_t*)malloc(32);
    uint8_t* cons = (uint8_t*)malloc(max_depth);
    memcpy(path, &paths[(size_t)i * max_depth], 4 * (size_t)max_depth);
    memcpy(key, &keys[32 * (size_t)i], 32);
    const MptWalk r = mpt_walk_path(nodes, hashes.data(), has_info ? foreign_info.data() : info.data(), n_nodes, path, depths[i], max_depth, key,
                                    has_roots ? &root_lanes[(size_t)(root_stride / 8) * i] : nullptr, mode, cons);
    status[i] = r.status; fail_level[i] = r.fail_level; val_off[i] = r.val_off; val_len[i] = r.val_len;
    if (mode != MP2G_MPT_VALUE_RAW) memcpy(&words[4 * (size_t)i], r.word, 32);
    memcpy(&consumed[(size_t)i * max_depth], cons, max_depth);
    free(path); free(key); free(cons);
  }
  for (uint8_t* b : nodes.blocks) free(b);
  f = fopen(argv[2], "wb");
  if (!f || !write_all(f, hashes) || !write_all(f, info) || !write_all(f, status) || !write_all(f, fail_level) || !write_all(f, words) ||
      !write_all(f, val_off) || !write_all(f, val_len) || !write_all(f, consumed)) {
    fprintf(stderr, "cannot write the result\n");
    return 2;
  }
  fclose(f);
  return 0;
}
