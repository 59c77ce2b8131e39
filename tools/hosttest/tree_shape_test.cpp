// Host-side view of csrc/tree_shape.h (heights, levels, min / max indices and roots of a binary forest; ryhope's sbbst), so that a
// test can hold Python restatements against it (tests/test_tree_shape_host.py).
// build: hipcc -x hip --cuda-host-only -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17
//        -I../../mapreduce-plonky2_amd/csrc tree_shape_test.cpp -o tree_shape_test
// run:   tree_shape_test < cases, one case per line:
//          tree N l0 r0 l1 r1 ...   the forest with these children (decimal, -1 = none), in arrays of exactly N entries
//          sbbst N                  the sbbst over N positions; prints "sbbst ROOT" (the root position) before the shape
//          chain N SIDE             a chain of N nodes built here, node i's only child i + 1 on SIDE (0 left, 1 right); prints only
//                                   "chain LEVELS NUM_ROOTS HEIGHT_OF_NODE_0 MIN_IDX_0 MAX_IDX_0"
//        a shape prints "ok LEVELS" and then the lines "left", "right", "height", "min", "max", "roots", "order", "off", each followed
//        by its numbers; a refused one prints "refused # MESSAGE".
#include "tree_shape.h"
#include <cinttypes>
#include <cstdio>
using namespace mp2g;

template <class T>
static void line(const char* name, const std::vector<T>& v) {
  printf("%s", name);
  for (T x : v) printf(" %lld", (long long)x);
  printf("\n");
}
static void show(const std::vector<int32_t>& l, const std::vector<int32_t>& r) {
  TreeShape s;
  const char* err = tree_shape_build(l.data(), r.data(), (uint32_t)l.size(), s);
  if (err) { printf("refused # %s\n", err); return; }
  printf("ok %u\n", s.levels());
  line("left", s.left); line("right", s.right); line("height", s.height); line("min", s.min_idx); line("max", s.max_idx);
  line("roots", s.roots); line("order", s.order); line("off", s.level_off);
}
int main() {
  char what[16];
  uint32_t n;
  while (scanf("%15s %" SCNu32, what, &n) == 2) {
    std::vector<int32_t> l(n), r(n);
    if (what[0] == 't') {
      for (uint32_t i = 0; i < n; i++)
        if (scanf("%" SCNd32 " %" SCNd32, &l[i], &r[i]) != 2) return 2;
      show(l, r);
    } else if (what[0] == 's') {
      sbbst_fill(n, l.data(), r.data());
      printf("sbbst %llu\n", (unsigned long long)sbbst_root(n));
      show(l, r);
    } else if (what[0] == 'c') {
      int side;
      if (scanf("%d", &side) != 1) return 2;
      for (uint32_t i = 0; i < n; i++) {
        l[i] = r[i] = -1;
        if (i + 1 < n) (side ? r : l)[i] = (int32_t)(i + 1);
      }
      TreeShape s;
      const char* err = tree_shape_build(l.data(), r.data(), n, s);
      if (err || !n) { printf("refused # %s\n", err ? err : "a chain needs a node"); continue; }
      printf("chain %u %zu %u %u %u\n", s.levels(), s.roots.size(), s.height[0], s.min_idx[0], s.max_idx[0]);
    } else
      return 2;
  }
  return 0;
}
