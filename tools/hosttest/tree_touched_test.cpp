// Host-side view of tree_shape_touched (csrc/tree_shape.h): the touched nodes of a forest and all their ancestors, grouped by
// height, so that a test can hold a plain parent walk in Python against it (tests/test_tree_touched_host.py).
// build: hipcc -x hip --cuda-host-only -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17
//        -I../../mapreduce-plonky2_amd/csrc tree_touched_test.cpp -o tree_touched_test
// run:   tree_touched_test < cases, one case per line:
//          tree N l0 r0 l1 r1 ...   makes the forest with these children (decimal, -1 = none) the current shape; prints "ok LEVELS"
//                                   and the line "parent" with its N numbers, or "refused # MESSAGE"
//          touch K t0 t1 ...        the closure of these K nodes in the current shape; prints "nodes" and "off", each followed by its
//                                   numbers, or "refused # MESSAGE"
//          deep N                   a left chain of N nodes built here (node i's only child is i + 1) with node N - 1 touched; prints
//                                   only "deep COUNT LEVELS WIDEST FIRST LAST SUM" (first and last closure node, the sum of all)
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
int main() {
  char what[16];
  uint32_t n;
  TreeShape s;
  TreeTouched c;
  while (scanf("%15s %" SCNu32, what, &n) == 2) {
    if (what[0] == 't' && what[1] == 'r') {
      std::vector<int32_t> l(n), r(n);
      for (uint32_t i = 0; i < n; i++)
        if (scanf("%" SCNd32 " %" SCNd32, &l[i], &r[i]) != 2) return 2;
      const char* err = tree_shape_build(l.data(), r.data(), n, s);
      if (err) { printf("refused # %s\n", err); continue; }
      printf("ok %u\n", s.levels());
      line("parent", s.parent);
    } else if (what[0] == 't') {
      std::vector<uint32_t> t(n);
      for (uint32_t i = 0; i < n; i++)
        if (scanf("%" SCNu32, &t[i]) != 1) return 2;
      const char* err = tree_shape_touched(s, t.data(), n, c);
      if (err) { printf("refused # %s\n", err); continue; }
      line("nodes", c.nodes);
      line("off", c.level_off);
    } else if (what[0] == 'd') {
      std::vector<int32_t> l(n, -1), r(n, -1);
      for (uint32_t i = 0; i + 1 < n; i++) l[i] = (int32_t)(i + 1);
      const char* err = tree_shape_build(l.data(), r.data(), n, s);
      const uint32_t deepest = n - 1;
      if (!err && n) err = tree_shape_touched(s, &deepest, 1, c);
      if (err || !n) { printf("refused # %s\n", err ? err : "a chain needs a node"); continue; }
      unsigned long long sum = 0;
      for (uint32_t x : c.nodes) sum += x;
      printf("deep %zu %u %u %u %u %llu\n", c.nodes.size(), c.levels(), c.widest, c.nodes.front(), c.nodes.back(), sum);
    } else
      return 2;
  }
  return 0;
}
