// What the index-hash kernels (index_hash.hip) need to know about a binary tree or forest over nodes 0..n-1 given by left[n] / right[n]
// (-1 = no child): every node's height (0 without children, else 1 + the larger of its children's; nodes of one height form one
// launch, and children always lie in lower levels), the node its min / max come from, the roots, and the nodes grouped by height.
//
// min_idx[i] / max_idx[i] is the node reached from i by following left (right) children until there is none: exactly
// RowPayload::aggregate's rule (mp2-v1/src/indexing/row.rs:261-285: min = left.min if a left child exists, else the node's own
// value; max symmetrically), carried as an index so that no U256 is compared -- the reference compares none either.
//
// The children arrays are caller data: tree_shape_build refuses, with a message that names the fault and without reading out of
// bounds, a child index outside -1..n-1, a node that is its own child, a node with two parents (left[i] == right[i] != -1 included)
// and a cycle (nodes no root reaches). Nothing here recurses: a chain of 2^20 nodes is a valid shape of height 2^20 - 1.
//
// Also ryhope's self-balanced BST over the positions 1..n (ryhope/src/tree/sbbst.rs: root :251-257, children :301-333 and :487-503),
// the shape of a cells tree and of the block tree; position k is node k - 1.
//
// tree_shape_touched is ryhope's touched() (ryhope/src/lib.rs:216-222): the dirty nodes and their lineages up to the roots, which is
// all that MerkleTreeKvDb::aggregate (:179-209) re-hashes after a block. It walks parent[] from each given node until it meets a node
// it has already taken, so its cost is the closure's size plus a sort, whatever the shape's.
// Host code only, no HIP: tools/hosttest/tree_shape_test.cpp and tree_touched_test.cpp compile it alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

namespace mp2g {

struct TreeShape {
  std::vector<int32_t> left, right;                 // [n] as given
  std::vector<uint32_t> height, min_idx, max_idx;   // [n]
  std::vector<uint32_t> roots;                      // nodes without a parent, ascending
  std::vector<uint32_t> order;                      // [n] the nodes sorted by height (ascending node index inside a height)
  std::vector<uint32_t> level_off;                  // [levels + 1]: level h is order[level_off[h] .. level_off[h + 1])
  std::vector<int32_t> parent;                      // [n], -1 for a root
  mutable std::vector<uint8_t> mark;                // [n] all zero between calls: tree_shape_touched's "already taken" (why a shape
                                                    // is not to be used from two threads at once)
  uint32_t size() const { return (uint32_t)left.size(); }
  uint32_t levels() const { return (uint32_t)level_off.size() - 1; }
};

// nullptr, or why the arrays are no forest (s is then empty). n = 0 is the empty shape: no level, no root.
inline const char* tree_shape_build(const int32_t* left, const int32_t* right, uint32_t n, TreeShape& s) {
  s = TreeShape();
  s.level_off.assign(1, 0);
  if (n > 0x7FFFFFFFu) return "more nodes than a 32-bit signed child index can name";
  if (n && (!left || !right)) return "left / right missing";
  std::vector<uint8_t> has_parent(n, 0);
  for (uint32_t i = 0; i < n; i++)
    for (int side = 0; side < 2; side++) {
      const int32_t c = side ? right[i] : left[i];
      if (c == -1) continue;
      if (c < 0 || (uint32_t)c >= n) return "child index outside -1 .. n-1";
      if ((uint32_t)c == i) return "a node is its own child";
      if (has_parent[c]) return "a node has two parents";
      has_parent[c] = 1;
    }
  std::vector<uint32_t> roots, visit;  // visit: parents before their children
  visit.reserve(n);
  for (uint32_t i = 0; i < n; i++)
    if (!has_parent[i]) { roots.push_back(i); visit.push_back(i); }
  // every node has at most one parent, so this reaches each node at most once and ends; what it does not reach hangs on a cycle
  for (size_t at = 0; at < visit.size(); at++) {
    const uint32_t i = visit[at];
    if (left[i] >= 0) visit.push_back((uint32_t)left[i]);
    if (right[i] >= 0) visit.push_back((uint32_t)right[i]);
  }
  if (visit.size() != n) return "a cycle: nodes that no root reaches";
  s.left.assign(left, left + n);
  s.right.assign(right, right + n);
  s.height.assign(n, 0);
  s.parent.assign(n, -1);
  s.mark.assign(n, 0);
  s.min_idx.resize(n);
  s.max_idx.resize(n);
  uint32_t top = 0;
  for (size_t at = visit.size(); at-- > 0;) {  // children before their parents
    const uint32_t i = visit[at];
    const int32_t l = left[i], r = right[i];
    uint32_t h = 0;
    if (l >= 0) h = s.height[l] + 1;
    if (r >= 0 && s.height[r] + 1 > h) h = s.height[r] + 1;
    s.height[i] = h;
    s.min_idx[i] = l >= 0 ? s.min_idx[l] : i;
    s.max_idx[i] = r >= 0 ? s.max_idx[r] : i;
    if (l >= 0) s.parent[l] = (int32_t)i;
    if (r >= 0) s.parent[r] = (int32_t)i;
    if (h > top) top = h;
  }
  s.roots.swap(roots);
  if (n) {
    s.level_off.assign((size_t)top + 2, 0);
    for (uint32_t i = 0; i < n; i++) s.level_off[s.height[i] + 1]++;
    for (uint32_t h = 0; h <= top; h++) s.level_off[h + 1] += s.level_off[h];
    std::vector<uint32_t> fill(s.level_off.begin(), s.level_off.end() - 1);
    s.order.resize(n);
    for (uint32_t i = 0; i < n; i++) s.order[fill[s.height[i]]++] = i;
  }
  return nullptr;
}

// The closure of a set of touched nodes: they and all their ancestors, as the compact level lists the update kernels take.
struct TreeTouched {
  std::vector<uint32_t> nodes;      // grouped by height in the shape's own order: ascending height, ascending node index inside one
  std::vector<uint32_t> level_off;  // [levels + 1]: the nodes of the l-th height that occurs are nodes[level_off[l] .. level_off[l + 1])
  uint32_t widest = 0;              // the largest level
  char err[96] = {0};               // why the last call was refused
  uint32_t levels() const { return (uint32_t)level_off.size() - 1; }
};
// nullptr, or why the list is refused (out.err: an index >= n, named; nothing out of bounds is read, and out is then empty).
// Duplicates collapse; k = 0 gives the empty closure (no level). Heights that no closure node has make no level.
inline const char* tree_shape_touched(const TreeShape& s, const uint32_t* touched, size_t k, TreeTouched& out) {
  out.nodes.clear();
  out.level_off.assign(1, 0);
  out.widest = 0;
  out.err[0] = 0;
  const uint32_t n = s.size();
  if (k && !touched) {
    snprintf(out.err, sizeof out.err, "touched list missing");
    return out.err;
  }
  for (size_t j = 0; j < k; j++) {
    const uint32_t t = touched[j];
    if (t >= n) {
      for (uint32_t i : out.nodes) s.mark[i] = 0;
      out.nodes.clear();
      snprintf(out.err, sizeof out.err, "touched index %u is outside the shape's %u nodes", t, n);
      return out.err;
    }
    for (int64_t i = t; i >= 0 && !s.mark[i]; i = s.parent[i]) {  // up to the root or to a lineage already taken
      s.mark[i] = 1;
      out.nodes.push_back((uint32_t)i);
    }
  }
  for (uint32_t i : out.nodes) s.mark[i] = 0;
  std::sort(out.nodes.begin(), out.nodes.end(), [&s](uint32_t a, uint32_t b) {
    return s.height[a] != s.height[b] ? s.height[a] < s.height[b] : a < b;
  });
  for (size_t j = 0; j < out.nodes.size(); j++) {
    if (j && s.height[out.nodes[j]] != s.height[out.nodes[j - 1]]) out.level_off.push_back((uint32_t)j);
  }
  if (!out.nodes.empty()) out.level_off.push_back((uint32_t)out.nodes.size());
  for (uint32_t l = 0; l + 1 < out.level_off.size(); l++) out.widest = std::max(out.widest, out.level_off[l + 1] - out.level_off[l]);
  return nullptr;
}

// ---- ryhope sbbst over positions 1..n (64-bit positions: a saturated child of a position <= 2^32 - 1 fits easily) ----------------------
// sbbst.rs:251-257: the largest power of two <= n; 0 for the empty tree
inline uint64_t sbbst_root(uint64_t n) {
  uint64_t r = 0;
  for (uint64_t b = 1; b && b <= n; b <<= 1) r = b;
  return r;
}
// sbbst.rs:487-503 children_inner_in_saturated: false for a position of layer 0 (a leaf of the saturated tree)
inline bool sbbst_saturated_children(uint64_t k, uint64_t* l, uint64_t* r) {
  const uint64_t low = k & (~k + 1);  // 2^layer
  if (low <= 1) return false;
  *l = k - (low >> 1);
  *r = k + (low >> 1);
  return true;
}
// sbbst.rs:301-333 children_inner: the children of position k in the tree over 1..n; 0 = none. A right child beyond n is replaced
// by its left descendants until one is inside the tree.
inline void sbbst_children(uint64_t n, uint64_t k, uint64_t* left, uint64_t* right) {
  uint64_t l, r;
  *left = *right = 0;
  if (!sbbst_saturated_children(k, &l, &r)) return;
  if (l > n) return;  // then r > n too, and everything under it
  *left = l;
  while (r > n) {
    uint64_t rl, rr;
    if (!sbbst_saturated_children(r, &rl, &rr)) return;
    r = rl;
  }
  *right = r;
}
// left / right [n] of the sbbst over n positions, position k = node k - 1
inline void sbbst_fill(uint32_t n, int32_t* left, int32_t* right) {
  for (uint32_t k = 1; k <= n; k++) {
    uint64_t l, r;
    sbbst_children(n, k, &l, &r);
    left[k - 1] = l ? (int32_t)(l - 1) : -1;
    right[k - 1] = r ? (int32_t)(r - 1) : -1;
  }
}
}  // namespace mp2g
