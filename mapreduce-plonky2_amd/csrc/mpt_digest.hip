// MPT subtree digests on the device, for gfx950: DV and N of every node of a storage trie (mpt_graph.cuh names what of the
// reference this replaces), from what mp2g_mpt_verify_paths and mp2g_leaf_values_digests leave on the device.
//
// The shape comes first. Four launches of one lane per proof walk the path rows again (the dependent loads of stage 2 without
// the node bytes: an index, then its info word): minima (each node's lowest proof and level, each (parent, nibble)'s lowest child),
// the owner of every node writes its tuple, every occurrence is compared with it, and conflicts are carried up the proofs. Every
// accepted proof meets the root's words; a wave sends them one atomic, not 64, and none once the stored value is as low as its own
// (MptAtomic below), so the root costs a few thousand atomics, not 2^20.
// Then one lane per node: the outputs, the neutral point of what is not OK, and the OK nodes counted and ranked per level with
// one atomic per wave and level; one lane turns the counts into offsets; the nodes go to their places. All of that is queued
// without the host; the host then reads 69 words and launches one level after the other, the deepest first.
//
// The level kernel is digest_level_kernel's shape (tree_digest.hip): one lane per node, 128 lanes, children by index from what an
// earlier launch wrote, pt_add out of line. A branch loops over its 16 child words in memory: no private array is indexed.
#include "mpt_digest.h"
#include "mpt_graph.cuh"
#include "poseidon.cuh"
#include "gl5.cuh"
#include "ec_curve.cuh"

namespace mp2g {

// Two ways of sparing a shared word its atomics, both taken (profiles/mpt_digests.md has what each cost):
// 1. The wave first. Every accepted proof meets the root's words, and half a million lanes are in flight before the first atomic
//    has landed, so looking at the word alone spares little. The first active lane of the wave speaks for every other lane that
//    aims at the same word with a value that cannot improve on its own: proofs lie in the lanes in ascending order, so near the
//    root that is the whole wave. __builtin_amdgcn_readfirstlane reads the first ACTIVE lane, so this holds inside the walk's
//    divergent loop, where the lanes of a wave are at the same level together.
// 2. Then load, and skip the atomic when the stored value is already as good. The load is a plain one while other workgroups
//    update the word atomically in the same launch, so it may return an old value (a line still in the vector cache). That is
//    safe: a word under min only falls and a word under or only gains bits, so an old value can only fail to justify the skip,
//    and the lane then sends an atomic that changes nothing. The atomic, not the load, decides what is stored. (A relaxed atomic
//    load at device scope in its place was measured and was slower.)
GLD u32 mpt_first(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
GLD u64 mpt_first(u64 v) { return (u64)mpt_first((u32)v) | (u64)mpt_first((u32)(v >> 32)) << 32; }
// the leader's (word, value) when another lane leads this one's word, else this lane's own
template <class T>
GLD bool mpt_led(const T* p, T v, T* lead) {
  const u32 lane = __lane_id();
  *lead = mpt_first(v);
  const bool same_word = mpt_first((u64)p) == (u64)p, another = mpt_first(lane) != lane;  // both read by every active lane
  return same_word && another;
}
struct MptAtomic {
  GLD static void min64(u64* p, u64 v) {
    u64 lead;
    if (mpt_led(p, v, &lead) && lead <= v) return;
    if (*p <= v) return;
    atomicMin((unsigned long long*)p, (unsigned long long)v);
  }
  GLD static void min32(u32* p, u32 v) {
    u32 lead;
    if (mpt_led(p, v, &lead) && lead <= v) return;
    if (*p <= v) return;
    atomicMin(p, v);
  }
  GLD static void or32(u32* p, u32 v) {
    u32 lead;
    if (mpt_led(p, v, &lead) && (lead & v) == v) return;
    if ((*p & v) == v) return;
    atomicOr(p, v);
  }
};

struct CurvePoints {
  using point = pt;
  GLD static pt neutral() { return pt_neutral(); }
  GLD static pt load(const u64* d) { return pt_load(d); }
  GLD static pt add(const pt& a, const pt& b) { return pt_add(a, b); }
  GLD static void store(u64* d, const pt& p) { pt_store(d, p); }
};

// what every pass over the proofs is given
struct MptProofs {
  const u32* info;
  const u32* paths;
  const u32* depths;
  const uint8_t* keys;
  const u32* status;
  u32 n_nodes, max_depth, count;
};

__global__ void __launch_bounds__(128) mpt_graph_minima_kernel(MptProofs p, MptGraphWork w) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  bool rejected = false;
  if (i < p.count) {
    const bool ok = mpt_graph_minima<MptAtomic>(p.info, p.n_nodes, p.paths + i * p.max_depth, p.depths[i], p.max_depth, p.keys + 32 * i, p.status,
                                                (u32)i, w.ref, w.child);
    w.accepted[i] = ok;
    rejected = !ok;
  }
  const u64 votes = __ballot(rejected);  // every lane of the wave is here: none has returned
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(w.ctl + MPT_CTL_REJECTED, (u32)__popcll(votes));
}

__global__ void __launch_bounds__(128) mpt_graph_own_kernel(MptProofs p, MptGraphWork w) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.count || !w.accepted[i]) return;
  mpt_graph_own(p.info, p.paths + i * p.max_depth, p.depths[i], p.keys + 32 * i, (u32)i, w.ref, w.parent, w.les);
}

__global__ void __launch_bounds__(128) mpt_graph_compare_kernel(MptProofs p, MptGraphWork w) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.count || !w.accepted[i]) return;
  mpt_graph_compare<MptAtomic>(p.info, p.paths + i * p.max_depth, p.depths[i], p.keys + 32 * i, w.parent, w.les, w.child, w.direct);
}

__global__ void __launch_bounds__(128) mpt_graph_above_kernel(MptProofs p, MptGraphWork w) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.count || !w.accepted[i]) return;
  mpt_graph_above<MptAtomic>(p.paths + i * p.max_depth, p.depths[i], w.direct, w.above);
}

// One lane per node: the shape outputs, the values of a node that is not OK, and the node's rank among the OK nodes of its level.
// The lanes of a wave that share a level send one atomic between them.
__global__ void __launch_bounds__(128) mpt_graph_nodes_kernel(MptGraphWork w, u32 n_nodes, u64* __restrict__ acc, u32* __restrict__ n_leaves,
                                                              u32* __restrict__ state, u32* __restrict__ via, u32* __restrict__ parent,
                                                              uint8_t* __restrict__ entered) {
  const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  bool reached = false, ok = false;
  u32 level = 0;
  if (x < n_nodes) {
    const MptNodeShape s = mpt_graph_node((u32)x, w.ref, w.parent, w.les, w.direct, w.above);
    reached = s.state != MP2G_MPT_SUBTREE_UNREACHED;
    ok = s.state == MP2G_MPT_SUBTREE_OK;
    level = s.level;
    if (state) state[x] = s.state;
    if (via) via[x] = s.via;
    if (parent) parent[x] = s.parent;
    if (entered) entered[x] = (uint8_t)s.entered;
    if (!ok) {
      n_leaves[x] = 0;
      if (acc) pt_store(acc + 20 * x, pt_neutral());
    }
  }
  const u64 conflicts = __ballot(reached && !ok);
  if (lane == 0 && conflicts) atomicAdd(w.ctl + MPT_CTL_CONFLICT, (u32)__popcll(conflicts));
  u64 todo = __ballot(reached);  // uniform over the wave, as is everything the loop branches on
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const u32 lv = __shfl(level, leader);
    const u64 same = __ballot(reached && level == lv), same_ok = __ballot(ok && level == lv);
    u32 base = 0;
    if ((int)lane == leader) {
      if (same_ok) base = atomicAdd(w.ctl + MPT_CTL_COUNT + lv, (u32)__popcll(same_ok));
      if (w.ctl[MPT_CTL_LEVELS] < lv + 1) atomicMax(w.ctl + MPT_CTL_LEVELS, lv + 1);
    }
    base = __shfl(base, leader);
    if (ok && level == lv) w.rank[x] = base + (u32)__popcll(same_ok & ((1ull << lane) - 1));
    todo &= ~same;
  }
}

// one lane: where each level's list starts
__global__ void mpt_graph_offsets_kernel(u32* __restrict__ ctl) {
  u32 off = 0;
  for (u32 lv = 0; lv < MP2G_MPT_MAX_DEPTH; lv++) {
    ctl[MPT_CTL_OFF + lv] = off;
    off += ctl[MPT_CTL_COUNT + lv];
  }
  ctl[MPT_CTL_OFF + MP2G_MPT_MAX_DEPTH] = off;
}

__global__ void __launch_bounds__(128) mpt_graph_order_kernel(MptGraphWork w, u32 n_nodes) {
  const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_nodes) return;
  const MptNodeShape s = mpt_graph_node((u32)x, w.ref, w.parent, w.les, w.direct, w.above);
  if (s.state == MP2G_MPT_SUBTREE_OK) w.order[w.ctl[MPT_CTL_OFF + s.level] + w.rank[x]] = (u32)x;
}

__global__ void __launch_bounds__(128) mpt_subtree_level_kernel(const u32* __restrict__ order, u32 count, const u32* __restrict__ info,
                                                                const u32* __restrict__ child, const u64* __restrict__ ref,
                                                                const u64* __restrict__ leaf_frac, u64* acc, u32* n_leaves) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  mpt_graph_sum<CurvePoints>(order[t], info, child, ref, leaf_frac, acc, n_leaves);
}

// ---- the working block and the launchers ------------------------------------------------------------------------------------------
static inline size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }
size_t mpt_graph_work_bytes(u32 n_nodes, u32 count) {
  // ctl; ref 8; child 64; direct, above, parent, les, rank, order, n_leaves 4 each; accepted 1 per proof
  return up8(MPT_CTL_WORDS * sizeof(u32)) + (size_t)n_nodes * (8 + 64) + up8((size_t)n_nodes * 7 * sizeof(u32)) + up8(count);
}
MptGraphWork mpt_graph_work(void* block, u32 n_nodes, u32 count) {
  MptGraphWork w;
  uint8_t* b = (uint8_t*)block;
  const size_t n = n_nodes;
  w.ctl = (u32*)b; b += up8(MPT_CTL_WORDS * sizeof(u32));
  w.ref = (u64*)b; b += n * 8;      // ref and child lie together: one fill with 0xff
  w.child = (u32*)b; b += n * 64;
  w.direct = (u32*)b;               // direct and above lie together: one fill with 0
  w.above = w.direct + n;
  w.parent = w.above + n;
  w.les = w.parent + n;
  w.rank = w.les + n;
  w.order = w.rank + n;
  w.n_leaves = w.order + n;
  b += up8(n * 7 * sizeof(u32));
  w.accepted = b;
  (void)count;
  return w;
}

static inline dim3 g128(u32 n) { return dim3((n + 127) / 128); }

hipError_t mpt_graph_shape(hipStream_t st, const MptGraphWork& w, const u32* info, u32 n_nodes, const u32* paths, const u32* depths, u32 max_depth,
                           const uint8_t* mpt_keys, const u32* status, u32 count, u64* acc, u32* n_leaves, u32* state, u32* via, u32* parent,
                           uint8_t* entered) {
  if (!n_nodes || !count || !max_depth || max_depth > MP2G_MPT_MAX_DEPTH || !n_leaves) return hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(w.ctl, 0, MPT_CTL_WORDS * sizeof(u32), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.ref, 0xff, (size_t)n_nodes * (8 + 64), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.direct, 0, (size_t)n_nodes * 2 * sizeof(u32), st)) != hipSuccess) return e;
  const MptProofs p = {info, paths, depths, mpt_keys, status, n_nodes, max_depth, count};
  hipLaunchKernelGGL(mpt_graph_minima_kernel, g128(count), dim3(128), 0, st, p, w);
  hipLaunchKernelGGL(mpt_graph_own_kernel, g128(count), dim3(128), 0, st, p, w);
  hipLaunchKernelGGL(mpt_graph_compare_kernel, g128(count), dim3(128), 0, st, p, w);
  hipLaunchKernelGGL(mpt_graph_above_kernel, g128(count), dim3(128), 0, st, p, w);
  hipLaunchKernelGGL(mpt_graph_nodes_kernel, g128(n_nodes), dim3(128), 0, st, w, n_nodes, acc, n_leaves, state, via, parent, entered);
  hipLaunchKernelGGL(mpt_graph_offsets_kernel, dim3(1), dim3(1), 0, st, w.ctl);
  hipLaunchKernelGGL(mpt_graph_order_kernel, g128(n_nodes), dim3(128), 0, st, w, n_nodes);
  return hipGetLastError();
}

hipError_t mpt_subtree_level(hipStream_t st, const MptGraphWork& w, const u32* order, u32 count, const u32* info, const u64* leaf_frac, u64* acc,
                             u32* n_leaves) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(mpt_subtree_level_kernel, g128(count), dim3(128), 0, st, order, count, info, w.child, w.ref, leaf_frac, acc, n_leaves);
  return hipGetLastError();
}
}  // namespace mp2g
