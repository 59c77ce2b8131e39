// C ABI of the MPT subtree digests (include/mp2g.h) over the kernels of mpt_digest.hip. Every argument is judged on the host before
// anything is uploaded or launched; a rejected proof and a conflict are outputs, not refusals.
#include "mpt_args.h"
#include "mpt.h"
#include "mpt_digest.h"

using namespace mp2g;

static const size_t PT_BYTES = 20 * sizeof(u64);

static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}
// the context's working block, grown when a call needs more
static int graph_work(mp2g_ctx* c, size_t bytes) {
  if (c->mpt_work.bytes < bytes) {
    CK(hipStreamSynchronize(c->stream));  // a kernel queued earlier may still use the old block
    CK(c->mpt_work.alloc(bytes));
  }
  return 0;
}
// no proof: every node is UNREACHED. Fills, not kernels. The neutral point is pt_neutral() = (X : Z : U : T) = (0 : 1 : 0 : 1) as
// pt_store lays a point out (ec_curve.cuh: X in words 0-4, Z in 5-9, U in 10-14, T in 15-19, coefficient 0 first): the value 1 in
// words 5 and 15, that is their low byte set, and every other byte 0. Whoever changes pt_store's layout changes this with it; the
// "no proof" case of tests/test_gpu_mpt_digests.py reads these points back through mp2g_curve_emit_dev.
static int fill_unreached(mp2g_ctx* c, uint32_t n_nodes, uint64_t* d_acc, uint32_t* d_n_leaves, uint32_t* d_state, uint32_t* d_via,
                          uint32_t* d_parent, uint8_t* d_entered) {
  const size_t n = n_nodes;
  if (d_acc) {
    CK(hipMemsetAsync(d_acc, 0, n * PT_BYTES, c->stream));
    CK(hipMemset2DAsync(d_acc + 5, PT_BYTES, 1, 1, n, c->stream));
    CK(hipMemset2DAsync(d_acc + 15, PT_BYTES, 1, 1, n, c->stream));
  }
  if (d_n_leaves) CK(hipMemsetAsync(d_n_leaves, 0, n * sizeof(u32), c->stream));
  if (d_state) CK(hipMemsetAsync(d_state, 0, n * sizeof(u32), c->stream));
  if (d_via) CK(hipMemsetAsync(d_via, 0xff, n * sizeof(u32), c->stream));
  if (d_parent) CK(hipMemsetAsync(d_parent, 0xff, n * sizeof(u32), c->stream));
  if (d_entered) CK(hipMemsetAsync(d_entered, 0xff, n, c->stream));
  return 0;
}

extern "C" {

int mp2g_mpt_subtree_digests_dev(mp2g_ctx* c, const uint32_t* d_info, uint32_t n_nodes, const uint32_t* d_paths, const uint32_t* d_depths,
                                 uint32_t max_depth, const uint8_t* d_mpt_keys, const uint32_t* d_status, uint32_t count,
                                 const uint64_t* d_leaf_frac, uint64_t* d_acc_frac, uint32_t* d_n_leaves, uint32_t* d_state, uint32_t* d_via,
                                 uint32_t* d_parent, uint8_t* d_entered, uint32_t totals[3]) {
  NEED(d_info || !n_nodes, "info");
  if (count) {
    NEED(d_paths, "paths");
    NEED(d_depths, "depths");
    NEED(d_mpt_keys, "mpt_keys");
    NEED(d_leaf_frac || !d_acc_frac || !n_nodes, "leaf_frac");
  }
  int rc = max_depth_arg(max_depth);
  if (rc || (rc = aligned_arg(d_leaf_frac, 8, "leaf_frac")) || (rc = aligned_arg(d_acc_frac, 8, "acc_frac")) || (rc = aligned_arg(d_info, 4, "info")) ||
      (rc = aligned_arg(d_paths, 4, "paths")) || (rc = aligned_arg(d_depths, 4, "depths")) || (rc = aligned_arg(d_status, 4, "status")) ||
      (rc = aligned_arg(d_n_leaves, 4, "n_leaves")) || (rc = aligned_arg(d_state, 4, "state")) || (rc = aligned_arg(d_via, 4, "via")) ||
      (rc = aligned_arg(d_parent, 4, "parent")))
    return rc;
  if (d_leaf_frac && d_acc_frac && overlap(d_leaf_frac, count * PT_BYTES, d_acc_frac, n_nodes * PT_BYTES))
    return fail("invalid argument: leaf_frac and acc_frac overlap");
  if (!n_nodes) {  // no index is below n_nodes: every proof is rejected
    if (totals) totals[0] = count, totals[1] = totals[2] = 0;
    return 0;
  }
  NEED(c, "ctx");
  if (!count) {
    if (totals) totals[0] = totals[1] = totals[2] = 0;
    return fill_unreached(c, n_nodes, d_acc_frac, d_n_leaves, d_state, d_via, d_parent, d_entered);
  }
  rc = graph_work(c, mpt_graph_work_bytes(n_nodes, count));
  if (rc) return rc;
  const MptGraphWork w = mpt_graph_work(c->mpt_work.p, n_nodes, count);
  u32* n_leaves = d_n_leaves ? d_n_leaves : w.n_leaves;
  CK(mpt_graph_shape(c->stream, w, d_info, n_nodes, d_paths, d_depths, max_depth, d_mpt_keys, d_status, count, (u64*)d_acc_frac, n_leaves, d_state,
                     d_via, d_parent, d_entered));
  u32 ctl[MPT_CTL_HOST_WORDS];
  CK(hipMemcpyAsync(ctl, w.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));  // the one synchronisation: the level counts and the totals
  if (totals) totals[0] = ctl[MPT_CTL_REJECTED], totals[1] = ctl[MPT_CTL_CONFLICT], totals[2] = ctl[MPT_CTL_LEVELS];
  u32 off[MP2G_MPT_MAX_DEPTH + 1] = {0};
  for (u32 lv = 0; lv < MP2G_MPT_MAX_DEPTH; lv++) off[lv + 1] = off[lv] + ctl[MPT_CTL_COUNT + lv];
  if (off[MP2G_MPT_MAX_DEPTH] > n_nodes) return fail("mp2g_mpt_subtree_digests_dev: the level counts do not add up");
  for (u32 lv = MP2G_MPT_MAX_DEPTH; lv-- > 0;)
    CK(mpt_subtree_level(c->stream, w, w.order + off[lv], ctl[MPT_CTL_COUNT + lv], d_info, (const u64*)d_leaf_frac, (u64*)d_acc_frac, n_leaves));
  return 0;
}

int mp2g_mpt_subtree_digests(mp2g_ctx* c, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, uint32_t n_nodes, const uint32_t* paths,
                             const uint32_t* depths, uint32_t max_depth, const uint8_t* mpt_keys, uint32_t count, const uint8_t* roots,
                             uint32_t root_stride, uint32_t mode, const uint64_t* leaf_w, uint32_t* status, uint64_t* out_w, uint64_t* out_wei,
                             uint32_t* n_leaves, uint32_t* state, uint32_t* via, uint32_t* parent, uint8_t* entered, uint32_t totals[3]) {
  int rc = table_args(nodes, stride, lens, n_nodes, true);
  if (rc || (rc = walk_args(paths, depths, max_depth, mpt_keys, root_stride, mode)) || (rc = depths_arg(depths, count, max_depth))) return rc;
  const bool points = (out_w || out_wei) && n_nodes;
  NEED(leaf_w || !points || !count, "leaf_w");
  if (!n_nodes && !count) {
    if (totals) totals[0] = totals[1] = totals[2] = 0;
    return 0;
  }
  NEED(c, "ctx");
  const size_t n = n_nodes, n_roots = root_stride ? count : 1;
  DevBuf dleaf, dnodes, dlens, dhash, dinfo, dpaths, ddepths, dkeys, droots, dstatus, dacc, dnl, dstate, dvia, dparent, dentered;
  if (points && count) {  // first: an encoding that is refused ends the call before anything else has run
    CK(dleaf.alloc(count * PT_BYTES));
    if ((rc = mp2g_curve_decode_dev(c, leaf_w, count, dleaf.p))) return rc;
  }
  if (n_nodes) {
    CK(upload(dnodes, nodes, n * stride, c->stream));
    CK(upload(dlens, lens, n * sizeof(u32), c->stream));
  }
  CK(dhash.alloc((n ? n : 1) * 32));
  CK(dinfo.alloc((n ? n : 1) * sizeof(u32)));
  if (count) {
    CK(upload(dpaths, paths, (size_t)count * max_depth * sizeof(u32), c->stream));
    CK(upload(ddepths, depths, (size_t)count * sizeof(u32), c->stream));
    CK(upload(dkeys, mpt_keys, (size_t)count * 32, c->stream));
    if (roots) CK(upload(droots, roots, n_roots * 32, c->stream));
    CK(dstatus.alloc((size_t)count * sizeof(u32)));
  }
  if (points) CK(dacc.alloc(n * PT_BYTES));
  if (n_leaves && n) CK(dnl.alloc(n * sizeof(u32)));
  if (state && n) CK(dstate.alloc(n * sizeof(u32)));
  if (via && n) CK(dvia.alloc(n * sizeof(u32)));
  if (parent && n) CK(dparent.alloc(n * sizeof(u32)));
  if (entered && n) CK(dentered.alloc(n));
  CK(mpt_open_nodes(c->stream, (const uint8_t*)dnodes.p, stride, (const u32*)dlens.p, n_nodes, (uint8_t*)dhash.p, (u32*)dinfo.p));
  CK(mpt_verify_paths(c->stream, (const uint8_t*)dnodes.p, stride, (const u32*)dlens.p, (const uint8_t*)dhash.p, (const u32*)dinfo.p, n_nodes,
                      (const u32*)dpaths.p, (const u32*)ddepths.p, max_depth, (const uint8_t*)dkeys.p, count, (const uint8_t*)droots.p, root_stride,
                      mode, (u32*)dstatus.p, nullptr, nullptr, nullptr, nullptr, nullptr));
  rc = mp2g_mpt_subtree_digests_dev(c, (const u32*)dinfo.p, n_nodes, (const u32*)dpaths.p, (const u32*)ddepths.p, max_depth, (const uint8_t*)dkeys.p,
                                    (const u32*)dstatus.p, count, dleaf.p, dacc.p, (u32*)dnl.p, (u32*)dstate.p, (u32*)dvia.p, (u32*)dparent.p,
                                    (uint8_t*)dentered.p, totals);
  if (rc) return rc;
  if (status && count) CK(hipMemcpyAsync(status, dstatus.p, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (dnl.p) CK(hipMemcpyAsync(n_leaves, dnl.p, n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (dstate.p) CK(hipMemcpyAsync(state, dstate.p, n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (dvia.p) CK(hipMemcpyAsync(via, dvia.p, n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (dparent.p) CK(hipMemcpyAsync(parent, dparent.p, n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (dentered.p) CK(hipMemcpyAsync(entered, dentered.p, n, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  if (points) return mp2g_curve_emit_dev(c, dacc.p, nullptr, n_nodes, out_w, out_wei);
  return 0;
}

}  // extern "C"
