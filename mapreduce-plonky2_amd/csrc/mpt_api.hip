// C ABI of the MPT inclusion-proof entry points (include/mp2g.h) over the kernels of mpt.hip. Every argument is judged on the host
// before anything is uploaded or launched; a refused call writes no output.
#include "mpt_args.h"
#include "mpt.h"

using namespace mp2g;

extern "C" {

int mp2g_mpt_open_nodes_dev(mp2g_ctx* c, const uint8_t* d_nodes, uint32_t stride, const uint32_t* d_lens, uint32_t n_nodes,
                            uint8_t* d_hashes, uint32_t* d_info) {
  int rc = table_args(d_nodes, stride, d_lens, n_nodes, false);
  if (rc) return rc;
  if (!n_nodes) return 0;
  NEED(c, "ctx");
  if ((rc = aligned_arg(d_nodes, 8, "nodes")) || (rc = aligned_arg(d_hashes, 8, "hashes")) || (rc = aligned_arg(d_lens, 4, "lens")) ||
      (rc = aligned_arg(d_info, 4, "info")))
    return rc;
  CK(mpt_open_nodes(c->stream, d_nodes, stride, d_lens, n_nodes, d_hashes, d_info));
  return 0;
}

int mp2g_mpt_open_nodes(mp2g_ctx* c, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, uint32_t n_nodes, uint8_t* hashes,
                        uint32_t* info) {
  int rc = table_args(nodes, stride, lens, n_nodes, true);
  if (rc) return rc;
  if (!n_nodes) return 0;
  NEED(c, "ctx");
  DevBuf dnodes, dlens, dhash, dinfo;
  CK(upload(dnodes, nodes, (size_t)n_nodes * stride, c->stream));
  CK(upload(dlens, lens, (size_t)n_nodes * sizeof(u32), c->stream));
  if (hashes) CK(dhash.alloc((size_t)n_nodes * 32));
  if (info) CK(dinfo.alloc((size_t)n_nodes * sizeof(u32)));
  CK(mpt_open_nodes(c->stream, (const uint8_t*)dnodes.p, stride, (const u32*)dlens.p, n_nodes, (uint8_t*)dhash.p, (u32*)dinfo.p));
  if (hashes) CK(hipMemcpyAsync(hashes, dhash.p, (size_t)n_nodes * 32, hipMemcpyDeviceToHost, c->stream));
  if (info) CK(hipMemcpyAsync(info, dinfo.p, (size_t)n_nodes * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

int mp2g_mpt_verify_paths_dev(mp2g_ctx* c, const uint8_t* d_nodes, uint32_t stride, const uint32_t* d_lens, const uint8_t* d_hashes,
                              const uint32_t* d_info, uint32_t n_nodes, const uint32_t* d_paths, const uint32_t* d_depths,
                              uint32_t max_depth, const uint8_t* d_mpt_keys, uint32_t count, const uint8_t* d_roots, uint32_t root_stride,
                              uint32_t mode, uint32_t* d_status, uint32_t* d_fail_level, uint8_t* d_words, uint32_t* d_val_off,
                              uint32_t* d_val_len, uint8_t* d_consumed) {
  int rc = table_args(d_nodes, stride, d_lens, n_nodes, false);
  if (rc || (rc = walk_args(d_paths, d_depths, max_depth, d_mpt_keys, root_stride, mode))) return rc;
  NEED(d_hashes, "hashes");
  NEED(d_info, "info");
  if (!count) return 0;
  NEED(c, "ctx");
  if ((rc = aligned_arg(d_nodes, 8, "nodes")) || (rc = aligned_arg(d_hashes, 8, "hashes")) || (rc = aligned_arg(d_roots, 8, "roots")) ||
      (rc = aligned_arg(d_words, 8, "words")) || (rc = aligned_arg(d_lens, 4, "lens")) || (rc = aligned_arg(d_info, 4, "info")) ||
      (rc = aligned_arg(d_paths, 4, "paths")) || (rc = aligned_arg(d_depths, 4, "depths")) || (rc = aligned_arg(d_status, 4, "status")) ||
      (rc = aligned_arg(d_fail_level, 4, "fail_level")) || (rc = aligned_arg(d_val_off, 4, "val_off")) || (rc = aligned_arg(d_val_len, 4, "val_len")))
    return rc;
  CK(mpt_verify_paths(c->stream, d_nodes, stride, d_lens, d_hashes, d_info, n_nodes, d_paths, d_depths, max_depth, d_mpt_keys, count, d_roots,
                      root_stride, mode, d_status, d_fail_level, d_words, d_val_off, d_val_len, d_consumed));
  return 0;
}

int mp2g_mpt_verify_paths(mp2g_ctx* c, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, uint32_t n_nodes, const uint32_t* paths,
                          const uint32_t* depths, uint32_t max_depth, const uint8_t* mpt_keys, uint32_t count, const uint8_t* roots,
                          uint32_t root_stride, uint32_t mode, uint32_t* status, uint32_t* fail_level, uint8_t* words, uint32_t* val_off,
                          uint32_t* val_len, uint8_t* consumed) {
  int rc = table_args(nodes, stride, lens, n_nodes, true);
  if (rc || (rc = walk_args(paths, depths, max_depth, mpt_keys, root_stride, mode))) return rc;
  if ((rc = depths_arg(depths, count, max_depth))) return rc;
  if (!count) return 0;
  NEED(c, "ctx");
  const bool word = mode != MP2G_MPT_VALUE_RAW && words;
  const size_t n_roots = root_stride ? count : 1;
  DevBuf dnodes, dlens, dhash, dinfo, dpaths, ddepths, dkeys, droots, dstatus, dlevel, dwords, dvoff, dvlen, dcons;
  if (n_nodes) {
    CK(upload(dnodes, nodes, (size_t)n_nodes * stride, c->stream));
    CK(upload(dlens, lens, (size_t)n_nodes * sizeof(u32), c->stream));
  }
  CK(dhash.alloc((size_t)(n_nodes ? n_nodes : 1) * 32));
  CK(dinfo.alloc((size_t)(n_nodes ? n_nodes : 1) * sizeof(u32)));
  CK(upload(dpaths, paths, (size_t)count * max_depth * sizeof(u32), c->stream));
  CK(upload(ddepths, depths, (size_t)count * sizeof(u32), c->stream));
  CK(upload(dkeys, mpt_keys, (size_t)count * 32, c->stream));
  if (roots) CK(upload(droots, roots, n_roots * 32, c->stream));
  if (status) CK(dstatus.alloc((size_t)count * sizeof(u32)));
  if (fail_level) CK(dlevel.alloc((size_t)count * sizeof(u32)));
  if (word) CK(dwords.alloc((size_t)count * 32));
  if (val_off) CK(dvoff.alloc((size_t)count * sizeof(u32)));
  if (val_len) CK(dvlen.alloc((size_t)count * sizeof(u32)));
  if (consumed) CK(dcons.alloc((size_t)count * max_depth));
  CK(mpt_open_nodes(c->stream, (const uint8_t*)dnodes.p, stride, (const u32*)dlens.p, n_nodes, (uint8_t*)dhash.p, (u32*)dinfo.p));
  CK(mpt_verify_paths(c->stream, (const uint8_t*)dnodes.p, stride, (const u32*)dlens.p, (const uint8_t*)dhash.p, (const u32*)dinfo.p, n_nodes,
                      (const u32*)dpaths.p, (const u32*)ddepths.p, max_depth, (const uint8_t*)dkeys.p, count, (const uint8_t*)droots.p,
                      root_stride, mode, (u32*)dstatus.p, (u32*)dlevel.p, (uint8_t*)dwords.p, (u32*)dvoff.p, (u32*)dvlen.p,
                      (uint8_t*)dcons.p));
  if (status) CK(hipMemcpyAsync(status, dstatus.p, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (fail_level) CK(hipMemcpyAsync(fail_level, dlevel.p, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (word) CK(hipMemcpyAsync(words, dwords.p, (size_t)count * 32, hipMemcpyDeviceToHost, c->stream));
  if (val_off) CK(hipMemcpyAsync(val_off, dvoff.p, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (val_len) CK(hipMemcpyAsync(val_len, dvlen.p, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (consumed) CK(hipMemcpyAsync(consumed, dcons.p, (size_t)count * max_depth, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
