// C ABI of the Keccak-256 entry points (include/mp2g.h) over the kernels of storage.hip. Every argument is judged on the host
// before anything is uploaded or launched; a refused call writes no output.
#include "keccak_args.h"

using namespace mp2g;

// everything mp2g_storage_slot_keys[_dev] refuses but its pointers to the leaves
static int slot_args(uint64_t slot, bool parents, uint32_t n_keys) {
  if (n_keys > MP2G_LEAF_MAX_KEYS)
    return fail("invalid argument: n_keys %u is above %d (chain two calls through parents)", n_keys, MP2G_LEAF_MAX_KEYS);
  if (n_keys && !parents && slot > 255)
    return fail("invalid argument: slot %llu of a mapping is above 255 (the reference writes it as one byte)", (unsigned long long)slot);
  return 0;
}

extern "C" {

int mp2g_keccak256_batch_dev(mp2g_ctx* c, const uint8_t* d_msgs, uint32_t stride, const uint32_t* d_lens, uint32_t len, uint32_t count,
                             uint8_t* d_out) {
  int rc = stride_arg(stride);
  if (rc) return rc;
  if (!d_lens && len > stride) return fail("invalid argument: len %u is above the stride %u", len, stride);
  if (!count) return 0;
  NEED(c, "ctx");
  NEED(d_msgs, "msgs");
  NEED(d_out, "out");
  if ((rc = aligned8(d_msgs, "msgs")) || (rc = aligned8(d_out, "out"))) return rc;
  if (d_lens && ((uintptr_t)d_lens & 3)) return fail("invalid argument: lens is not 4-byte aligned");
  CK(keccak256_batch(c->stream, d_msgs, stride, d_lens, len, count, d_out));
  return 0;
}

int mp2g_keccak256_batch(mp2g_ctx* c, const uint8_t* msgs, uint32_t stride, const uint32_t* lens, uint32_t len, uint32_t count,
                         uint8_t* out) {
  int rc = stride_arg(stride);
  if (rc) return rc;
  if (!lens && len > stride) return fail("invalid argument: len %u is above the stride %u", len, stride);
  if (!count) return 0;
  NEED(c, "ctx");
  NEED(msgs, "msgs");
  NEED(out, "out");
  if (lens && (rc = lens_arg(lens, count, stride))) return rc;
  DevBuf dmsgs, dlens, dout;
  CK(upload(dmsgs, msgs, (size_t)count * stride, c->stream));
  if (lens) CK(upload(dlens, lens, (size_t)count * sizeof(u32), c->stream));
  CK(dout.alloc((size_t)count * 32));
  CK(keccak256_batch(c->stream, (const uint8_t*)dmsgs.p, stride, lens ? (const u32*)dlens.p : nullptr, len, count, (uint8_t*)dout.p));
  CK(hipMemcpyAsync(out, dout.p, (size_t)count * 32, hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

int mp2g_storage_slot_keys_dev(mp2g_ctx* c, uint64_t slot, const uint8_t* d_parents, const uint8_t* d_keys, uint32_t n_keys,
                               uint32_t evm_offset, uint32_t count, uint8_t* d_locations, uint8_t* d_mpt_keys, uint8_t* d_nibbles,
                               uint32_t* n_overflow) {
  int rc = slot_args(slot, d_parents != nullptr, n_keys);
  if (rc) return rc;
  if (!count) {
    if (n_overflow) *n_overflow = 0;
    return 0;
  }
  NEED(c, "ctx");
  NEED(d_keys || !n_keys, "keys");
  if ((rc = aligned8(d_parents, "parents")) || (rc = aligned8(d_keys, "keys")) || (rc = aligned8(d_locations, "locations")) ||
      (rc = aligned8(d_mpt_keys, "mpt_keys")) || (rc = aligned8(d_nibbles, "nibbles")))
    return rc;
  DevBuf dover;
  if (n_overflow) CK(dover.alloc(sizeof(u32)));
  CK(storage_slot_keys(c->stream, slot, d_parents, d_keys, n_keys, evm_offset, count, d_locations, d_mpt_keys, d_nibbles,
                       n_overflow ? (u32*)dover.p : nullptr));
  if (n_overflow) {  // the one synchronisation a host output costs
    uint32_t over = 0;
    CK(hipMemcpyAsync(&over, dover.p, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    CK(hipStreamSynchronize(c->stream));
    *n_overflow = over;
  }
  return 0;
}

int mp2g_storage_slot_keys(mp2g_ctx* c, uint64_t slot, const uint8_t* parents, const uint8_t* keys, uint32_t n_keys, uint32_t evm_offset,
                           uint32_t count, uint8_t* locations, uint8_t* mpt_keys, uint8_t* nibbles, uint32_t* n_overflow) {
  int rc = slot_args(slot, parents != nullptr, n_keys);
  if (rc) return rc;
  if (!count) {
    if (n_overflow) *n_overflow = 0;
    return 0;
  }
  NEED(c, "ctx");
  NEED(keys || !n_keys, "keys");
  DevBuf dparents, dkeys, dloc, dkey, dnib, dover;
  if (parents) CK(upload(dparents, parents, (size_t)count * 32, c->stream));
  if (n_keys) CK(upload(dkeys, keys, (size_t)count * n_keys * 32, c->stream));
  if (locations) CK(dloc.alloc((size_t)count * 32));
  if (mpt_keys) CK(dkey.alloc((size_t)count * 32));
  if (nibbles) CK(dnib.alloc((size_t)count * 64));
  CK(dover.alloc(sizeof(u32)));
  CK(storage_slot_keys(c->stream, slot, (const uint8_t*)dparents.p, (const uint8_t*)dkeys.p, n_keys, evm_offset, count, (uint8_t*)dloc.p,
                       (uint8_t*)dkey.p, (uint8_t*)dnib.p, (u32*)dover.p));
  uint32_t over = 0;
  if (locations) CK(hipMemcpyAsync(locations, dloc.p, (size_t)count * 32, hipMemcpyDeviceToHost, c->stream));
  if (mpt_keys) CK(hipMemcpyAsync(mpt_keys, dkey.p, (size_t)count * 32, hipMemcpyDeviceToHost, c->stream));
  if (nibbles) CK(hipMemcpyAsync(nibbles, dnib.p, (size_t)count * 64, hipMemcpyDeviceToHost, c->stream));
  CK(hipMemcpyAsync(&over, dover.p, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  if (n_overflow) *n_overflow = over;
  return 0;
}

int mp2g_mpt_storage_leaves_dev(mp2g_ctx* c, const uint8_t* d_nodes, uint32_t stride, const uint32_t* d_lens, const uint8_t* d_mpt_keys,
                                uint32_t count, uint8_t* d_hashes, uint8_t* d_words, uint32_t* d_n_nibbles, uint32_t* d_status) {
  int rc = stride_arg(stride);
  if (rc) return rc;
  if (!count) return 0;
  NEED(c, "ctx");
  NEED(d_nodes, "nodes");
  NEED(d_lens, "lens");
  if ((rc = aligned8(d_nodes, "nodes")) || (rc = aligned8(d_hashes, "hashes")) || (rc = aligned8(d_words, "words"))) return rc;
  if (((uintptr_t)d_lens | (uintptr_t)d_n_nibbles | (uintptr_t)d_status) & 3)
    return fail("invalid argument: lens, n_nibbles or status is not 4-byte aligned");
  CK(mpt_storage_leaves(c->stream, d_nodes, stride, d_lens, d_mpt_keys, count, d_hashes, d_words, d_n_nibbles, d_status));
  return 0;
}

int mp2g_mpt_storage_leaves(mp2g_ctx* c, const uint8_t* nodes, uint32_t stride, const uint32_t* lens, const uint8_t* mpt_keys,
                            uint32_t count, uint8_t* hashes, uint8_t* words, uint32_t* n_nibbles, uint32_t* status) {
  int rc = stride_arg(stride);
  if (rc) return rc;
  if (!count) return 0;
  NEED(c, "ctx");
  NEED(nodes, "nodes");
  NEED(lens, "lens");
  if ((rc = lens_arg(lens, count, stride))) return rc;
  DevBuf dnodes, dlens, dkeys, dhash, dwords, dnib, dstatus;
  CK(upload(dnodes, nodes, (size_t)count * stride, c->stream));
  CK(upload(dlens, lens, (size_t)count * sizeof(u32), c->stream));
  if (mpt_keys) CK(upload(dkeys, mpt_keys, (size_t)count * 32, c->stream));
  if (hashes) CK(dhash.alloc((size_t)count * 32));
  if (words) CK(dwords.alloc((size_t)count * 32));
  if (n_nibbles) CK(dnib.alloc((size_t)count * sizeof(u32)));
  if (status) CK(dstatus.alloc((size_t)count * sizeof(u32)));
  CK(mpt_storage_leaves(c->stream, (const uint8_t*)dnodes.p, stride, (const u32*)dlens.p, (const uint8_t*)dkeys.p, count, (uint8_t*)dhash.p,
                        (uint8_t*)dwords.p, (u32*)dnib.p, (u32*)dstatus.p));
  if (hashes) CK(hipMemcpyAsync(hashes, dhash.p, (size_t)count * 32, hipMemcpyDeviceToHost, c->stream));
  if (words) CK(hipMemcpyAsync(words, dwords.p, (size_t)count * 32, hipMemcpyDeviceToHost, c->stream));
  if (n_nibbles) CK(hipMemcpyAsync(n_nibbles, dnib.p, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (status) CK(hipMemcpyAsync(status, dstatus.p, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  CK(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
