// Internal entry points of the batched verifier (verifier.hip) for the other translation units.
#pragma once
#include "ctx.h"
namespace mp2g {
mp2g_ctx* verifier_ctx(const mp2g_verifier* v);
uint32_t verifier_capacity(const mp2g_verifier* v);
// verify `count` proofs that lie anywhere on the verifier's device, each as proof_words contiguous words in a parent's input
// order (a forest's pool slots): gathered by device copies into the verifier's staging buffer, then verified there
int verifier_verify_gathered(mp2g_verifier* v, const u64* const* d_srcs, uint32_t count, uint32_t* status);
}  // namespace mp2g
