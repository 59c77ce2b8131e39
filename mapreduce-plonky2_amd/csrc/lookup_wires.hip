// prove()'s set_lookup_wires for a batch of wire matrices on the device ([dep] plonk/prover.rs set_lookup_wires, as
// circuits.fill_lookup_row restates it): per table the unused LookupGate slots get the table's first pair, every table entry's
// multiplicity is the number of LookupGate slots (padding included) that hold the entry's pair, and the LookupTableGate rows get
// (input, output, multiplicity) with the table running down from first_lut_row. A slot whose pair is not in the table counts for
// nothing: that proof fails the lookup argument in prove() (witness-check flag 4), nothing fails here.
//
// One block per (proof, table). The counters live in LDS, LW_WINDOW entries at a time: a table of up to LW_WINDOW entries takes one
// pass over its LookupGate slots, a 65536-entry table eight. Counting is integer addition into the block's own LDS, so the result
// does not depend on the order the lanes arrive in; no two blocks touch the same word of the matrix (a table's rows are its own).
// The matrix is addressed by (column stride, row stride): the same body serves the prover's polynomial-major layout and the
// witness executor's row-major staging, where a LookupGate row is one contiguous run of 80 words.
#include "gl.cuh"
#include "lookup_wires.h"

namespace mp2g {
namespace {
constexpr int LW_LANES = 256;
constexpr u32 LW_WINDOW = 8192;  // 32 KiB of LDS counters

__global__ void __launch_bounds__(LW_LANES) lookup_wires_kernel(const LutIndex L, u64* __restrict__ wires_all, u64 bstride, u64 cs, u64 rs) {
  __shared__ u32 cnt[LW_WINDOW];
  const u32 t = blockIdx.x, tid = threadIdx.x;
  u64* wires = wires_all + (u64)blockIdx.y * bstride;
#define W(col, row) wires[(u64)(col) * cs + (u64)(row) * rs]
  const u16* __restrict__ tab = L.table[t];
  const u32 len = L.table_len[t], n_lookups = L.n_lookups[t], lu_row = L.last_lu_row[t], top = L.first_lut_row[t];
  const u32 n_lu = (L.last_lut_row[t] - lu_row) * L.lu_slots, n_lut = (top - L.last_lut_row[t] + 1) * L.lut_slots;
  const u64 pad_inp = tab[0], pad_out = tab[1];
  for (u32 j = n_lookups + tid; j < n_lu; j += LW_LANES) {
    const u32 row = lu_row + j / L.lu_slots, c = 2 * (j % L.lu_slots);
    W(c, row) = pad_inp;
    W(c + 1, row) = pad_out;
  }
  for (u32 base = 0; base < n_lut; base += LW_WINDOW) {
    for (u32 i = tid; i < LW_WINDOW; i += LW_LANES) cnt[i] = 0;
    __syncthreads();
    if (base < len)
      for (u32 j = tid; j < n_lu; j += LW_LANES) {
        u64 inp = pad_inp, out = pad_out;  // the padding this block wrote above is not read back
        if (j < n_lookups) {
          const u32 row = lu_row + j / L.lu_slots, c = 2 * (j % L.lu_slots);
          inp = W(c, row);
          out = W(c + 1, row);
        }
        const u32 e = lut_entry(L, t, inp, out);
        if (e != LUT_ABSENT && e - base < LW_WINDOW) atomicAdd(&cnt[e - base], 1u);  // e < base wraps past the window
      }
    __syncthreads();
    const u32 end = base + LW_WINDOW < n_lut ? base + LW_WINDOW : n_lut;
    for (u32 e = base + tid; e < end; e += LW_LANES) {
      const u32 row = top - e / L.lut_slots, c = 3 * (e % L.lut_slots);
      const bool in = e < len;
      W(c, row) = in ? tab[2 * e] : 0;
      W(c + 1, row) = in ? tab[2 * e + 1] : 0;
      W(c + 2, row) = in ? cnt[e - base] : 0;
    }
    __syncthreads();
  }
#undef W
}
}  // namespace

hipError_t lookup_wires_launch(hipStream_t s, const LutIndex& L, u64* d_wires, u32 batch, u64 bstride, u64 cs, u64 rs) {
  if (!L.n_luts || !batch) return hipSuccess;
  hipLaunchKernelGGL(lookup_wires_kernel, dim3(L.n_luts, batch), dim3(LW_LANES), 0, s, L, d_wires, bstride, cs, rs);
  return hipGetLastError();
}

void lookup_wires_host(const LutIndex& L, u64* wires, u64 cs, u64 rs) {
#define W(col, row) wires[(u64)(col) * cs + (u64)(row) * rs]
  std::vector<u32> cnt;
  for (u32 t = 0; t < L.n_luts; t++) {
    const u16* tab = L.table[t];
    const u32 len = L.table_len[t], lu_row = L.last_lu_row[t], top = L.first_lut_row[t];
    const u32 n_lu = (L.last_lut_row[t] - lu_row) * L.lu_slots, n_lut = (top - L.last_lut_row[t] + 1) * L.lut_slots;
    cnt.assign(len, 0);
    for (u32 j = 0; j < n_lu; j++) {
      const u32 row = lu_row + j / L.lu_slots, c = 2 * (j % L.lu_slots);
      if (j >= L.n_lookups[t]) { W(c, row) = tab[0]; W(c + 1, row) = tab[1]; }
      const u32 e = lut_entry(L, t, W(c, row), W(c + 1, row));
      if (e != LUT_ABSENT) cnt[e]++;
    }
    for (u32 e = 0; e < n_lut; e++) {
      const u32 row = top - e / L.lut_slots, c = 3 * (e % L.lut_slots);
      W(c, row) = e < len ? tab[2 * e] : 0;
      W(c + 1, row) = e < len ? tab[2 * e + 1] : 0;
      W(c + 2, row) = e < len ? cnt[e] : 0;
    }
  }
#undef W
}
}  // namespace mp2g
