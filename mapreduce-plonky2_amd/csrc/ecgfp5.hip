// Batched Ecgfp5 arithmetic for the off-circuit multiset digest, for gfx950.
//
// Replaces, on the value (non-circuit) side:
//   mp2-common/src/group_hashing/field_to_curve.rs:36-48   map_to_curve_point
//   mp2-common/src/group_hashing/sswu_value.rs:31-77       simple_swu (same operation order)
//   mp2-common/src/group_hashing/utils.rs:9-82             SWU constants
//   mp2-common/src/group_hashing/curve_add.rs:17-33        add_curve_point
//   mp2-common/src/group_hashing/mod.rs:163-174,220-225    Weierstrass limbs, field_hashed_scalar_mul
//   mp2-common/src/poseidon.rs:120-133                     hash_to_int_value
//   mp2-v1/src/values_extraction/mod.rs:499-571            row_unique_data / compute_row_id /
//                                                          compute_table_row_digest
//   verifiable-db/src/cells_tree/mod.rs:65-72              Cell::values_digest
// and [dep] plonky2_ecgfp5 curve/curve.rs (Point decode / encode / add / double / scalar mul); the GF(p^5) field (sqrt /
// inverse / sgn0 / legendre) is gl5.cuh.
//
// ALU-bound: one lane owns one point in fractional coordinates (X:Z:U:T), x = X/Z, u = U/T,
// using the complete 10M addition and 4M+5S doubling of the ecgfp5 paper (checked against the
// affine chord/tangent law of the oracle). GF(p^5) products accumulate the five partial products of an
// output limb in carry-free 64-bit columns (gl_cols) and reduce once. Encodings are canonical, so results are identical
// to the reference's regardless of the coordinate system.
#include "ecgfp5.h"
#include "poseidon.cuh"
#include "gl5.cuh"
#include "ec_curve.cuh"

namespace mp2g {

// ---- kernels ----------------------------------------------------------------------------------
// The heavy kernels declare the 128 lanes they are launched with; the bound reaches the out-of-line bodies too, and larger bounds
// (fewer VGPRs, more waves) were measured slower.
template <int V>
__global__ void __launch_bounds__(128) map_to_curve_kernel(const u64* in, u32 in_len, u32 count, u64* w_out, u64* wei_out, u64* frac_out) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  pt p = map_to_curve<V>(in + (u64)i * in_len, in_len);
  pt_emit(p, w_out ? w_out + 5 * (u64)i : nullptr, wei_out ? wei_out + 11 * (u64)i : nullptr);
  if (frac_out) pt_store(frac_out + 20 * (u64)i, p);
}
// decode encodings into fractional points; bad[0] is set when an encoding is invalid
__global__ void __launch_bounds__(128) decode_kernel(const u64* w_in, u32 count, u64* frac_out, u32* bad) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  gl5 w;
  for (int k = 0; k < 5; k++) w.c[k] = w_in[5 * (u64)i + k];
  pt p;
  if (!pt_decode(w, p)) atomicOr(bad, 1u);
  pt_store(frac_out + 20 * (u64)i, p);
}
// out[blockIdx] = sum of a strided subset of pts[0..count): lanes accumulate serially, then a
// tree over the block through LDS
__global__ void __launch_bounds__(128) sum_kernel(const u64* pts, u32 count, u64* out) {
  __shared__ u64 sm[128 * 20];
  const u32 t = threadIdx.x, stride = gridDim.x * blockDim.x;
  pt acc = pt_neutral();
  for (u32 i = blockIdx.x * blockDim.x + t; i < count; i += stride) acc = pt_add(acc, pt_load(pts + 20 * (u64)i));
  pt_store(sm + 20 * t, acc);
  __syncthreads();
#pragma unroll 1
  for (u32 s = 64; s > 0; s >>= 1) {
    if (t < s) {
      pt a = pt_load(sm + 20 * t), b = pt_load(sm + 20 * (t + s));
      pt_store(sm + 20 * t, pt_add(a, b));
    }
    __syncthreads();
  }
  if (t < 20) out[20 * (u64)blockIdx.x + t] = sm[t];
}
// out[blockIdx] = sum of pts[ranges[blockIdx][0] .. ranges[blockIdx][1]): one 64-lane block per range (a subtree of a tree laid out in
// order is one contiguous range), lanes stride through the range, then a tree over the wave through LDS
__global__ void __launch_bounds__(64) sum_ranges_kernel(const u64* pts, const u32* ranges, u64* out) {
  __shared__ u64 sm[64 * 20];
  const u32 t = threadIdx.x, lo = ranges[2 * blockIdx.x], hi = ranges[2 * blockIdx.x + 1];
  pt acc = pt_neutral();
  for (u32 i = lo + t; i < hi; i += 64) acc = pt_add(acc, pt_load(pts + 20 * (u64)i));
  pt_store(sm + 20 * t, acc);
  __syncthreads();
#pragma unroll 1
  for (u32 s = 32; s > 0; s >>= 1) {
    if (t < s && lo + t + s < hi) {  // lanes past the range hold the neutral point
      pt a = pt_load(sm + 20 * t), b = pt_load(sm + 20 * (t + s));
      pt_store(sm + 20 * t, pt_add(a, b));
    }
    __syncthreads();
  }
  if (t < 20) out[20 * (u64)blockIdx.x + t] = sm[t];
}
__global__ void emit_kernel(const u64* frac, u32 count, u64* w_out, u64* wei_out) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  pt p = pt_load(frac + 20 * (u64)i);
  pt_emit(p, w_out ? w_out + 5 * (u64)i : nullptr, wei_out ? wei_out + 11 * (u64)i : nullptr);
}
__global__ void __launch_bounds__(128) scalar_mul_kernel(const u64* frac_in, const u32* scalars, u32 count, u64* frac_out) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  u32 k[4];
  for (int j = 0; j < 4; j++) k[j] = scalars[4 * (u64)i + j];
  pt_store(frac_out + 20 * (u64)i, pt_mul128(pt_load(frac_in + 20 * (u64)i), k));
}
// one lane per table row: sum_c D(id_c || value_c), row id, row_id * row digest
template <int V>
__global__ void __launch_bounds__(128) row_digest_kernel(const u64* col_ids, u32 n_cols, const u32* values, const u32* unique,
                                                          u32 n_unique, u32 rows, u64* frac_out) {
  u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  pt rd = pt_neutral();
  for (u32 c = 0; c < n_cols; c++) {
    u64 in[9];
    in[0] = col_ids[c];
    const u32* v = values + ((u64)r * n_cols + c) * 8;
#pragma unroll
    for (int j = 0; j < 8; j++) in[1 + j] = v[j];
    rd = pt_add(rd, map_to_curve<V>(in, 9));
  }
  // row_unique_data = H(unique columns as 8 big-endian u32 limbs each)   (mod.rs:499-510)
  u64 s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  const u32* uq = unique + (u64)r * n_unique * 8;
  for (u32 c = 0; c < n_unique; c++) {
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = uq[c * 8 + k];
    perm<V>(s);
  }
  // compute_row_id: H(row_unique_data(4) || num_actual_columns)[0..2] -> 128-bit scalar (mod.rs:512-523)
  u64 h[4] = {s[0], s[1], s[2], s[3]};
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  s[0] = h[0]; s[1] = h[1]; s[2] = h[2]; s[3] = h[3]; s[4] = n_cols;
  perm<V>(s);
  u32 k128[4] = {(u32)s[0], (u32)(s[0] >> 32), (u32)s[1], (u32)(s[1] >> 32)};
  pt_store(frac_out + 20 * (u64)r, pt_mul128(rd, k128));
}
// ---- launchers --------------------------------------------------------------------------------
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)
static inline dim3 g128(u32 n) { return dim3((n + 127) / 128); }

hipError_t ec_map_to_curve(hipStream_t s, int variant, const u64* in, u32 in_len, u32 count, u64* w_out, u64* wei_out, u64* frac_out) {
  if (!count) return hipSuccess;
  if (variant == MP2G_POSEIDON2) hipLaunchKernelGGL((map_to_curve_kernel<MP2G_POSEIDON2>), g128(count), dim3(128), 0, s, in, in_len, count, w_out, wei_out, frac_out);
  else hipLaunchKernelGGL((map_to_curve_kernel<MP2G_POSEIDON>), g128(count), dim3(128), 0, s, in, in_len, count, w_out, wei_out, frac_out);
  return hipGetLastError();
}
hipError_t ec_decode(hipStream_t s, const u64* w_in, u32 count, u64* frac_out, u32* bad) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(decode_kernel, g128(count), dim3(128), 0, s, w_in, count, frac_out, bad);
  return hipGetLastError();
}
// reduces frac[0..count) to one point in scratch[0..20); scratch needs 20*1024 words
hipError_t ec_sum(hipStream_t s, const u64* frac, u32 count, u64* scratch) {
  u32 blocks = (count + 127) / 128;
  if (blocks > 1024) blocks = 1024;
  if (blocks == 0) blocks = 1;
  if (blocks > 1) {
    hipLaunchKernelGGL(sum_kernel, dim3(blocks), dim3(128), 0, s, frac, count, scratch + 20);
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(128), 0, s, scratch + 20, blocks, scratch);
  } else {
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(128), 0, s, frac, count, scratch);
  }
  return hipGetLastError();
}
hipError_t ec_sum_ranges(hipStream_t s, const u64* frac, const u32* ranges, u32 n_ranges, u64* frac_out) {
  if (!n_ranges) return hipSuccess;
  hipLaunchKernelGGL(sum_ranges_kernel, dim3(n_ranges), dim3(64), 0, s, frac, ranges, frac_out);
  return hipGetLastError();
}
hipError_t ec_emit(hipStream_t s, const u64* frac, u32 count, u64* w_out, u64* wei_out) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(emit_kernel, g128(count), dim3(128), 0, s, frac, count, w_out, wei_out);
  return hipGetLastError();
}
hipError_t ec_scalar_mul(hipStream_t s, const u64* frac_in, const u32* scalars, u32 count, u64* frac_out) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(scalar_mul_kernel, g128(count), dim3(128), 0, s, frac_in, scalars, count, frac_out);
  return hipGetLastError();
}
hipError_t ec_row_digest(hipStream_t s, int variant, const u64* col_ids, u32 n_cols, const u32* values, const u32* unique,
                         u32 n_unique, u32 rows, u64* frac_out) {
  if (!rows) return hipSuccess;
  if (variant == MP2G_POSEIDON2) hipLaunchKernelGGL((row_digest_kernel<MP2G_POSEIDON2>), g128(rows), dim3(128), 0, s, col_ids, n_cols, values, unique, n_unique, rows, frac_out);
  else hipLaunchKernelGGL((row_digest_kernel<MP2G_POSEIDON>), g128(rows), dim3(128), 0, s, col_ids, n_cols, values, unique, n_unique, rows, frac_out);
  return hipGetLastError();
}
}  // namespace mp2g
