// The scalar routines of the field-arithmetic tests, listed once for the device harness (field_dev.hip) and the host program
// (tools/hosttest/perm_host_test.cpp): X(name, body), where body computes (o0, o1) from the operands (a, b, c).
// Weak-output routines return their value in o0 and its gl_canon in o1.
#pragma once

// routines with a host and a device body
#define SCALAR_OPS_HD(X)                                                \
  X(gl_canon, o0 = gl_canon(a))                                         \
  X(gl_add, o0 = gl_add(a, b))                                          \
  X(gl_sub, o0 = gl_sub(a, b))                                          \
  X(gl_neg, o0 = gl_neg(a))                                             \
  X(gl_addw, o0 = gl_addw(a, b); o1 = gl_canon(o0))                     \
  X(gl_reduce128w, o0 = gl_reduce128w(a, b); o1 = gl_canon(o0))         \
  X(gl_reduce96w, o0 = gl_reduce96w(a, b); o1 = gl_canon(o0))           \
  X(gl_reduce128, o0 = gl_reduce128(a, b))                              \
  X(gl_mul_wide, gl_mul_wide(a, b, o0, o1))                             \
  X(gl_mul_add_wide, gl_mul_add_wide(a, b, c, o0, o1))                  \
  X(gl_mul, o0 = gl_mul(a, b))                                          \
  X(gl_mulw, o0 = gl_mulw(a, b); o1 = gl_canon(o0))                     \
  X(gl_mul_addw, o0 = gl_mul_addw(a, b, c); o1 = gl_canon(o0))          \
  X(gl_mul_add, o0 = gl_mul_add(a, b, c))                               \
  X(gl_mul_small, o0 = gl_mul_small(a, (u32)b))                         \
  X(gl_mul_small_w, o0 = gl_mul_small_w(a, (u32)b); o1 = gl_canon(o0))  \
  X(gl_pow7, o0 = gl_pow7(a))                                           \
  X(gl_inv, o0 = gl_inv(a))                                             \
  X(gl_inv_chain, o0 = gl_inv_chain(a))                                 \
  X(gl_sqrt, o1 = gl_sqrt(a, o0) ? 1 : 0)                               \
  X(gl_is_square, o0 = gl_is_square(a) ? 1 : 0)                         \
  X(p2_sbox, o0 = p2_sbox(a, b); o1 = gl_canon(o0))                     \
  X(p2_sbox0, o0 = p2_sbox0(a); o1 = gl_canon(o0))                      

// device only: the NTT shift arithmetic of ntt_arith.cuh (mul_2pow_any: gl_mul_2pow<S> for a run-time S, field_dev.hip)
#define SCALAR_OPS_DEV(X)                          \
  X(gl_mul_2p24, o0 = gl_mul_2p24(a))              \
  X(gl_mul_2p48, o0 = gl_mul_2p48(a))              \
  X(gl_mul_2p72, o0 = gl_mul_2p72(a))              \
  X(gl_sub_mul_2p48, o0 = gl_sub_mul_2p48(a, b))   \
  X(gl_sub_mul_2p72, o0 = gl_sub_mul_2p72(a, b))   \
  X(gl_mul_w8_1, o0 = gl_mul_w8<1>(a))             \
  X(gl_mul_w8_2, o0 = gl_mul_w8<2>(a))             \
  X(gl_mul_w8_3, o0 = gl_mul_w8<3>(a))             \
  X(gl_sub_mul_w8_1, o0 = gl_sub_mul_w8<1>(a, b))  \
  X(gl_sub_mul_w8_2, o0 = gl_sub_mul_w8<2>(a, b))  \
  X(gl_sub_mul_w8_3, o0 = gl_sub_mul_w8<3>(a, b))  \
  X(bfly_lo_1, o0 = bfly_lo<1>(a, b, c != 0))      \
  X(bfly_lo_2, o0 = bfly_lo<2>(a, b, c != 0))      \
  X(bfly_lo_3, o0 = bfly_lo<3>(a, b, c != 0))      \
  X(gl_mul_2pow, o0 = mul_2pow_any(a, (u32)b))     
