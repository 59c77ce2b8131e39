// What a witness-tape instruction IS (include/mp2g.h enum mp2g_witness_op, _gf5, _lut, _wide), defined ONCE for the host
// (witness.hip: validation, level schedule, replay) and the device replay (witness_dev.hip): op_shape gives an instruction's length
// and operand roles, exec_core_op replays the recursion circuits' opcodes (MP2G_OP_ARITH .. MP2G_OP_HINT_SPLIT), exec_gate_op the
// leaf-circuit gates (MP2G_OP_U32_ARITH .. MP2G_OP_EXP; the GF(p^5) hints are witness_gf5.h, the wide block witness_wide.h). The gate generators restate
// mp2-common/src/serialization/circuit_data_serialization.rs:186-231 -- [dep] plonky2-u32 gates/{arithmetic_u32, subtraction_u32,
// add_many_u32, range_check_u32, comparison}.rs, plonky2 gates/{base_sum, multiplication_extension, exponentiation}.rs -- with the
// wire layouts of the gate evaluators (gates.hip / oracle/gates_body.inc). t = the operands after the opcode, vals = the proof's
// slot table, put(col, row, value) writes a wire. recursion.py's _OPS is the same table for the Python builder
// (tests/test_witness_shape_host.py holds the two together).
#pragma once
#include "gl.cuh"
#include "witness.h"

namespace mp2g {
// len = operands after the opcode (~0u: malformed); the operands [first_slot, len) are slots, the ones before it rows, indices and
// constants; the instruction reads the slots t[r0 .. r0 + nr) and writes t[w0 .. w0 + nw). OP_PAR has a length only (section count,
// then the sections' lengths in words; the sections follow as ordinary instructions).
struct OpShape { u32 len, first_slot, r0, nr, w0, nw; };
// left = how many words the tape holds after the opcode. The counts of the variable-length instructions are read here and nowhere
// else, after they are known to be there; the rest of the instruction may still run past the tape (len > left).
GLHD OpShape op_shape(u64 op, const u64* t, size_t left) {
  const OpShape malformed = {~0u, 0, 0, 0, 0, 0};
  switch (op) {
    case OP_ARITH: return {8, 4, 4, 3, 7, 1};
    case OP_ARITH_EXT: return {12, 4, 4, 6, 10, 2};
    case OP_P2: case OP_POSEIDON: return {26, 1, 1, 13, 14, 12};
    case OP_BASE_SUM: return {2 + BASE_SUM_LIMBS, 1, 1, 1, 2, BASE_SUM_LIMBS};
    case OP_RA: return {20, 2, 2, 17, 19, 1};
    case OP_REDUCING: return {5 + RED_COEFFS + 2, 1, 1, 4 + RED_COEFFS, 5 + RED_COEFFS, 2};
    case OP_REDUCING_EXT: return {5 + 2 * RED_EXT_COEFFS + 2, 1, 1, 4 + 2 * RED_EXT_COEFFS, 5 + 2 * RED_EXT_COEFFS, 2};
    case OP_COSET: {  // row, bits, shift, 2^bits values, point, result
      if (left < 2 || t[1] < 2 || t[1] > 5) return malformed;
      const u32 nv = 2u << t[1];
      return {3 + nv + 4, 2, 2, 3 + nv, 5 + nv, 2};
    }
    case OP_WIRE: return {3, 2, 2, 1, 0, 0};
    case OP_HINT_DIV_EXT: return {6, 0, 0, 4, 4, 2};
    case OP_HINT_LO63: case OP_HINT_HI: return {2, 0, 0, 1, 1, 1};
    case OP_HINT_SPLIT: return {4, 2, 0, 1, 2, 2};  // source slot, bit position, low slot, high slot (split_low_high's LowHighGenerator)
    case OP_PAR: return left >= 1 && t[0] <= 4096 ? OpShape{1 + (u32)t[0], 0, 0, 0, 0, 0} : malformed;
    case OP_U32_ARITH: case OP_U32_SUB: return {8, 3, 3, 3, 6, 2};
    case OP_U32_ADD_MANY: {  // row, operation, operations, addends, the addends, carry in, result, carry out
      if (left < 4 || t[3] < 1 || t[3] > 16) return malformed;
      const u32 na = (u32)t[3];
      return {4 + na + 3, 4, 4, na + 1, 5 + na, 2};
    }
    case OP_U32_RANGE_CHECK: return {4, 3, 3, 1, 0, 0};
    case OP_COMPARISON: return {6, 3, 3, 2, 5, 1};
    case OP_BASE_SPLIT: return left >= 3 && t[2] >= 1 && t[2] <= 63 ? OpShape{4 + (u32)t[2], 3, 3, 1, 4, (u32)t[2]} : malformed;
    case OP_MUL_EXT: return {9, 3, 3, 4, 7, 2};
    case OP_EXP: return left >= 2 && t[1] >= 1 && t[1] <= 66 ? OpShape{3 + (u32)t[1] + 1, 2, 2, 1 + (u32)t[1], 3 + (u32)t[1], 1} : malformed;
    case OP_QUINTIC_SQRT: return {11, 0, 0, 5, 5, 6};
    case OP_QUINTIC_QUOTIENT: return {15, 0, 0, 10, 10, 5};
    case OP_LOOKUP: return {5, 3, 3, 1, 4, 1};  // row, slot of the LookupGate row, table, input, output
    // the wide block (bodies: witness_wide.h)
    case OP_U32_INTERLEAVE: return {5, 3, 3, 1, 4, 1};  // row, operation, operations, x, x interleaved
    case OP_UNINTERLEAVE_TO_B32: case OP_UNINTERLEAVE_TO_U32: return {6, 3, 3, 1, 4, 2};  // row, operation, operations, x interleaved, evens, odds
    case OP_U256_DIV: return {33, 0, 0, 17, 17, 16};  // dividend[8], divisor[8], is_div, quotient[8], remainder[8]
    case OP_BIGUINT_DIV_REM: {  // limbs of a, limbs of b, a, b, div (as many limbs as a), rem (as many as b)
      if (left < 2 || t[0] < 1 || t[0] > BIGUINT_MAX_LIMBS || t[1] < 1 || t[1] > BIGUINT_MAX_LIMBS) return malformed;
      const u32 nl = (u32)t[0] + (u32)t[1];
      return {2 + 2 * nl, 2, 2, nl, 2 + nl, nl};
    }
    case OP_POSEIDON_MDS: return {49, 1, 1, 24, 25, 24};  // row, 12 extension inputs, 12 extension outputs
    default: return malformed;
  }
}

// The recursion circuits' opcodes. dom_tab / bw_tab = [6][32] words: the two-adic subgroup of 2^bits points and its barycentric
// weights in row `bits` (CosetInterpolation). MP2G_OP_P2 and MP2G_OP_POSEIDON are NOT here: their host and device replays are
// different algorithms, not copies -- the host (witness.hip) runs canonical values through 128-bit linear layers, the device
// (witness_dev.hip) weak representatives, and for short levels the 16-lane cooperative permutation.
template <class Put>
GLHD bool exec_core_op(u64 op, const u64* t, u64* vals, Put put, const u64* dom_tab, const u64* bw_tab) {
  switch (op) {
    case OP_WIRE: put(t[1], t[0], vals[t[2]]); return true;
    case OP_ARITH: {
      const u64 row = t[0], i = t[1], c0 = t[2], c1 = t[3];
      const u64 m0 = vals[t[4]], m1 = vals[t[5]], ad = vals[t[6]];
      const u64 o = gl_add(gl_mul(gl_mul(m0, m1), c0), gl_mul(ad, c1));
      put(4 * i, row, m0); put(4 * i + 1, row, m1); put(4 * i + 2, row, ad); put(4 * i + 3, row, o);
      vals[t[7]] = o;
      return true;
    }
    case OP_ARITH_EXT: {
      const u64 row = t[0], i = t[1], c0 = t[2], c1 = t[3];
      const gl2 m0 = gl2_make(vals[t[4]], vals[t[5]]), m1 = gl2_make(vals[t[6]], vals[t[7]]), ad = gl2_make(vals[t[8]], vals[t[9]]);
      const gl2 o = gl2_add(gl2_scale(gl2_mul(m0, m1), c0), gl2_scale(ad, c1));
      const u64 b = 8 * i;
      put(b, row, m0.a); put(b + 1, row, m0.b); put(b + 2, row, m1.a); put(b + 3, row, m1.b);
      put(b + 4, row, ad.a); put(b + 5, row, ad.b); put(b + 6, row, o.a); put(b + 7, row, o.b);
      vals[t[10]] = o.a; vals[t[11]] = o.b;
      return true;
    }
    case OP_BASE_SUM: {
      const u64 row = t[0], x = vals[t[1]];
      put(0, row, x);
#pragma unroll 1
      for (u32 i = 0; i < BASE_SUM_LIMBS; i++) { const u64 b = (x >> i) & 1; put(1 + i, row, b); vals[t[2 + i]] = b; }
      return true;
    }
    case OP_RA: {
      const u64 row = t[0], c = t[1], idx = vals[t[2]];
      const u32 vs = 1u << RA_BITS, base = (2 + vs) * (u32)c, routed = (2 + vs) * RA_COPIES + 2;
      put(base, row, idx);
#pragma unroll 1
      for (u32 i = 0; i < vs; i++) put(base + 2 + i, row, vals[t[3 + i]]);
      for (u32 i = 0; i < RA_BITS; i++) put(routed + c * RA_BITS + i, row, (idx >> i) & 1);
      const u64 o = vals[t[3 + (idx & (vs - 1))]];
      put(base + 1, row, o);
      vals[t[19]] = o;
      return true;
    }
    case OP_REDUCING: case OP_REDUCING_EXT: {
      const bool ext = op == OP_REDUCING_EXT;
      const u32 nc = ext ? RED_EXT_COEFFS : RED_COEFFS, start_accs = 6 + (ext ? 2 * nc : nc);
      const u64 row = t[0];
      const gl2 alpha = gl2_make(vals[t[1]], vals[t[2]]);
      gl2 acc = gl2_make(vals[t[3]], vals[t[4]]);
      put(2, row, alpha.a); put(3, row, alpha.b); put(4, row, acc.a); put(5, row, acc.b);
#pragma unroll 1
      for (u32 i = 0; i < nc; i++) {
        gl2 cf;
        if (ext) { cf = gl2_make(vals[t[5 + 2 * i]], vals[t[6 + 2 * i]]); put(6 + 2 * i, row, cf.a); put(7 + 2 * i, row, cf.b); }
        else { cf = gl2_make(vals[t[5 + i]], 0); put(6 + i, row, cf.a); }
        acc = gl2_add(gl2_mul(acc, alpha), cf);
        if (i < nc - 1) { put(start_accs + 2 * i, row, acc.a); put(start_accs + 2 * i + 1, row, acc.b); }
      }
      put(0, row, acc.a); put(1, row, acc.b);
      const u32 o = 5 + (ext ? 2 * nc : nc);
      vals[t[o]] = acc.a; vals[t[o + 1]] = acc.b;
      return true;
    }
    case OP_COSET: {
      const u64 row = t[0];
      const u32 bits = (u32)t[1], npts = 1u << bits;
      const u64* dom = dom_tab + 32 * bits;
      const u64* bw = bw_tab + 32 * bits;
      // CosetInterpolationGate::with_max_degree(bits, 8)
      const u32 nint0 = (npts - 2) / 7, deg = (npts - 2) / (nint0 + 1) + 2, nint = (npts - 2) / (deg - 1);
      const u32 w_pt = 1 + 2 * npts, w_val = w_pt + 2, w_int = w_val + 2, w_sh = w_int + 4 * nint;
      const u64 shift = vals[t[2]];
      put(0, row, shift);
      const u64* v = t + 3;
#pragma unroll 1
      for (u32 i = 0; i < 2 * npts; i++) put(1 + i, row, vals[v[i]]);
      const gl2 pt = gl2_make(vals[v[2 * npts]], vals[v[2 * npts + 1]]);
      put(w_pt, row, pt.a); put(w_pt + 1, row, pt.b);
      const gl2 sh = gl2_scale(pt, gl_inv(shift));
      put(w_sh, row, sh.a); put(w_sh + 1, row, sh.b);
      gl2 ev = gl2_make(0, 0), pr = gl2_make(1, 0);
      u32 start = 0, endi = deg;
#pragma unroll 1
      for (u32 c = 0; c <= nint; c++) {
#pragma unroll 1
        for (u32 i = start; i < endi; i++) {
          const gl2 val = gl2_scale(gl2_make(vals[v[2 * i]], vals[v[2 * i + 1]]), bw[i]);
          const gl2 term = gl2_make(gl_sub(sh.a, dom[i]), sh.b);
          const gl2 nev = gl2_add(gl2_mul(ev, term), gl2_mul(val, pr));
          pr = gl2_mul(pr, term);
          ev = nev;
        }
        if (c == nint) break;
        put(w_int + 2 * c, row, ev.a); put(w_int + 2 * c + 1, row, ev.b);
        put(w_int + 2 * (nint + c), row, pr.a); put(w_int + 2 * (nint + c) + 1, row, pr.b);
        start = 1 + (deg - 1) * (c + 1);
        endi = start + deg - 1 < npts ? start + deg - 1 : npts;
      }
      put(w_val, row, ev.a); put(w_val + 1, row, ev.b);
      vals[v[2 * npts + 2]] = ev.a; vals[v[2 * npts + 3]] = ev.b;
      return true;
    }
    case OP_HINT_DIV_EXT: {
      const gl2 num = gl2_make(vals[t[0]], vals[t[1]]), den = gl2_make(vals[t[2]], vals[t[3]]);
      const gl2 q = gl2_mul(num, gl2_inv(den));
      vals[t[4]] = q.a; vals[t[5]] = q.b;
      return true;
    }
    case OP_HINT_LO63: vals[t[1]] = vals[t[0]] & (((u64)1 << 63) - 1); return true;
    case OP_HINT_HI: vals[t[1]] = vals[t[0]] >> 63; return true;
    case OP_HINT_SPLIT: vals[t[2]] = vals[t[0]] & (((u64)1 << t[1]) - 1); vals[t[3]] = vals[t[0]] >> t[1]; return true;
    default: return false;
  }
}

// The lookup block. L = the program's tables (lookup_wires.h; create and set_lookups checked the row, the slot and the table).
// LookupGate / LookupGenerator: wires 2i, 2i+1 = the looked-up input and the table's output for it. An input the table does not
// hold gives 0: the pair is then in no table entry and the proof fails the lookup argument.
template <class Put>
GLHD bool exec_lut_op(u64 op, const u64* t, u64* vals, Put put, const LutIndex& L) {
  if (op != OP_LOOKUP) return false;
  const u64 row = t[0], i = t[1], lut = t[2], x = vals[t[3]];
  const u32 e = x < LUT_INPUTS ? L.index[lut][x] : LUT_ABSENT;
  const u64 out = e != LUT_ABSENT ? L.table[lut][2 * e + 1] : 0;
  put(2 * i, row, x); put(2 * i + 1, row, out);
  vals[t[4]] = out;
  return true;
}

// The leaf-circuit gates.
template <class Put>
GLHD bool exec_gate_op(u64 op, const u64* t, u64* vals, Put put) {
  switch (op) {
    case OP_U32_ARITH: {
      const u64 row = t[0], i = t[1], ops = t[2];
      const u64 m0 = vals[t[3]], m1 = vals[t[4]], ad = vals[t[5]];
      const u64 out = gl_add(gl_mul(m0, m1), ad);  // u32 operands: below p, the integer m0 m1 + addend itself
      const u64 lo = out & 0xFFFFFFFFull, hi = out >> 32;
      const u64 b = 6 * i;
      put(b, row, m0); put(b + 1, row, m1); put(b + 2, row, ad); put(b + 3, row, lo); put(b + 4, row, hi);
      put(b + 5, row, gl_inv(0xFFFFFFFFull - hi));  // (u32::MAX - high)^-1, 0 when high = u32::MAX (then low must be 0)
      for (u32 j = 0; j < 32; j++) put(6 * ops + 32 * i + j, row, (out >> (2 * j)) & 3);
      vals[t[6]] = lo; vals[t[7]] = hi;
      return true;
    }
    case OP_U32_SUB: {
      const u64 row = t[0], i = t[1], ops = t[2];
      const u64 x = vals[t[3]], y = vals[t[4]], bi = vals[t[5]];
      const u64 r0 = gl_sub(gl_sub(x, y), bi);          // negative differences sit just below p
      const u64 bo = r0 > ((u64)1 << 32) ? 1 : 0;
      const u64 r = gl_add(r0, bo << 32);
      const u64 b = 5 * i;
      put(b, row, x); put(b + 1, row, y); put(b + 2, row, bi); put(b + 3, row, r); put(b + 4, row, bo);
      for (u32 j = 0; j < 16; j++) put(5 * ops + 16 * i + j, row, (r >> (2 * j)) & 3);
      vals[t[6]] = r; vals[t[7]] = bo;
      return true;
    }
    case OP_U32_ADD_MANY: {
      const u64 row = t[0], i = t[1], ops = t[2], na = t[3];
      const u64 per = na + 3, b = per * i;
      u64 tot = 0;
      for (u32 k = 0; k < na; k++) { const u64 a = vals[t[4 + k]]; put(b + k, row, a); tot = gl_add(tot, a); }
      const u64 ci = vals[t[4 + na]];
      tot = gl_add(tot, ci);
      const u64 res = tot & 0xFFFFFFFFull, co = tot >> 32;
      put(b + na, row, ci); put(b + na + 1, row, res); put(b + na + 2, row, co);
      for (u32 j = 0; j < 16; j++) put(per * ops + 18 * i + j, row, (res >> (2 * j)) & 3);
      for (u32 j = 0; j < 2; j++) put(per * ops + 18 * i + 16 + j, row, (co >> (2 * j)) & 3);
      vals[t[5 + na]] = res; vals[t[6 + na]] = co;
      return true;
    }
    case OP_U32_RANGE_CHECK: {
      const u64 row = t[0], i = t[1], k = t[2], x = vals[t[3]];
      put(i, row, x);
      for (u32 j = 0; j < 16; j++) put(k + 16 * i + j, row, (x >> (2 * j)) & 3);
      return true;
    }
    case OP_COMPARISON: {
      const u64 row = t[0];
      const u32 nb = (u32)t[1], nch = (u32)t[2], cb = (nb + nch - 1) / nch;
      const u64 a = vals[t[3]], b = vals[t[4]], cmask = ((u64)1 << cb) - 1;
      put(0, row, a); put(1, row, b);
      // the chunks' differences first, then ALL their inverses from one field inversion (Montgomery's trick: prefix products over the
      // non-zero differences, one gl_inv, back-substitution): a lane replays the whole row, and 16 inversions of 64 squarings each
      // one after the other would make this row the longest instruction of its level
      u64 diff[16], pre[16], msd = 0, acc = 1;
      for (u32 i = 0; i < nch; i++) {
        const u64 fc = cb * i < 64 ? (a >> (cb * i)) & cmask : 0, sc = cb * i < 64 ? (b >> (cb * i)) & cmask : 0;
        put(4 + i, row, fc); put(4 + nch + i, row, sc);
        diff[i] = gl_sub(sc, fc);
        pre[i] = acc;                                   // product of the non-zero differences before chunk i
        if (diff[i]) acc = gl_mul(acc, diff[i]);
      }
      u64 inv_all = gl_inv(acc);                        // acc != 0: a product of non-zero field elements (1 when every chunk is equal)
      for (u32 i = nch; i-- > 0;) {
        if (!diff[i]) { pre[i] = 1; continue; }         // equality dummy of equal chunks: 1
        const u64 inv_i = gl_mul(inv_all, pre[i]);      // 1 / diff[i]
        inv_all = gl_mul(inv_all, diff[i]);
        pre[i] = inv_i;
      }
      for (u32 i = 0; i < nch; i++) {
        const u64 eq = diff[i] == 0 ? 1 : 0;
        put(4 + 2 * nch + i, row, pre[i]);              // equality dummy: 1 / (second - first), 1 for equal chunks
        put(4 + 3 * nch + i, row, eq);
        const u64 iv = eq ? msd : 0;
        put(4 + 4 * nch + i, row, iv);
        msd = eq ? iv : diff[i];                        // intermediate + (1 - equal) diff
      }
      put(3, row, msd);
      const u64 val = gl_add((u64)1 << cb, msd);  // 2^chunk_bits + most significant difference, in [1, 2^(chunk_bits + 1))
      for (u32 i = 0; i <= cb; i++) put(4 + 5 * nch + i, row, (val >> i) & 1);
      const u64 res = (val >> cb) & 1;
      put(2, row, res);
      vals[t[5]] = res;
      return true;
    }
    case OP_BASE_SPLIT: {
      const u64 row = t[0], bb = t[1], n = t[2], x = vals[t[3]], mask = ((u64)1 << bb) - 1;
      put(0, row, x);
      for (u32 j = 0; j < n; j++) { const u64 l = (x >> (bb * j)) & mask; put(1 + j, row, l); vals[t[4 + j]] = l; }
      return true;
    }
    case OP_MUL_EXT: {
      const u64 row = t[0], i = t[1], c0 = t[2];
      const gl2 m0 = gl2_make(vals[t[3]], vals[t[4]]), m1 = gl2_make(vals[t[5]], vals[t[6]]);
      const gl2 o = gl2_scale(gl2_mul(m0, m1), c0);
      const u64 b = 6 * i;
      put(b, row, m0.a); put(b + 1, row, m0.b); put(b + 2, row, m1.a); put(b + 3, row, m1.b); put(b + 4, row, o.a); put(b + 5, row, o.b);
      vals[t[7]] = o.a; vals[t[8]] = o.b;
      return true;
    }
    case OP_EXP: {
      const u64 row = t[0];
      const u32 nb = (u32)t[1];
      const u64 base = vals[t[2]];
      put(0, row, base);
      for (u32 j = 0; j < nb; j++) put(1 + j, row, vals[t[3 + j]]);
      u64 cur = 1;
      for (u32 i = 0; i < nb; i++) {  // most significant bit first: square, then multiply by base where the bit is set
        const u64 prev = i == 0 ? 1 : gl_mul(cur, cur);
        cur = vals[t[3 + nb - 1 - i]] ? gl_mul(prev, base) : prev;
        put(nb + 2 + i, row, cur);
      }
      put(nb + 1, row, cur);
      vals[t[3 + nb]] = cur;
      return true;
    }
    default: return false;
  }
}
}  // namespace mp2g
