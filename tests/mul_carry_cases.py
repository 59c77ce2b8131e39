"""Operands and exact references for the general 64 x 64 product as the S-boxes form it (gl_mulw_k, csrc/gl.cuh): pure Python, no product
code. The routine sums both middle products in ONE 64-bit accumulator and takes the bit that sum can carry past 2^64 from the
multiply-add itself; `columns()` is a model of that sequence on Python integers, so which side of 2^64 an operand pair puts the
accumulator on is known from the operands alone. tests/test_mul_carry_cases.py guards the tables, tests/test_gpu_mul_carry.py runs the
device bodies on them.

The multiply-add gl_mul_addw keeps the product hipcc schedules (gl_mul_add_wide: the halves of c ride in the first two addend slots, the
middle products stay apart); `columns_add()` models that one, and ADD_CASES holds the addends that push its columns to their ends."""
import itertools

import numpy as np

import field_cases as F

P, M32, M64 = F.P, F.M32, F.M64
M = M32
N_UNIFORM = 1 << 16

# the column bounds that the comment of gl_mulw_k states
BOUND_P = M * M                  # a0 b0
BOUND_M1 = M * M + M - 1         # a0 b1 + (P >> 32), fits 64 bits
BOUND_M2 = 2 * M * M + M - 1     # a1 b0 + m1, below 2^65
BOUND_HI = (1 << 64) - 2         # the high word of (2^64 - 1)^2
# ... and of gl_mul_add_wide
BOUND_ADD_P = M * M + M          # a0 b0 + c0
BOUND_ADD_M1 = M * M + 2 * M     # a0 b1 + (P >> 32) + c1 = 2^64 - 1


def columns(a, b):
    """the columns of gl_mulw_k -> dict(P, m1, m2, k, q, lo, hi) with lo + 2^64 hi == a b"""
    a0, a1, b0, b1 = a & M, a >> 32, b & M, b >> 32
    p = a0 * b0
    m1 = a0 * b1 + (p >> 32)
    m2 = a1 * b0 + m1
    k, q = m2 >> 64, m2 & M64
    hi = a1 * b1 + ((q >> 32) | (k << 32))
    lo = (p & M) | ((q & M) << 32)
    return dict(P=p, m1=m1, m2=m2, k=k, q=q, lo=lo, hi=hi)


def columns_add(a, b, c):
    """the columns of gl_mul_add_wide -> dict(P, m1, m2, lo, hi) with lo + 2^64 hi == a b + c"""
    a0, a1, b0, b1 = a & M, a >> 32, b & M, b >> 32
    p = a0 * b0 + (c & M)
    m1 = a0 * b1 + (p >> 32) + (c >> 32)
    m2 = a1 * b0 + (m1 & M)
    hi = a1 * b1 + (m1 >> 32) + (m2 >> 32)
    lo = (p & M) | ((m2 & M) << 32)
    return dict(P=p, m1=m1, m2=m2, lo=lo, hi=hi)


# (a, b): the middle accumulator on both sides of 2^64 and at its ends
ACC_EXACTLY_2P64 = ((M << 32) | 2, (M << 32) | M)        # m2 = 2^64: k = 1 and a zero low word
ACC_JUST_BELOW = ((M << 32) | 2, ((M - 1) << 32) | M)    # m2 = 2^64 - 2: k = 0
ACC_MAXIMUM = (M64, M64)                                 # every column at its bound
CARRY_PAIRS = [
    ACC_EXACTLY_2P64, ACC_JUST_BELOW, ACC_MAXIMUM,
    ((M << 32) | 1, (M << 32) | M), ((M << 32) | 3, (M << 32) | M),            # around 2^64 from the a0 side: 2^64 - M - 1, 2^64 + M + 1
    (M << 32, M << 32), (M, M), (M << 32, M), (M, M << 32), (0, M64), (M64, 0), (0, 0),   # zero halves
    (1 << 32, 1 << 32), (1 << 32, M64), (M64, 1 << 32), (1, M64),
] + list(itertools.product([P - 1, P, P + 1], repeat=2)) + [(x, M64) for x in (P - 1, P, P + 1)]

# (a, b, c) for the multiply-add: the addends that push its columns to their ends, and the pairs above with the extreme addends
ADD_COLUMNS_AT_BOUND = (M64, M64, M64)   # P = M^2 + M, m1 = 2^64 - 1
ADD_CASES = [ADD_COLUMNS_AT_BOUND, (M64, M64, M32), (M64, M64, M32 << 32), (M, M64, M64), (M64, M, M64), (0, 0, M64), (0, 0, P), (M64, M64, 0)]
ADD_CASES += [(a, b, c) for a, b in CARRY_PAIRS[:5] for c in (0, M32, M32 << 32, P - 1, M64)]
LATTICE_ADDENDS = [0, M32, M32 << 32, P - 1, M64]


def pairs(n_uniform=N_UNIFORM):
    """(a, b) columns: the carry pairs, every pair of the 49 any-u64 lattice values of tests/field_cases.py, then n_uniform seeded
    uniform pairs"""
    lat = CARRY_PAIRS + list(itertools.product(F.EANY, F.EANY))
    a = np.concatenate([np.array([x for x, _ in lat], dtype=np.uint64), F.uniform(n_uniform, 1 << 64, (0, 0xCA44))])
    b = np.concatenate([np.array([y for _, y in lat], dtype=np.uint64), F.uniform(n_uniform, 1 << 64, (1, 0xCA44))])
    return a, b


def triples(n_uniform=N_UNIFORM):
    """(a, b, c) columns for the multiply-add: ADD_CASES, the pairs of pairs() with the lattice pairs' addends cycling through
    LATTICE_ADDENDS and the carry pairs' at zero, uniform pairs with uniform addends"""
    a, b = pairs(n_uniform)
    n_lat = len(a) - n_uniform
    c = np.concatenate([np.zeros(len(CARRY_PAIRS), dtype=np.uint64),
                        np.array([LATTICE_ADDENDS[i % len(LATTICE_ADDENDS)] for i in range(n_lat - len(CARRY_PAIRS))], dtype=np.uint64),
                        F.uniform(n_uniform, 1 << 64, (2, 0xCA44))])
    t = np.array(ADD_CASES, dtype=np.uint64)
    return np.concatenate([t[:, 0], a]), np.concatenate([t[:, 1], b]), np.concatenate([t[:, 2], c])


def bad_wide(a, b, lo, hi):
    """indices where lo + 2^64 hi != a b"""
    return [i for i, (x, y, l, h) in enumerate(zip(a.tolist(), b.tolist(), lo.tolist(), hi.tolist())) if l + (h << 64) != x * y]


def bad_weak(want, out, canon):
    """indices where a weak result breaks its contract: out congruent to want (mod p), canon == want mod p exactly"""
    return [i for i, (w, r, k) in enumerate(zip(want, out.tolist(), canon.tolist())) if r % P != w % P or k != w % P]


def bad_canon(want, out):
    return [i for i, (w, r) in enumerate(zip(want, out.tolist())) if r != w % P]
