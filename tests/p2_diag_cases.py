"""Operands and the exact reference for the constant-operand multiply-add gl_mulc_addw (csrc/gl.cuh) over the twelve entries of
Poseidon2's internal diagonal: pure Python, no product code. tests/test_gpu_p2_diag.py runs the device body on them,
tests/test_p2_diag_constants.py the portable one."""
import itertools

import numpy as np

import field_cases as F

P, M32, M64 = F.P, F.M32, F.M64
N_UNIFORM = 1 << 16


def diag():
    return F.header_table("POSEIDON2_DIAG_M1")


def column_cases(d):
    """(a, c) that drive the columns of X = a0 d + a1 e + c, e = d 2^32 mod p, to their ends: where a missed carry shows"""
    e = (d << 32) % P
    out = [(M64, M64), (0, 0), (0, P)]  # every column at its largest; nothing at all; a bare p in the addend
    # X = 2^96 - 1, 2^96, 2^96 + 1 where operands reach it: the top word needs its 33rd bit from 2^96 on, and at X = 2^96 every other
    # word is zero (a fold of that bit with 2^96 = -1 would have to borrow from nothing)
    for target in ((1 << 96) - 1, 1 << 96, (1 << 96) + 1):
        a1 = min(M32, target // e)
        rem = target - a1 * e
        a0 = min(M32, rem // d)
        rem -= a0 * d
        if rem <= M64:
            out.append(((a1 << 32) | a0, rem))
    # a1 alone around the first carry out of the a1 e column: a1 e = 2^96 -/+ less than e
    a1 = (1 << 96) // e
    for x in (a1 - 1, a1, a1 + 1):
        if 0 <= x <= M32:
            out += [(x << 32, 0), (x << 32, M64), ((x << 32) | M32, M64)]
    return out


def cases(k, n_uniform=N_UNIFORM):
    """(a, c) columns for diagonal entry k: the full edge-word lattice (every pair of any-u64 lattice values), the column cases, then
    n_uniform seeded uniform pairs"""
    lat = list(itertools.product(F.EANY, F.EANY)) + column_cases(diag()[k])
    a = np.concatenate([np.array([x for x, _ in lat], dtype=np.uint64), F.uniform(n_uniform, 1 << 64, (k, 0, 0xD1A6))])
    c = np.concatenate([np.array([y for _, y in lat], dtype=np.uint64), F.uniform(n_uniform, 1 << 64, (k, 1, 0xD1A6))])
    return a, c


def bad_cases(k, a, c, out):
    """indices where canon(out) != (a d_k + c) mod p"""
    d = diag()[k]
    return [i for i, (x, y, r) in enumerate(zip(a.tolist(), c.tolist(), out.tolist())) if r % P != (x * d + y) % P]
