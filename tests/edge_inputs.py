"""Edge-valued inputs for the tests that go through the C ABI (tests/test_gpu_edge_operands.py and its MP2G_NTT_V1 child): rows drawn
from the canonical edge lattice of tests/field_cases.py, and the NTT cases built from them. Seeded, so that the parent and the child
process construct the same arrays."""
import hashlib

import numpy as np

import field_cases as F
import oracle as O

EC = np.array(F.EC, dtype=np.uint64)
NTT_LOG_N = [3, 6, 9, 11, 12, 13, 15]  # single-pass tiles, the LT >= 11 global-twiddle round, the two-pass kernels
NTT_BATCH = 3
NTT_MODES = [{}, {"inverse": True}, {"coset_shift": O.MULT_GEN}, {"inverse": True, "coset_shift": O.MULT_GEN}, {"bitrev_out": True}]


def edge_rows(shape, seed):
    """an array of the given shape with every entry drawn from the canonical lattice"""
    return EC[np.random.default_rng(seed).integers(0, len(EC), size=shape)]


def constant_rows(width):
    """one row per lattice value, all entries equal"""
    return np.repeat(EC[:, None], width, axis=1)


def oracle_ntt(a, inverse=False, coset_shift=0, bitrev_out=False):
    out = O.fft(a, inverse=inverse, coset_shift=coset_shift)
    return out[:, O.bitrev_perm(a.shape[1])] if bitrev_out else out


def ntt_cases(log_n):
    """(label, input, mode, expected) for one size.
    'in': edge-valued inputs in every mode. 'out': inputs whose transform is edge-valued -- the oracle's inverse transform of an
    edge row e, so that the transform must return e itself and the last butterfly round lands on sums and differences at 0, p - 1
    and just across p; the same with the directions swapped, and through the coset."""
    e = edge_rows((NTT_BATCH, 1 << log_n), 7000 + log_n)
    for i, mode in enumerate(NTT_MODES):
        yield "in%d" % i, e, mode, oracle_ntt(e, **mode)
    g = O.MULT_GEN
    yield "out-fwd", O.fft(e, inverse=True), {}, e
    yield "out-inv", O.fft(e), {"inverse": True}, e
    yield "out-coset", O.fft(e, inverse=True, coset_shift=g), {"coset_shift": g}, e
    yield "out-inv-coset", O.fft(e, coset_shift=g), {"inverse": True, "coset_shift": g}, e
    yield "out-bitrev", O.fft(e, inverse=True), {"bitrev_out": True}, e[:, O.bitrev_perm(1 << log_n)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()
