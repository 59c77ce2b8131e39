"""Edge operands through the C ABI, bit for bit against the oracle: the transforms, hashes, trees, LDE and FRI folding on inputs drawn
from the canonical edge lattice of tests/field_cases.py (32-bit words 0, 1, 2, 2^31 - 1, 2^31, 2^32 - 2, 2^32 - 1 in both halves,
plus p - 1 and p - 2) instead of uniform field elements, which reach the rare carry and borrow branches of the field arithmetic with
probability ~2^-32 per operation."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_inputs as X
import oracle as O

pytestmark = pytest.mark.gpu
P = O.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("log_n", X.NTT_LOG_N)
def test_ntt_edge_inputs_and_edge_outputs(ctx, log_n):
    for label, a, mode, want in X.ntt_cases(log_n):
        if label.startswith("out"):
            assert np.array_equal(X.oracle_ntt(a, **mode), want), label  # the oracle inverts itself: the input really transforms to e
        assert np.array_equal(ctx.ntt(a, **mode), want), (log_n, label)


def test_ntt_edge_cases_through_the_barrier_per_round_kernels():
    """the same cases under MP2G_NTT_V1=1, in one child process that prints a digest per case; compared with the oracle's outputs"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ntt_edge_child.py"), ROOT], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, MP2G_NTT_V1="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(line.split()) for line in r.stdout.strip().splitlines() if len(line.split()) == 3 and len(line.split()[2]) == 64]
    want = [(str(log_n), label, X.digest(w)) for log_n in X.NTT_LOG_N for label, _, _, w in X.ntt_cases(log_n)]
    assert got == want


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("in_len", [1, 8, 9, 135])
def test_hash_no_pad_batch_edge_rows(ctx, variant, in_len):
    x = np.concatenate([X.edge_rows((300, in_len), 7100 + in_len), X.constant_rows(in_len)])
    assert np.array_equal(ctx.hash_no_pad_batch(x, 4, variant), O.hash_no_pad_batch(x, 4, variant))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("log_leaves,leaf_len,cap_h", [(3, 4, 0), (6, 7, 2), (8, 135, 4)])
def test_merkle_tree_edge_leaves(ctx, mp2, variant, log_leaves, leaf_len, cap_h):
    L = 1 << log_leaves
    leaves = X.edge_rows((L, leaf_len), 7200 + log_leaves)
    const = X.constant_rows(leaf_len)[np.random.default_rng(log_leaves).permutation(len(X.EC))[:L // 2]]
    leaves[1::2][:len(const)] = const  # every other leaf a constant row, as many as fit
    t = mp2.MerkleTree(ctx, leaves, cap_h, variant)
    levels = O.merkle_build(leaves, cap_h, variant)
    cap = O.merkle_cap(levels, cap_h)
    assert np.array_equal(t.cap, cap)
    idx = sorted({0, 1, L - 1, L // 2, min(3, L - 1)})
    got_leaves, sib = t.prove(idx)
    for k, i in enumerate(idx):
        assert np.array_equal(got_leaves[k], leaves[i])
        assert np.array_equal(sib[k], O.merkle_prove(levels, log_leaves, cap_h, i))
        assert O.merkle_verify(leaves[i], i, sib[k], cap, variant)
    t.free()


@pytest.mark.parametrize("log_n,w", [(6, 5), (12, 3)])
def test_lde_leaves_edge_coefficients(ctx, log_n, w):
    c = X.edge_rows((w, 1 << log_n), 7300 + log_n)
    assert np.array_equal(ctx.lde_leaves(c, 3), O.lde_leaves(c, 3))


@pytest.mark.parametrize("beta", [(0, 0), (1, 0), (P - 1, P - 1)])
@pytest.mark.parametrize("log_m,ab", [(4, 4), (7, 4), (11, 4), (15, 4), (6, 1), (6, 2), (9, 3)])
def test_fri_fold_edge_evaluations(ctx, mp2, log_m, ab, beta):
    m = 1 << log_m
    vb = O.arr(X.edge_rows((m, 2), 7400 + log_m))  # evaluations in leaf (bit-reversed) order; any values are evaluations of something
    beta = np.array(beta, dtype=np.uint64)
    shift = O.MULT_GEN
    want = np.zeros((m >> ab, 2), dtype=np.uint64)
    O.lib().orc_fri_fold_values(O.p(vb), log_m, ab, O.p(beta), ctypes.c_uint64(shift), O.p(want))
    got = mp2.fri_fold(ctx, vb, ab, beta, shift)
    assert np.array_equal(got, want[O.bitrev_perm(m >> ab)])  # the oracle returns natural order
