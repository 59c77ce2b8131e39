"""mp2g_swu_batch: simple_swu (mp2-common/src/group_hashing/sswu_value.rs:31-77) of GF(p^5) elements on the device, without the
sponge -- the reference's own known-answer inputs fed to the HIP kernel as raw words, random inputs against the CPU oracle, and limbs
in [p, 2^64) read mod p."""
import json
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
P = O.P


def o_swu(u):
    """the oracle's simple_swu of canonical inputs u [count][5]"""
    u = O.arr(u).reshape(-1, 5)
    w = np.zeros((u.shape[0], 5), dtype=np.uint64)
    wei = np.zeros((u.shape[0], 11), dtype=np.uint64)
    for i in range(u.shape[0]):
        row = np.ascontiguousarray(u[i])
        O.lib().orc_swu(O.p(row), O.p(w[i]), O.p(wei[i]))
    return w, wei


def test_swu_kats_through_hip(ctx, mp2):
    """sswu_value.rs:88-118: the three KAT inputs, as the raw u64 words the reference writes (the third holds u64::MAX limbs, which
    GoldilocksField reads mod p), give the three KAT outputs"""
    kat = json.load(open(os.path.join(G, "sswu_kat.json")))["vectors"]
    u = np.array([v["input"] for v in kat], dtype=np.uint64)
    assert (u >= np.uint64(P)).any()  # not reduced on the way in
    w, wei = mp2.swu_batch(ctx, u, weierstrass=True)
    assert [[int(x) for x in r] for r in w] == [v["output"] for v in kat]
    assert np.array_equal(mp2.swu_batch(ctx, u), w)
    ow, owei = o_swu([[x % P for x in v["input"]] for v in kat])
    assert np.array_equal(wei, owei)


def test_swu_batch_equals_the_oracle(ctx, mp2):
    """4096 random inputs and u = 0 (more than one block, a partial last block), encodings and Weierstrass limbs"""
    u = O.rand_field((4097, 5), 0x5A1)
    u[1234] = 0
    w, wei = mp2.swu_batch(ctx, u, weierstrass=True)
    ow, owei = o_swu(u)
    assert np.array_equal(w, ow) and np.array_equal(wei, owei)
    w1, wei1 = mp2.swu_batch(ctx, u[:1], weierstrass=True)
    assert np.array_equal(w1, ow[:1]) and np.array_equal(wei1, owei[:1])
    assert mp2.swu_batch(ctx, np.zeros((0, 5), dtype=np.uint64)).shape == (0, 5)


def test_swu_batch_reads_limbs_mod_p(ctx, mp2):
    """limbs in [p, 2^64) give what the same limbs reduced mod p give"""
    rng = np.random.default_rng(0x5A2)
    red = rng.integers(0, (1 << 32) - 1, size=(300, 5), dtype=np.uint64)  # values v < 2^32 - 1: v + p < 2^64
    raw = red.copy()
    hi = rng.random((300, 5)) < 0.6
    raw[hi] += np.uint64(P)
    raw[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    red[0] = np.uint64(0xFFFFFFFFFFFFFFFF - P)
    raw[1] = np.uint64(P)
    red[1] = 0
    assert (raw >= np.uint64(P)).sum() > 600
    w, wei = mp2.swu_batch(ctx, raw, weierstrass=True)
    w2, wei2 = mp2.swu_batch(ctx, red, weierstrass=True)
    assert np.array_equal(w, w2) and np.array_equal(wei, wei2)
    ow, owei = o_swu(red)
    assert np.array_equal(w, ow) and np.array_equal(wei, owei)
