"""The proof-of-work search (csrc/fri.hip: pow_kernel hands a proof's candidates out in order, in chunks of 256, from a ticket
counter of that proof) against the CPU oracle: the lone search against a full scan of every candidate up to the witness, the
batched search through the batched prover against the oracle's proofs word for word, and a prover object proving again (tickets
are reset by every search, under graph replay too)."""
import ctypes

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

_buf = (ctypes.c_uint64 * 12)()


def smallest_witness(state, pos, bits, variant, upto):
    """the first candidate of range(0, upto + 1) whose response has >= bits leading zeros (O.perm's routine, orc_perm, called on
    one reused buffer: the scan of the large witness is a few 10^5 permutations), or None"""
    perm, base = O.lib().orc_perm, [int(x) for x in state]
    for c in range(upto + 1):
        _buf[:] = base
        _buf[pos] = c
        perm(variant, _buf)
        if bits == 0 or _buf[7] >> (64 - bits) == 0:
            return c
    return None


def test_scan_helper_is_the_oracle_permutation():
    state = O.rand_field(12, 78)
    for variant in (0, 1):
        s = state.copy()
        s[3] = 5
        want = int(O.perm(s, variant)[7])
        _buf[:] = [int(x) for x in state]
        _buf[3] = 5
        O.lib().orc_perm(variant, _buf)
        assert _buf[7] == want


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("pos", [0, 3, 7])
def test_lone_search_full_scan(ctx, mp2, variant, pos):
    state = O.rand_field(12, 77 + pos)
    for bits in (0, 1, 8, 12):
        w = mp2.fri_pow(ctx, state, pos, bits, variant)
        assert smallest_witness(state, pos, bits, variant, w) == w, (pos, bits)


# (seed of the state, pos, bits, variant, witness): found on the CPU by scanning seeds with smallest_witness. 255 / 256: the last
# candidate of the first chunk and the first of the second; >= 2^18: beyond the 2^18 lanes of a lone launch, so every block of it
# takes a second ticket
CHOSEN = [
    (1005, 5, 4, 0, 0), (1253, 5, 9, 0, 255), (1291, 3, 10, 0, 256), (2018, 2, 19, 0, 293004),
    (1009, 1, 6, 1, 0), (1236, 4, 7, 1, 255), (1035, 3, 6, 1, 256), (2004, 4, 19, 1, 307173),
]


@pytest.mark.parametrize("seed,pos,bits,variant,witness", CHOSEN)
def test_lone_search_chosen_witness(ctx, mp2, seed, pos, bits, variant, witness):
    state = O.rand_field(12, seed)
    assert smallest_witness(state, pos, bits, variant, witness) == witness  # the case is what it says
    assert mp2.fri_pow(ctx, state, pos, bits, variant) == witness


# ---- batched search through the batched prover -------------------------------------------------
LOG_N, WS, POW_BITS, MAX_B = 3, (3, 4, 2, 2), 14, 300
_oracle_proofs = {}


def batch_params():
    return O.standard_params(LOG_N, WS, pow_bits=POW_BITS, num_queries=4)


def batch_inputs(b):
    return [O.rand_field((w, 1 << LOG_N), 100 * b + i) for i, w in enumerate(WS[1:])]


def shared():
    if "pre" not in _oracle_proofs:
        _oracle_proofs["pre"] = (O.rand_field((WS[0], 1 << LOG_N), 1), O.rand_field(4, 3), O.rand_field((MAX_B, 4), 4))
    return _oracle_proofs["pre"]


def oracle_proofs(B):
    """proof b is the same transcript in every batch that holds it: proved once by the oracle (the calls release the interpreter
    lock, so the missing ones are proved a few at a time), kept unchanged"""
    from concurrent.futures import ThreadPoolExecutor
    pre, cd, ph = shared()
    missing = [b for b in range(B) if b not in _oracle_proofs]
    with ThreadPoolExecutor(8) as pool:
        for b, proof in zip(missing, pool.map(lambda b: O.pcs_prove(batch_params(), [pre] + batch_inputs(b), cd, ph[b]), missing)):
            _oracle_proofs[b] = proof
    return [_oracle_proofs[b] for b in range(B)]


def make_prover(ctx, mp2, B):
    ofp = batch_params()
    fp = mp2.FriParams()
    ctypes.memmove(ctypes.byref(fp), ctypes.byref(ofp), ctypes.sizeof(fp))
    pre, cd, ph = shared()
    pr = mp2.BatchedProver(ctx, fp, B)
    pr.set_preprocessed(ctx.to_device(pre))
    per = [batch_inputs(b) for b in range(B)]
    args = ([ctx.to_device(np.stack([per[b][i] for b in range(B)])) for i in range(len(WS) - 1)], ctx.to_device(cd), ctx.to_device(ph[:B]))
    return pr, args


def check_batch(pr, B):
    caps, openings, proofs = pr.results()
    for b, (oc, oo, op) in enumerate(oracle_proofs(B)):
        assert np.array_equal(proofs[b], op), f"proof {b} of {B}"  # every word, the witness word among them
        assert np.array_equal(caps[b], oc) and np.array_equal(openings[b], oo)


@pytest.mark.parametrize("B", [1, 2, 5, 48, 300])
def test_batched_search_matches_oracle(ctx, mp2, B):
    """48: 42 blocks a proof, several ticket rounds; 300: the floor of 8 blocks a proof"""
    pr, args = make_prover(ctx, mp2, B)
    pr.prove(*args)
    check_batch(pr, B)
    pr.free()


def test_repeated_prove_resets_tickets(ctx, mp2):
    """the same prover object, the same buffers: from the third prove() on the launch sequence is replayed as a graph"""
    B = 5
    pr, args = make_prover(ctx, mp2, B)
    pr.enable_graph()
    for _ in range(5):
        pr.prove(*args)
        check_batch(pr, B)
    pr.free()
