"""The checker of the Keccak-256 kernels, held against what does not depend on it (no GPU, no code under test): the sponge against
hashlib's SHA3-256 (the same permutation and padding, another domain byte), against the standard Keccak-256 answers of
tests/golden/keccak_kat.json, and the case tables against the statuses they were built for."""
import hashlib

import pytest

import keccak_cases as K


@pytest.mark.parametrize("lengths", [range(0, 101), range(101, 201), range(201, 301), [532, 543, 544, 545]], ids=["0-100", "101-200", "201-300", "long"])
def test_sponge_is_sha3_256_with_its_domain_byte(lengths):
    for n in lengths:
        msg = K.message(n, 7)
        assert K.sponge256(msg, 0x06) == hashlib.sha3_256(msg).digest(), n


def test_golden_answers():
    assert len(K.GOLDEN["keccak256"]) == 4
    for kat in K.GOLDEN["keccak256"]:
        assert K.sponge256(bytes.fromhex(kat["message_hex"]), 0x01).hex() == kat["digest_hex"], kat["name"]
    assert K.sponge256(b"", 0x01) != K.sponge256(b"", 0x06)


def test_slot_restatement():
    want = bytes.fromhex(K.GOLDEN["mapping_key0_slot0_location_hex"])
    assert K.location(K.mapping(b"", 0)) == want and K.location(K.mapping(bytes(32), 0)) == want
    assert K.slot_keys(0, None, [bytes(32)], 0)[0] == want
    assert K.location(K.simple(7)) == bytes(31) + b"\x07" and K.location(K.simple((1 << 64) - 1)) == bytes(24) + b"\xff" * 8
    assert K.location(K.mapping(b"\x01", 0x1FF)) == K.location(K.mapping(b"\x01", 0xFF))  # `as u8`
    s = K.node_mapping(K.node_struct(K.mapping(b"\xaa" * 20, 3), 2), b"\x05")
    step = K.slot_keys(3, None, [K.left_pad32(b"\xaa" * 20)], 2)
    assert K.location(K.node_struct(K.mapping(b"\xaa" * 20, 3), 2)) == step[0]
    assert (K.location(s), K.mpt_key(s), bytes(K.mpt_nibbles(s))) == K.slot_keys(0, step[0], [K.left_pad32(b"\x05")], 0)[:3]
    assert K.mpt_nibbles(s)[:2] == [K.mpt_key(s)[0] >> 4, K.mpt_key(s)[0] & 15] and len(K.mpt_nibbles(s)) == 64
    # checked_add: the carry that crosses every word, and the one that leaves 256 bits
    assert K.slot_keys(0, b"\x00" + b"\xff" * 31, [], 1)[0] == b"\x01" + bytes(31)
    assert K.slot_keys(0, b"\xff" * 32, [], 1) == (bytes(32), bytes(32), bytes(64), 1)
    assert K.location(K.node_struct(("simple", (1 << 64) - 1), 1)) == bytes(23) + b"\x01" + bytes(8)


def test_good_leaves_decode():
    leaves = K.good_leaves()
    assert len(leaves) == len(K.VALUES) * len(K.PATH_LENGTHS) + 2
    for label, node, key in leaves:
        status, word, n = K.decode_leaf(node, key)
        assert status == K.OK and K.decode_leaf(node)[0] == K.OK, label
        assert n == (64 if label.startswith("list") else int(label.split(", ")[1].split()[0])), label
    by = {label: K.decode_leaf(node, key)[1] for label, node, key in leaves}
    assert by["value 05, 0 nibbles"] == bytes(31) + b"\x05" and by["value 80, 1 nibbles"] == bytes(31) + b"\x80"
    assert by["value empty, 64 nibbles"] == bytes(32) and by["value 1234, 63 nibbles"] == bytes(30) + b"\x12\x34"
    assert by[f"value {bytes(range(0xE0, 0x100)).hex()}, 2 nibbles"] == bytes(range(0xE0, 0x100))
    assert {node[0] for _, node, _ in leaves if len(node) > 57} == {0xF8} and max(len(node) for _, node, _ in leaves) == 70


def test_damaged_leaves_have_the_intended_status():
    cases = K.damaged_leaves()
    assert {c[3] for c in cases} == {K.MALFORMED, K.NOT_A_LEAF, K.BAD_VALUE, K.KEY_MISMATCH}
    for label, node, key, want in cases:
        status, word, n = K.decode_leaf(node, key)
        assert (status, word, n) == (want, bytes(32), 0), label
        if want == K.KEY_MISMATCH:
            assert K.decode_leaf(node)[0] == K.OK, label  # without a key the leaf is sound
