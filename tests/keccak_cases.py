"""Case tables for the Keccak-256 kernels (csrc/keccak.cuh, csrc/storage.hip) and the checker's restatement of what the reference
computes between an eth_getProof answer and a storage leaf's 32-byte word: a plain-Python Keccak-f[1600] sponge with the domain
byte as a parameter (0x01 = Ethereum's keccak256, 0x06 = SHA3-256, which hashlib has: tests/test_keccak_cases.py holds the two
together), StorageSlot::location / mpt_key / mpt_nibbles (mp2-common/src/eth.rs:233-276), a minimal RLP encoder for leaf nodes and
the leaf decode with the status rules of include/mp2g.h. No GPU is used here and nothing here calls the code under test.

The builders are seeded and cached: every caller gets the same objects and must leave them unchanged."""
import functools
import json
import os

import numpy as np

MASK = (1 << 64) - 1
RATE = 136
RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
      0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keccak_kat.json")))


def _rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f1600(a):
    """the permutation on 25 lanes, lane (x, y) at a[x + 5 y]; rho's offsets come from the walk (x, y) -> (y, 2 x + 3 y), as the
    specification generates them, not from a table"""
    a = list(a)
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1)
            for y in range(5):
                a[x + 5 * y] ^= d
        b = [0] * 25
        b[0] = a[0]
        x, y = 1, 0
        for t in range(24):
            b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y], ((t + 1) * (t + 2) // 2) % 64)
            x, y = y, (2 * x + 3 * y) % 5
        a = [b[i] ^ (~b[5 * (i // 5) + (i + 1) % 5] & MASK & b[5 * (i // 5) + (i + 2) % 5]) for i in range(25)]
        a[0] ^= rc
    return a


def sponge256(msg, domain=0x01):
    """32 bytes out of the rate-136 sponge: pad10*1 after the domain bits"""
    msg = bytearray(msg)
    pad = RATE - len(msg) % RATE
    msg += bytes(pad)
    msg[-pad] ^= domain
    msg[-1] ^= 0x80
    a = [0] * 25
    for off in range(0, len(msg), RATE):
        for j in range(17):
            a[j] ^= int.from_bytes(msg[off + 8 * j:off + 8 * j + 8], "little")
        a = keccak_f1600(a)
    return b"".join(x.to_bytes(8, "little") for x in a[:4])


@functools.lru_cache(maxsize=None)
def keccak256(msg):
    return sponge256(msg, 0x01)


# ---- StorageSlot (mp2-common/src/eth.rs:158-300) as nested tuples -----------------------------------------------------------------
def left_pad32(b):
    assert len(b) <= 32
    return bytes(32 - len(b)) + bytes(b)


def simple(slot):
    return ("simple", slot)


def mapping(key, slot):
    return ("mapping", bytes(key), slot)


def node_mapping(parent, key):
    """the enum variant StorageSlotNode::Mapping itself, which takes any parent (a mapping below a struct's field); new_mapping is
    the constructor that refuses a parent that is not of mapping type (eth.rs:175-185)"""
    return ("node_mapping", parent, bytes(key))


def new_mapping(parent, key):
    if parent[0] not in ("mapping", "node_mapping"):
        raise ValueError("The parent of a Slot mapping entry must be type of mapping")
    return node_mapping(parent, key)


def node_struct(parent, evm_offset):
    return ("node_struct", parent, evm_offset)


def location(s):
    """eth.rs:233-266; None where checked_add(..).unwrap() panics"""
    if s[0] == "simple":
        return (s[1] & MASK).to_bytes(32, "big")
    if s[0] == "mapping":
        return keccak256(left_pad32(s[1]) + left_pad32(bytes([s[2] & 0xFF])))
    parent = location(s[1])
    if parent is None:
        return None
    if s[0] == "node_mapping":
        return keccak256(left_pad32(s[2]) + parent)
    v = int.from_bytes(parent, "big") + s[2]
    return None if v >> 256 else v.to_bytes(32, "big")


def mpt_key(s):
    loc = location(s)
    return None if loc is None else keccak256(loc)


def bytes_to_nibbles(b):
    return [n for x in b for n in (x >> 4, x & 15)]


def mpt_nibbles(s):
    k = mpt_key(s)
    return None if k is None else bytes_to_nibbles(k)


def slot_keys(slot, parent, keys, evm_offset):
    """what mp2g_storage_slot_keys computes for one leaf, step by step: (location, mpt_key, nibbles as bytes), all zero on overflow"""
    loc = parent if parent is not None else (slot & MASK).to_bytes(32, "big")
    for k in keys:
        loc = keccak256(bytes(k) + loc)
    v = int.from_bytes(loc, "big") + evm_offset
    if v >> 256:
        return bytes(32), bytes(32), bytes(64), 1
    loc = v.to_bytes(32, "big")
    key = keccak256(loc)
    return loc, key, bytes(bytes_to_nibbles(key)), 0


# ---- RLP for leaf nodes ---------------------------------------------------------------------------------------------------------------
def rlp_string(b):
    b = bytes(b)
    if len(b) == 1 and b[0] < 0x80:
        return b
    if len(b) < 56:
        return bytes([0x80 + len(b)]) + b
    assert len(b) < 256
    return bytes([0xB8, len(b)]) + b


def rlp_list(items):
    payload = b"".join(items)
    if len(payload) < 56:
        return bytes([0xC0 + len(payload)]) + payload
    assert len(payload) < 256
    return bytes([0xF8, len(payload)]) + payload


def hex_prefix(nibbles, leaf=True):
    flag = (2 if leaf else 0) + (len(nibbles) & 1)
    ns = [flag] + ([] if len(nibbles) & 1 else [0]) + list(nibbles)
    return bytes(ns[i] << 4 | ns[i + 1] for i in range(0, len(ns), 2))


def leaf_node(path_nibbles, value, leaf=True):
    """[hex-prefix path, rlp(value)]: the value is a byte string as it stands"""
    return rlp_list([rlp_string(hex_prefix(path_nibbles, leaf)), rlp_string(rlp_string(value))])


OK, MALFORMED, NOT_A_LEAF, BAD_VALUE, KEY_MISMATCH = range(5)


def _item(node, off, end):
    """(payload offset, payload length, offset after the item) of the string item at off, or None"""
    if off >= end:
        return None
    b = node[off]
    if b < 0x80:
        return off, 1, off + 1
    if b <= 0xB7:
        return off + 1, b - 0x80, off + 1 + b - 0x80
    if b == 0xB8:
        if off + 1 >= end or node[off + 1] < 56:
            return None
        return off + 2, node[off + 1], off + 2 + node[off + 1]
    return None


def decode_leaf(node, key=None):
    """(status, word, n_nibbles) by the rules of include/mp2g.h, judged in their order: structure, prefix, value, key"""
    bad = lambda st: (st, bytes(32), 0)
    n = len(node)
    if n < 1:
        return bad(MALFORMED)
    if 0xC0 <= node[0] <= 0xF7:
        off, length = 1, node[0] - 0xC0
    elif node[0] == 0xF8 and n >= 2 and node[1] >= 56:
        off, length = 2, node[1]
    else:
        return bad(MALFORMED)
    if off + length != n:
        return bad(MALFORMED)
    path = _item(node, off, n)
    if path is None or node[off] > 0xB7 or not 1 <= path[1] <= 33 or path[2] > n:
        return bad(MALFORMED)
    val = _item(node, path[2], n)
    if val is None or val[2] != n:
        return bad(MALFORMED)
    p = node[path[0]:path[0] + path[1]]
    flag = p[0] >> 4
    if flag not in (2, 3):
        return bad(NOT_A_LEAF)
    nibbles = bytes_to_nibbles(p)[1 if flag == 3 else 2:]
    if len(nibbles) > 64:
        return bad(MALFORMED)
    v = node[val[0]:val[0] + val[1]]
    if len(v) == 1 and v[0] < 0x80:
        value = v
    elif len(v) >= 1 and 0x80 <= v[0] <= 0x80 + 32 and len(v) == 1 + v[0] - 0x80:
        value = v[1:]
    else:
        return bad(BAD_VALUE)
    if key is not None and nibbles != bytes_to_nibbles(key)[64 - len(nibbles):]:
        return bad(KEY_MISMATCH)
    return OK, left_pad32(value), len(nibbles)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# 135: the domain byte and the final bit share a byte; 136 / 272: a whole number of rate blocks; 532 = MAX_BRANCH_NODE_LEN
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 134, 135, 136, 137, 271, 272, 273, 532]
COUNTS = [1, 63, 64, 65, 129]  # the wave's edge, more than one block, a grid tail
STRIDE = 536


@functools.lru_cache(maxsize=None)
def message(length, seed=0):
    return np.random.default_rng(0x6ECCA6 + 1000 * seed + length).integers(0, 256, size=length, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """129 messages of all of LENGTHS, shuffled: the lanes of one wave run different block counts"""
    rng = np.random.default_rng(0x6ECCA7)
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(129)]
    rng.shuffle(lens)
    return tuple(message(n, i) for i, n in enumerate(lens))


# mapping keys: all zero, all ff, a single low byte, a 20-byte address left-padded
EDGE_KEYS = [bytes(32), b"\xff" * 32, bytes(31) + b"\x07", bytes(12) + bytes(range(0xA0, 0xB4))]
EVM_OFFSETS = [0, 1, (1 << 32) - 1]


@functools.lru_cache(maxsize=None)
def key_rows(count, n_keys, seed=0x6ECCA8):
    """uint8 [count][n_keys][32]: the edge keys first, then seeded random ones"""
    k = np.random.default_rng(seed + n_keys).integers(0, 256, size=(count, n_keys, 32), dtype=np.uint8)
    for i in range(min(count, len(EDGE_KEYS))):
        for j in range(n_keys):
            k[i, j] = np.frombuffer(EDGE_KEYS[(i + j) % len(EDGE_KEYS)], dtype=np.uint8)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def parent_rows(count, seed=0x6ECCA9):
    """uint8 [count][32]: random parents; row 0 ends in ff..ff below a zero top byte (a carry that crosses every word without
    leaving 256 bits at offset 1), the last row is all ff (offset 1 overflows)"""
    p = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    p[0] = 0xFF
    p[0, 0] = 0
    if count > 1:
        p[-1] = 0xFF
    p.setflags(write=False)
    return p


VALUES = [b"\x05", b"\x80", b"\xff", b"\x12\x34", bytes(range(1, 32)), bytes(range(0xE0, 0x100)), b""]
PATH_LENGTHS = [0, 1, 2, 63, 64]


@functools.lru_cache(maxsize=None)
def leaf_key(i):
    return keccak256(b"leaf key %d" % i)


def _leaf(key, n_nibbles, value):
    return leaf_node(bytes_to_nibbles(key)[64 - n_nibbles:], value)


@functools.lru_cache(maxsize=None)
def good_leaves():
    """[(label, node, key)]: every value form under every path length, and the list header's boundary (payload 55 against 56)"""
    out, i = [], 0
    for v in VALUES:
        for n in PATH_LENGTHS:
            out.append((f"value {v.hex() or 'empty'}, {n} nibbles", _leaf(leaf_key(i), n, v), leaf_key(i)))
            i += 1
    for vlen in (19, 20):  # 34 bytes of path item + 2 + vlen: 55 is the last short list, 56 the first 0xf8 one
        node = _leaf(leaf_key(i), 64, bytes(range(1, vlen + 1)))
        assert len(node) == (1 if vlen == 19 else 2) + 36 + vlen and node[0] == (0xC0 + 55 if vlen == 19 else 0xF8)
        out.append((f"list payload {36 + vlen}", node, leaf_key(i)))
        i += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def damaged_leaves():
    """[(label, node, key, intended status)]: one damage per rule"""
    key = leaf_key(1000)
    nib = bytes_to_nibbles(key)
    good = _leaf(key, 64, b"\x12\x34\x56")
    path, val = rlp_string(hex_prefix(nib)), rlp_string(rlp_string(b"\x12\x34\x56"))
    flipped = list(nib)
    flipped[40] ^= 1
    return (
        ("truncated len", good[:-1], key, MALFORMED),
        ("a trailing byte", good + b"\x00", key, MALFORMED),
        ("three items", rlp_list([path, val, rlp_string(b"\x01")]), key, MALFORMED),
        ("one item", rlp_list([path]), key, MALFORMED),
        ("a list header above 0xf8", bytes([0xF9, 0, len(good) - 1]) + good[1:], key, MALFORMED),
        ("0xf8 with a short payload", bytes([0xF8, len(good) - 1]) + good[1:], key, MALFORMED),
        ("a nested list as the value", rlp_list([path, rlp_list([b"\x01"])]), key, MALFORMED),
        ("65 nibbles", rlp_list([rlp_string(bytes([0x31]) + key), val]), key, MALFORMED),
        ("the empty input", b"", key, MALFORMED),
        ("an extension prefix, even", leaf_node(nib, b"\x12\x34\x56", leaf=False), key, NOT_A_LEAF),
        ("an extension prefix, odd", leaf_node(nib[1:], b"\x12\x34\x56", leaf=False), key, NOT_A_LEAF),
        ("a 33-byte value", _leaf(key, 64, bytes(range(1, 34))), key, BAD_VALUE),
        ("an inner length above the item", rlp_list([path, rlp_string(b"\x84\x12\x34\x56")]), key, BAD_VALUE),
        ("an inner length below the item", rlp_list([path, rlp_string(b"\x82\x12\x34\x56")]), key, BAD_VALUE),
        ("an empty item 1", rlp_list([path, b"\x80"]), key, BAD_VALUE),
        ("one flipped path nibble", leaf_node(flipped, b"\x12\x34\x56"), key, KEY_MISMATCH),
        ("one flipped nibble of a short odd path", leaf_node([nib[61] ^ 8] + nib[62:], b"\x12\x34\x56"), key, KEY_MISMATCH),
    )
