"""Case tables for the MPT inclusion-proof kernels (csrc/mpt.cuh, csrc/mpt.hip) and the checker's restatement of include/mp2g.h's
rules in plain Python: open_node (the info word of a node of any kind) and walk (one proof from its root to its leaf), over the
Keccak of tests/keccak_cases.py; a small hexary-trie builder over arbitrary 32-byte keys, which embeds a child whose RLP is under
32 bytes as the protocol does; tries whose every part is the smallest shape at which that part can go wrong; one damage per node
reason and per path status; and the recorded proofs of tests/golden/. No GPU is used here and nothing here calls the code under
test. Every table carries the status it intends, set by its construction; tests/test_mpt_cases.py holds the restatement to them.

The builders are cached: every caller gets the same objects and must leave them unchanged."""
import functools
import json
import os

import numpy as np

import keccak_cases as K

MAX_DEPTH = 65
INVALID, BRANCH, EXTENSION, LEAF = range(4)
MALFORMED, ITEM_COUNT, EMBEDDED_CHILD, BRANCH_VALUE, BAD_PREFIX = range(1, 6)
WORD, ACCOUNT, RAW = range(3)
(OK, BAD_PATH, ROOT_MISMATCH, HASH_MISMATCH, BAD_NODE, LEAF_ABOVE, NO_LEAF, KEY_LENGTH, EMPTY_CHILD, KEY_MISMATCH, BAD_VALUE) = range(11)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIDE = K.STRIDE  # 536: a 532-byte branch node in a row of 8-byte words


# ---- the restatement: a node ----------------------------------------------------------------------------------------------------------
def invalid(reason):
    return INVALID | reason << 2


def _item(node, off, end):
    """(is_list, payload offset, payload length, offset after the item) of the item at off < end, or None: rule 2"""
    b = node[off]
    if b < 0x80:
        it = (False, off, 1)
    elif b <= 0xB7:
        it = (False, off + 1, b - 0x80)
    elif b == 0xB8:
        if off + 1 >= end or node[off + 1] < 56:
            return None
        it = (False, off + 2, node[off + 1])
    elif 0xC0 <= b <= 0xF7:
        it = (True, off + 1, b - 0xC0)
    else:
        return None
    return None if it[1] + it[2] > end else it + (it[1] + it[2],)


def list_header(node):
    """rule 1: the header's length, or 0"""
    n = len(node)
    if n >= 1 and 0xC0 <= node[0] <= 0xF7:
        off, length = 1, node[0] - 0xC0
    elif n >= 2 and node[0] == 0xF8 and node[1] >= 56:
        off, length = 2, node[1]
    elif n >= 3 and node[0] == 0xF9 and (node[1] << 8 | node[2]) >= 256:
        off, length = 3, node[1] << 8 | node[2]
    else:
        return 0
    return off if off + length == n else 0


def open_node(node):
    """the info word of a node, by the header's rules in their order"""
    node = bytes(node)
    hl = list_header(node)
    if not hl:
        return invalid(MALFORMED)
    items, off = [], hl
    while off < len(node):
        if len(items) == 17:
            return invalid(ITEM_COUNT)
        it = _item(node, off, len(node))
        if it is None:
            return invalid(MALFORMED)
        items.append((off,) + it)
        off = it[3]
    if len(items) == 17:
        mask = 0
        for k, (hdr, is_list, p_off, p_len, _) in enumerate(items):
            empty = not is_list and p_len == 0
            if k == 16:
                if not empty:
                    return invalid(BRANCH_VALUE)
            elif not is_list and p_len == 32:
                mask |= 1 << k
            elif not empty:
                return invalid(EMBEDDED_CHILD if is_list else MALFORMED)
        return BRANCH | hl << 5 | mask << 8
    if len(items) != 2:
        return invalid(ITEM_COUNT)
    (_, list0, p_off, p_len, _), (hdr1, list1, _, len1, _) = items
    if list0 or not 1 <= p_len <= 33:
        return invalid(MALFORMED)
    flag = node[p_off] >> 4
    if flag > 3:
        return invalid(BAD_PREFIX)
    nib = 2 * (p_len - 1) + (flag & 1)
    if nib > 64:
        return invalid(MALFORMED)
    if flag < 2:
        if nib < 1:
            return invalid(MALFORMED)
        if list1:
            return invalid(EMBEDDED_CHILD)
        if len1 != 32:
            return invalid(MALFORMED)
        return EXTENSION | hl << 5 | nib << 8 | hdr1 << 16
    if list1:
        return invalid(MALFORMED)
    return LEAF | hl << 5 | nib << 8 | hdr1 << 16


def kind(info):
    return info & 3


def reason(info):
    return info >> 2 & 7


def branch_child_offset(info, k):
    """where the 32 bytes of the child at nibble k start: the mask trick the walk relies on"""
    return (info >> 5 & 3) + k + 32 * bin(info >> 8 & 0xFFFF & ((1 << k) - 1)).count("1") + 1


def path_nibbles(node, info):
    """the nibbles of an extension's or a leaf's hex-prefix path"""
    hl, nib = info >> 5 & 3, info >> 8 & 0x7F
    p_off = hl + (node[hl] >= 0x80)
    p = K.bytes_to_nibbles(node[p_off:p_off + (nib + 2) // 2])
    return p[2 - (nib & 1):]


def leaf_value(payload, mode):
    """(sound, word) of a leaf's item-1 payload under a value mode"""
    if mode == RAW:
        return True, bytes(32)
    if mode == WORD:
        if len(payload) == 1 and payload[0] < 0x80:
            return True, K.left_pad32(payload)
        if len(payload) >= 1 and 0x80 <= payload[0] <= 0x80 + 32 and len(payload) == 1 + payload[0] - 0x80:
            return True, K.left_pad32(payload[1:])
        return False, bytes(32)
    bad = (False, bytes(32))
    n = len(payload)
    if n >= 1 and 0xC0 <= payload[0] <= 0xF7 and 1 + payload[0] - 0xC0 == n:
        off = 1
    elif n >= 2 and payload[0] == 0xF8 and payload[1] >= 56 and 2 + payload[1] == n:
        off = 2
    else:
        return bad
    items = []
    for k in range(4):
        it = _item(payload, off, n) if off < n else None
        if it is None or it[0] or (k >= 2 and it[2] != 32):
            return bad
        items.append(payload[it[1]:it[1] + it[2]])
        off = it[3]
    return (True, items[2]) if off == n else bad


def walk(nodes, hashes, infos, path, depth, key, root, mode, max_depth):
    """one proof by the header's steps in their order: dict of status, fail_level, word, val_off, val_len, consumed"""
    consumed = [0xFF] * max_depth
    fail = lambda status, level: dict(status=status, fail_level=level, word=bytes(32), val_off=0, val_len=0, consumed=bytes(consumed))
    if not 1 <= depth <= max_depth:
        return fail(BAD_PATH, 0)
    ptr, expected = 0, root
    nib_of = K.bytes_to_nibbles(key)
    for level in range(depth):
        consumed[level] = ptr
        idx = path[level]
        if idx >= len(nodes):
            return fail(BAD_PATH, level)
        if expected is not None and hashes[idx] != expected:
            return fail(HASH_MISMATCH if level else ROOT_MISMATCH, level)
        node, info = nodes[idx], infos[idx]
        last = level + 1 == depth
        if kind(info) == INVALID:
            return fail(BAD_NODE, level)
        if kind(info) == LEAF and not last:
            return fail(LEAF_ABOVE, level)
        if kind(info) != LEAF and last:
            return fail(NO_LEAF, level)
        if kind(info) == BRANCH:
            if ptr == 64:
                return fail(KEY_LENGTH, level)
            k = nib_of[ptr]
            if not info >> 8 + k & 1:
                return fail(EMPTY_CHILD, level)
            off = branch_child_offset(info, k)
            expected, ptr = node[off:off + 32], ptr + 1
            continue
        p, i1 = path_nibbles(node, info), info >> 16
        if kind(info) == EXTENSION:
            if ptr + len(p) > 64:
                return fail(KEY_LENGTH, level)
            if p != nib_of[ptr:ptr + len(p)]:
                return fail(KEY_MISMATCH, level)
            expected, ptr = node[i1 + 1:i1 + 33], ptr + len(p)
            continue
        if ptr + len(p) != 64:
            return fail(KEY_LENGTH, level)
        if p != nib_of[ptr:]:
            return fail(KEY_MISMATCH, level)
        _, v_off, v_len, _ = _item(node, i1, len(node))
        sound, word = leaf_value(node[v_off:v_off + v_len], mode)
        if not sound:
            return fail(BAD_VALUE, level)
        return dict(status=OK, fail_level=0, word=word, val_off=v_off, val_len=v_len, consumed=bytes(consumed))
    raise AssertionError("the last level either fails or is a leaf")


# ---- RLP and the trie builder -------------------------------------------------------------------------------------------------------
def rlp_list(items):
    payload = b"".join(items)
    if len(payload) < 56:
        return bytes([0xC0 + len(payload)]) + payload
    if len(payload) < 256:
        return bytes([0xF8, len(payload)]) + payload
    return bytes([0xF9, len(payload) >> 8, len(payload) & 0xFF]) + payload


def reference_to(node):
    """how a parent holds a child: its hash, or the child itself when its RLP is under 32 bytes"""
    return node if len(node) < 32 else K.rlp_string(K.keccak256(node))


def leaf(path, stored):
    return rlp_list([K.rlp_string(K.hex_prefix(path, True)), K.rlp_string(stored)])


def extension(path, child_item):
    return rlp_list([K.rlp_string(K.hex_prefix(path, False)), child_item])


def branch(children, value=b"\x80"):
    """children: 16 items (b"\\x80" where there is none)"""
    return rlp_list(list(children) + [value])


def _build(entries, depth):
    """entries: [(nibbles, key, stored)] sorted, all sharing their first `depth` nibbles. Returns (the node's RLP, {key: the hashed
    nodes from this one down to the key's leaf}): an embedded node is part of its parent, not an entry of its own"""
    if len(entries) == 1:
        nib, key, stored = entries[0]
        node = leaf(nib[depth:], stored)
        return node, {key: [node]}
    first, last = entries[0][0], entries[-1][0]
    shared = 0
    while first[depth + shared] == last[depth + shared]:  # sorted: what the first and the last share, all share
        shared += 1
    if shared:
        subs = [_build(entries, depth + shared)]
        node = extension(first[depth:depth + shared], reference_to(subs[0][0]))
    else:
        subs = [_build(sub, depth + 1) for sub in ([e for e in entries if e[0][depth] == k] for k in range(16)) if sub]
        refs = {K.bytes_to_nibbles(next(iter(proofs)))[depth]: reference_to(child) for child, proofs in subs}
        node = branch([refs.get(k, b"\x80") for k in range(16)])
    return node, {key: [node] + (p if len(child) >= 32 else []) for child, proofs in subs for key, p in proofs.items()}


class Trie:
    """root hash, and proofs[key]: the nodes an eth_getProof answer lists for the key, the root first"""

    def __init__(self, entries):
        """entries: {32-byte key: what the leaf stores as item 1's payload}"""
        rows = sorted((K.bytes_to_nibbles(k), k, v) for k, v in entries.items())
        self.root_node, self.proofs = _build(rows, 0) if rows else (b"\x80", {})
        self.root = K.keccak256(self.root_node)
        self.keys = [r[1] for r in rows]


def storage_value(v):
    """what a storage leaf stores of a value: the RLP of the value without its leading zero bytes"""
    return K.rlp_string(bytes(v).lstrip(b"\0"))


# ---- batches: a node table, paths into it, and what every path is intended to give --------------------------------------------------
class Batch:
    """rows: [(label, proof, key, root, (status, fail_level))]. A proof is a list of nodes, the root first; an entry None stands for
    the index n_nodes, which names no node; (proof, depth) gives a depth other than the proof's length."""

    def __init__(self, name, mode, rows, max_depth=None):
        self.name, self.mode, self.labels = name, mode, [r[0] for r in rows]
        proofs = [r[1] if isinstance(r[1], tuple) else (r[1], len(r[1])) for r in rows]
        self.keys, self.roots, self.intended = [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows]
        index = {}
        for proof, _ in proofs:
            for node in proof:
                if node is not None:
                    index.setdefault(node, len(index))
        self.nodes = list(index)
        self.max_depth = max_depth or max(1, max(len(p) for p, _ in proofs))
        self.depths = np.array([d for _, d in proofs], dtype=np.uint32)
        self.paths = np.zeros((len(rows), self.max_depth), dtype=np.uint32)
        for i, (proof, _) in enumerate(proofs):
            self.paths[i, :len(proof)] = [len(self.nodes) if node is None else index[node] for node in proof]
        self.count = len(rows)

    def key_rows(self):
        return np.frombuffer(b"".join(self.keys), dtype=np.uint8).reshape(self.count, 32)

    def root_rows(self):
        return np.frombuffer(b"".join(self.roots), dtype=np.uint8).reshape(self.count, 32)

    @functools.lru_cache(maxsize=None)
    def want(self, with_roots=True):
        """what the restatement gives: (hashes [n_nodes][32], info [n_nodes], {output name: array})"""
        hashes, infos = [K.keccak256(n) for n in self.nodes], [open_node(n) for n in self.nodes]
        got = [walk(self.nodes, hashes, infos, [int(x) for x in self.paths[i]], int(self.depths[i]), self.keys[i],
                    self.roots[i] if with_roots else None, self.mode, self.max_depth) for i in range(self.count)]
        col = lambda name: np.array([g[name] for g in got], dtype=np.uint32)
        as_bytes = lambda name, w: np.frombuffer(b"".join(g[name] for g in got), dtype=np.uint8).reshape(self.count, w)
        return (np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(len(hashes), 32), np.array(infos, dtype=np.uint32),
                {"status": col("status"), "fail_level": col("fail_level"), "words": as_bytes("word", 32), "val_off": col("val_off"),
                 "val_len": col("val_len"), "consumed": as_bytes("consumed", self.max_depth)})


def value32(i, size=32):
    """a value of `size` bytes without a leading zero byte"""
    return (b"\x9a" + K.keccak256(b"mpt value %d" % i))[:size]


def key_with(prefix, seed):
    """a 32-byte key that starts with the nibbles `prefix` and goes on with those of a seeded hash"""
    nib = list(prefix) + K.bytes_to_nibbles(K.keccak256(b"mpt filler %d" % seed))[len(prefix):]
    return bytes(nib[i] << 4 | nib[i + 1] for i in range(0, 64, 2))


def with_nibble(key, pos, value):
    nib = K.bytes_to_nibbles(key)
    nib[pos] = value
    return key_with(nib, 0)


def _all_ok(trie):
    return [(f"key {k.hex()[:8]}", trie.proofs[k], k, trie.root, (OK, 0)) for k in trie.keys]


@functools.lru_cache(maxsize=None)
def random_trie():
    """129 random keys: a full root, sparse second-level branches, lanes of one wave at different depths"""
    keys = [K.keccak256(b"mpt key %d" % i) for i in range(129)]
    return Trie({k: storage_value(K.VALUES[i % len(K.VALUES)]) for i, k in enumerate(keys)})


# (name, key prefixes, value sizes, the (kind, path nibbles) of every node on the first key's proof)
EXTENSION_SHAPES = (
    ("a 1-nibble extension at the root", [[1, 0], [1, 5], [1, 9]], 32, [(EXTENSION, 1), (BRANCH, None), (LEAF, 62)]),
    ("a 2-nibble extension at the root", [[10, 11, 1], [10, 11, 2]], 32, [(EXTENSION, 2), (BRANCH, None), (LEAF, 61)]),
    ("a 2-nibble extension below a branch", [[2, 3, 4, 0], [2, 3, 4, 7], [8]], 32, [(BRANCH, None), (EXTENSION, 2), (BRANCH, None), (LEAF, 60)]),
    ("a 1-nibble extension below a branch", [[1, 5, 0], [1, 5, 9], [7]], 32, [(BRANCH, None), (EXTENSION, 1), (BRANCH, None), (LEAF, 61)]),
    ("a 62-nibble extension", None, 32, [(EXTENSION, 62), (BRANCH, None), (LEAF, 1)]),
    ("a 63-nibble extension, two leaves with empty paths", None, (31, 32), [(EXTENSION, 63), (BRANCH, None), (LEAF, 0)]),
)


@functools.lru_cache(maxsize=None)
def extension_tries():
    """[(name, trie, shape)]: extensions of 1, 2, 62 and 63 nibbles, odd and even, at the root and below a branch; the last is two keys
    that differ only in their last nibble, their values of 31 and 32 bytes so that the leaves are not embedded"""
    out = []
    for t, (name, prefixes, sizes, shape) in enumerate(EXTENSION_SHAPES):
        if prefixes is None:
            first = key_with([], 100 + t)
            share = shape[0][1]
            keys = [first, with_nibble(first, share, K.bytes_to_nibbles(first)[share] ^ 5)]
        else:
            keys = [key_with(p, 10 * t + j) for j, p in enumerate(prefixes)]
        sizes = sizes if isinstance(sizes, tuple) else (sizes,) * len(keys)
        out.append((name, Trie({k: storage_value(value32(10 * t + j, sizes[j])) for j, k in enumerate(keys)}), shape))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain_trie():
    """65 keys where key j + 1 shares exactly j nibbles with key 0: a path of 64 branches and a leaf with an empty path, so that ptr
    reaches 64 only at the leaf"""
    first = K.keccak256(b"mpt chain")
    keys = [first] + [with_nibble(first, j, K.bytes_to_nibbles(first)[j] ^ 8) for j in range(64)]
    return Trie({k: storage_value(value32(200 + j)) for j, k in enumerate(keys)})


@functools.lru_cache(maxsize=None)
def embedded_trie():
    """two keys that differ in their last nibble, one with a one-byte value: its leaf is 3 bytes and lies inside the branch"""
    first = key_with([], 300)
    return Trie({first: storage_value(b"\x05"), with_nibble(first, 63, K.bytes_to_nibbles(first)[63] ^ 1): storage_value(value32(300))})


@functools.lru_cache(maxsize=None)
def recorded():
    """the recorded answers of tests/golden/: (eth_getProof answer, three-node proof)"""
    load = lambda name: json.load(open(os.path.join(GOLDEN_DIR, name)))
    return load("eip1186_account_proof.json"), load("mpt_three_node_proof.json")


def unhex(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


def recorded_rows():
    """{name: (mode, row)} of the three recorded proofs, with the figures the issue quotes"""
    answer, three = recorded()
    account = [unhex(n) for n in answer["accountProof"]]
    storage = [unhex(n) for n in answer["storageProof"][0]["proof"]]
    slot_key = K.keccak256(K.left_pad32(unhex("0x08")))
    nodes3 = [unhex(n) for n in three["proof_root_first"]]
    return {
        "account": (ACCOUNT, ("the recorded account proof", account, K.keccak256(unhex(answer["address"])), K.keccak256(account[0]), (OK, 0))),
        "storage": (WORD, ("the recorded storage proof of slot 8", storage, slot_key, unhex(answer["storageHash"]), (OK, 0))),
        "three raw": (RAW, ("extension, branch, leaf", nodes3, unhex(three["key"]), K.keccak256(nodes3[0]), (OK, 0))),
        "three word": (WORD, ("extension, branch, leaf: a bare 32-byte value", nodes3, unhex(three["key"]), K.keccak256(nodes3[0]), (BAD_VALUE, 2))),
    }


def account_value(i, items=4, hash_len=32):
    strings = [K.rlp_string(bytes([i + 1])), K.rlp_string(b"" if i % 2 else b"\x0d\xe0\xb6\xb3\xa7\x64"), K.rlp_string(value32(400 + i, hash_len)),
               K.rlp_string(value32(500 + i))]
    return rlp_list(strings[:items])


@functools.lru_cache(maxsize=None)
def account_trie():
    """five accounts: three sound, one of three items, one whose storage hash has 31 bytes"""
    keys = [K.keccak256(b"mpt account %d" % i) for i in range(5)]
    values = [account_value(0), account_value(1), account_value(2), account_value(3, items=3), account_value(4, hash_len=31)]
    return Trie(dict(zip(keys, values))), keys


def _key_length_rows():
    """hand-made paths whose hashes chain but whose nibbles do not add up to 64"""
    key = key_with([], 600)
    nib = K.bytes_to_nibbles(key)
    short_leaf = leaf(nib[2:], storage_value(value32(600)))  # 62 nibbles at the root
    rows = [("a leaf of 62 nibbles at the root", [short_leaf], key, K.keccak256(short_leaf), (KEY_LENGTH, 0))]
    e63 = extension(nib[1:64], K.rlp_string(K.keccak256(short_leaf)))
    e2 = extension(nib[:2], K.rlp_string(K.keccak256(e63)))
    rows.append(("an extension of 63 nibbles after 2", [e2, e63, short_leaf], key, K.keccak256(e2), (KEY_LENGTH, 1)))
    deep = leaf([], storage_value(value32(601)))
    b2 = branch([K.rlp_string(K.keccak256(deep)) if k == 3 else b"\x80" for k in range(16)])
    b1 = branch([K.rlp_string(K.keccak256(b2)) if k == nib[63] else b"\x80" for k in range(16)])
    top = extension(nib[:63], K.rlp_string(K.keccak256(b1)))
    rows.append(("a branch after 64 nibbles", [top, b1, b2, deep], key, K.keccak256(top), (KEY_LENGTH, 2)))
    return rows


@functools.lru_cache(maxsize=None)
def damaged_path_rows():
    """one damage per path status, in WORD mode; every intended (status, level) follows from how the row is made"""
    t = random_trie()
    nibbles = {k: K.bytes_to_nibbles(k) for k in t.keys}
    assert {n[0] for n in nibbles.values()} == set(range(16))  # the root is full: a flipped first nibble finds another child
    deep = next(k for k in t.keys if len(t.proofs[k]) >= 3)  # level 1 is a branch
    other = next(k for k in t.keys if nibbles[k][0] != nibbles[deep][0])
    free = next(v for v in range(16) if not any(n[0] == nibbles[deep][0] and n[1] == v for n in nibbles.values()))
    p, d = t.proofs[deep], len(t.proofs[deep])
    ext_name, ext_trie, _ = extension_tries()[2]
    ext_key = ext_trie.keys[0]
    big = Trie({key_with([j], 700 + j): K.rlp_string(value32(700 + j, 33 if j == 1 else 32)) for j in range(3)})
    rows = [
        ("a sound proof", p, deep, t.root, (OK, 0)),
        ("a wrong root", p, deep, K.keccak256(b"not the root"), (ROOT_MISMATCH, 0)),
        ("a node swapped for a sound node of another path", [p[0], t.proofs[other][1]] + p[2:], deep, t.root, (HASH_MISMATCH, 1)),
        ("the key's first nibble flipped under a full branch", p, with_nibble(deep, 0, nibbles[deep][0] ^ 1), t.root, (HASH_MISMATCH, 1)),
        ("the key's second nibble sent to an empty child", p, with_nibble(deep, 1, free), t.root, (EMPTY_CHILD, 1)),
        ("a key nibble flipped inside an extension", ext_trie.proofs[ext_key], with_nibble(ext_key, 2, K.bytes_to_nibbles(ext_key)[2] ^ 1),
         ext_trie.root, (KEY_MISMATCH, 1)),
        ("a key nibble flipped inside the leaf's path", p, with_nibble(deep, 63, nibbles[deep][63] ^ 1), t.root, (KEY_MISMATCH, d - 1)),
        ("a path cut one short", p[:-1], deep, t.root, (NO_LEAF, d - 2)),
        ("the leaf repeated", p + [p[-1]], deep, t.root, (LEAF_ABOVE, d - 1)),
        ("an index equal to n_nodes", [p[0], None] + p[2:], deep, t.root, (BAD_PATH, 1)),
        ("depth 0", (p, 0), deep, t.root, (BAD_PATH, 0)),
        ("a 33-byte value", big.proofs[big.keys[1]], big.keys[1], big.root, (BAD_VALUE, 1)),
        ("beside the 33-byte value", big.proofs[big.keys[0]], big.keys[0], big.root, (OK, 0)),
    ] + _key_length_rows()
    e = embedded_trie()
    rows += [(f"an embedded child on the way, key {j}", e.proofs[k], k, e.root, (BAD_NODE, 1)) for j, k in enumerate(e.keys)]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def batches():
    """every case table as a batch: the built tries (every proof OK), the recorded proofs, the damaged paths"""
    rec = recorded_rows()
    acc, acc_keys = account_trie()
    ext_rows = [(f"{name}: {r[0]}",) + r[1:] for name, trie, _ in extension_tries() for r in _all_ok(trie)]
    return (
        Batch("129 random keys", WORD, _all_ok(random_trie())),
        Batch("extensions", WORD, ext_rows),
        Batch("a 65-node path", WORD, _all_ok(chain_trie())),
        Batch("recorded account proof", ACCOUNT, [rec["account"][1]]),
        Batch("recorded storage proof", WORD, [rec["storage"][1]]),
        Batch("recorded three nodes, raw", RAW, [rec["three raw"][1]]),
        Batch("recorded three nodes, word", WORD, [rec["three word"][1]]),
        Batch("damaged paths", WORD, list(damaged_path_rows())),
        Batch("accounts", ACCOUNT, [(f"account {i}", acc.proofs[k], k, acc.root, (OK, 0) if i < 3 else (BAD_VALUE, len(acc.proofs[k]) - 1))
                                    for i, k in enumerate(acc_keys)]),
    )


# ---- nodes: sound ones with what they are, and one damage per reason ----------------------------------------------------------------
def child(i):
    return K.rlp_string(K.keccak256(b"mpt child %d" % i))


def sparse(present, fill=None):
    return [(fill or child)(k) if k in present else b"\x80" for k in range(16)]


@functools.lru_cache(maxsize=None)
def node_table():
    """[(label, node, intended info word)]: sound nodes by their fields, damaged ones by their reason"""
    good = branch(sparse({1, 4, 15}))
    payload = good[2:]
    path = K.rlp_string(K.hex_prefix([7, 8, 9], False))
    small = leaf([1, 2, 3], storage_value(value32(800)))
    full = branch(sparse(set(range(16))))
    assert len(full) == 532 and full[:3] == bytes([0xF9, 0x02, 0x11]) and good[0] == 0xF8 and len(payload) < 256
    bad = lambda r: invalid(r)
    return (
        ("a branch of three children", good, BRANCH | 2 << 5 | (1 << 1 | 1 << 4 | 1 << 15) << 8),
        ("a full branch of 532 bytes", full, BRANCH | 3 << 5 | 0xFFFF << 8),
        ("an empty branch", branch(sparse(set())), BRANCH | 1 << 5),
        ("an extension of 3 nibbles", extension([7, 8, 9], child(0)), EXTENSION | 1 << 5 | 3 << 8 | 4 << 16),
        ("an extension of 64 nibbles", extension(K.bytes_to_nibbles(K.leaf_key(0)), child(0)), EXTENSION | 2 << 5 | 64 << 8 | 36 << 16),
        ("a leaf of 3 nibbles", small, LEAF | 1 << 5 | 3 << 8 | 4 << 16),
        ("a leaf with an empty path", leaf([], storage_value(b"\x05")), LEAF | 1 << 5 | 0 << 8 | 2 << 16),
        ("a leaf of one odd nibble", leaf([9], storage_value(b"\x05")), LEAF | 1 << 5 | 1 << 8 | 2 << 16),
        ("a truncated node", good[:-1], bad(MALFORMED)),
        ("a trailing byte", good + b"\x00", bad(MALFORMED)),
        ("the empty input", b"", bad(MALFORMED)),
        ("16 items", rlp_list(sparse({1, 4, 15})), bad(ITEM_COUNT)),
        ("18 items", rlp_list(sparse({1, 4, 15}) + [b"\x80", b"\x80"]), bad(ITEM_COUNT)),
        ("19 items, the last one bad: the scan has ended", rlp_list(sparse({1}) + [b"\x80", b"\x80", b"\xb9"]), bad(ITEM_COUNT)),
        ("one item", rlp_list([path]), bad(ITEM_COUNT)),
        ("three items", rlp_list([path, child(0), child(1)]), bad(ITEM_COUNT)),
        ("the empty list", b"\xc0", bad(ITEM_COUNT)),
        ("a 31-byte child", branch(sparse({1, 4}, lambda k: K.rlp_string(K.keccak256(b"x")[:31]))), bad(MALFORMED)),
        ("a one-byte child", branch(sparse({4}, lambda k: b"\x05")), bad(MALFORMED)),
        ("a list child", branch(sparse({1, 4}, lambda k: leaf([], b"\x05") if k == 4 else child(k))), bad(EMBEDDED_CHILD)),
        ("a list child before a 31-byte one: the first decides", branch(sparse({1, 4}, lambda k: leaf([], b"\x05") if k == 1 else K.rlp_string(bytes(31)))),
         bad(EMBEDDED_CHILD)),
        ("a non-empty item 16", branch(sparse({1, 4, 15}), K.rlp_string(b"\x01\x02")), bad(BRANCH_VALUE)),
        ("a list as item 16", branch(sparse({1, 4, 15}), b"\xc0"), bad(BRANCH_VALUE)),
        ("a zero-nibble extension", extension([], child(0)), bad(MALFORMED)),
        ("prefix nibble 4", rlp_list([K.rlp_string(b"\x40\x12"), child(0)]), bad(BAD_PREFIX)),
        ("prefix nibble f", rlp_list([K.rlp_string(b"\xf1"), child(0)]), bad(BAD_PREFIX)),
        ("65 nibbles", rlp_list([K.rlp_string(b"\x31" + K.leaf_key(0)), child(0)]), bad(MALFORMED)),
        ("a path of 34 bytes", rlp_list([K.rlp_string(b"\x20" + K.leaf_key(0) + b"\x01"), child(0)]), bad(MALFORMED)),
        ("a list as item 0", rlp_list([b"\xc1\x20", child(0)]), bad(MALFORMED)),
        ("an extension that embeds its child", extension([7, 8, 9], leaf([], b"\x05")), bad(EMBEDDED_CHILD)),
        ("an extension with a 31-byte item 1", extension([7, 8, 9], K.rlp_string(bytes(range(31)))), bad(MALFORMED)),
        ("a leaf with a list as item 1", rlp_list([K.rlp_string(K.hex_prefix([1, 2, 3])), rlp_list([b"\x01"])]), bad(MALFORMED)),
        ("f8 with a payload below 56", bytes([0xF8, len(small) - 1]) + small[1:], bad(MALFORMED)),
        ("f9 with a payload below 256", bytes([0xF9, 0, len(payload)]) + payload, bad(MALFORMED)),
        ("fa", bytes([0xFA, 0, 2, 0x11]) + full[3:], bad(MALFORMED)),
        ("an item header b9", rlp_list([path, b"\xb9\x00\x20" + bytes(32)]), bad(MALFORMED)),
        ("b8 with a length below 56", rlp_list([path, b"\xb8\x20" + bytes(32)]), bad(MALFORMED)),
        ("an item that runs past the payload", bytes([0xC0 + len(path) + 32]) + path + b"\xa0" + bytes(31), bad(MALFORMED)),
    )


HOSTILE_STRIDE = 40


@functools.lru_cache(maxsize=None)
def hostile_rows():
    """(rows [n][40], device lengths): length bytes that point past the stride, in every header form and item form; some lengths are
    themselves above the stride, which only the device forms take and clamp. The last row is sound."""
    good = leaf([1, 2, 3, 4, 5, 6], storage_value(b"\x12\x34"))
    rows = [
        bytes([0xF8, 0xFF]) + bytes(38),                        # a list that claims 255 bytes
        bytes([0xF9, 0xFF, 0xFF]) + bytes(37),                  # ... 65535 bytes
        bytes([0xF9, 0x02, 0x11, 0xA0]) + bytes(36),            # a real branch's header over a 40-byte row
        bytes([0xC0 + 39, 0xB7]) + bytes(38),                   # a first item that claims 55 bytes
        bytes([0xC0 + 39, 0xB8, 0xFF]) + bytes(37),             # ... 255 bytes in the long form
        bytes([0xC0 + 39, 0x83, 0x20, 1, 2, 0xB8, 0xFF]) + bytes(33),  # a second item that does
        bytes([0xC0 + 39]) + bytes([0x80] * 16) + bytes([0xA0]) + bytes(22),  # a seventeenth item that runs past the row
        bytes([0xC0 + 39, 0x87, 0x00, 1, 2, 3, 4, 5, 6, 0xA0]) + bytes(30),  # an extension whose hash would end two bytes past the row
        bytes([0xC0 + 39, 0x83, 0x20, 1, 2, 0xF7]) + bytes(34),  # a list item that claims 55 bytes
        good + bytes(HOSTILE_STRIDE - len(good)),
    ]
    assert all(len(r) == HOSTILE_STRIDE for r in rows)
    lens = [HOSTILE_STRIDE] * len(rows)
    lens[1], lens[4], lens[-1] = 65535, HOSTILE_STRIDE + 100, len(good)
    return tuple(rows), tuple(lens)
