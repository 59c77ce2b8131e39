"""mp2g_storage_slot_keys[_dev], mp2g_mpt_storage_leaves[_dev] (csrc/storage.hip, csrc/storage_api.hip) and extraction.py's
StorageSlot / storage_leaf_words against the restatement of tests/keccak_cases.py (StorageSlot::location / mpt_key / mpt_nibbles,
the leaf decode with the header's status rules), bit for bit, and end to end against leaf_mapping_values_digests over words and
keys the host knows."""
import ctypes
import importlib

import numpy as np
import pytest

import keccak_cases as K
import leaf_digest_cases as LD

pytestmark = pytest.mark.gpu

X = importlib.import_module("mapreduce-plonky2_amd.extraction")
MAX64 = (1 << 64) - 1


def want_slot_keys(slot, parents, keys, n_keys, evm_offset, count):
    rows = [K.slot_keys(slot, None if parents is None else bytes(parents[i]), [bytes(keys[i, j]) for j in range(n_keys)], evm_offset)
            for i in range(count)]
    as_array = lambda col, w: np.frombuffer(b"".join(r[col] for r in rows), dtype=np.uint8).reshape(count, w)
    return as_array(0, 32), as_array(1, 32), as_array(2, 64), sum(r[3] for r in rows)


def check_slot_keys(ctx, mp2, slot, parents, n_keys, evm_offset, count):
    keys = K.key_rows(count, n_keys) if n_keys else None
    want = want_slot_keys(slot, parents, keys, n_keys, evm_offset, count)
    loc, key, nib, over = mp2.storage_slot_keys(ctx, slot, keys, n_keys, evm_offset, parents, count)
    assert np.array_equal(loc, want[0]) and np.array_equal(key, want[1]) and np.array_equal(nib, want[2]) and over == want[3]
    return want


# ---- slot keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 65, 129])
@pytest.mark.parametrize("n_keys", [0, 1, 2])
def test_slot_keys(ctx, mp2, count, n_keys):
    """with and without parents, every evm_offset; with parents and offset 1 the last leaf (all ff) overflows and is zeroed, the
    first (00 ff..ff) carries through every word"""
    for evm_offset in K.EVM_OFFSETS:
        check_slot_keys(ctx, mp2, 0xFF if n_keys else 0x0123456789ABCDEF, None, n_keys, evm_offset, count)
        want = check_slot_keys(ctx, mp2, 0, K.parent_rows(count), n_keys, evm_offset, count)
        if n_keys == 0 and evm_offset == 1:
            assert bytes(want[0][0]) == b"\x01" + bytes(31)
            assert want[3] == (1 if count > 1 else 0) and (count == 1 or not want[0][-1].any() and not want[1][-1].any() and not want[2][-1].any())


def test_slot_carry_chains(ctx, mp2):
    loc, key, nib, over = mp2.storage_slot_keys(ctx, MAX64, evm_offset=1)
    assert bytes(loc[0]) == bytes(23) + b"\x01" + bytes(8) and over == 0 and bytes(key[0]) == K.keccak256(bytes(loc[0]))
    loc, _, _, over = mp2.storage_slot_keys(ctx, MAX64, evm_offset=(1 << 32) - 1)
    assert int.from_bytes(bytes(loc[0]), "big") == MAX64 + (1 << 32) - 1 and over == 0
    parents = np.full((3, 32), 0xFF, dtype=np.uint8)
    parents[1, 31] = 0xFE
    parents[2, 0] = 0
    loc, key, nib, over = mp2.storage_slot_keys(ctx, 0, evm_offset=1, parents=parents)
    assert over == 1 and not loc[0].any() and not key[0].any() and not nib[0].any()
    assert bytes(loc[1]) == b"\xff" * 32 and bytes(loc[2]) == b"\x01" + bytes(31) and bytes(key[2]) == K.keccak256(bytes(loc[2]))
    assert bytes(nib[2]) == bytes(K.bytes_to_nibbles(bytes(key[2])))


def test_golden_mapping_location_and_storage_slot(ctx, mp2):
    want = bytes.fromhex(K.GOLDEN["mapping_key0_slot0_location_hex"])
    S = X.StorageSlot
    assert S.mapping(b"", 0).location(ctx) == want and bytes(mp2.storage_slot_keys(ctx, 0, [bytes(32)], 1)[0][0]) == want
    addr = bytes(range(0xA0, 0xB4))
    for mine, theirs in ((S.simple(7), K.simple(7)), (S.simple(MAX64), K.simple(MAX64)), (S.mapping(addr, 3), K.mapping(addr, 3)),
                         (S.node_mapping(S.mapping(addr, 3), b"\x05"), K.new_mapping(K.mapping(addr, 3), b"\x05")),
                         (S.node_struct(S.node_mapping(S.mapping(addr, 3), b"\x05"), 2), K.node_struct(K.node_mapping(K.mapping(addr, 3), b"\x05"), 2)),
                         (S.node_struct(S.simple(9), (1 << 32) - 1), K.node_struct(K.simple(9), (1 << 32) - 1))):
        assert (mine.location(ctx), mine.mpt_key(ctx), mine.mpt_nibbles(ctx)) == (K.location(theirs), K.mpt_key(theirs), K.mpt_nibbles(theirs))
    with pytest.raises(OverflowError):
        S.node_struct(_AllOnes(), 1).location(ctx)  # the reference's checked_add(..).unwrap()


class _AllOnes:
    """a parent whose location is 2^256 - 1"""

    def location(self, ctx):
        return b"\xff" * 32


def test_two_calls_chained_through_parents(ctx, mp2):
    """a mapping below a struct's field below a mapping: Node(Mapping(Node(Struct(Mapping)), key)), the first call's locations being
    the second call's parents, on the device"""
    count, slot, off = 65, 6, 3
    outer, inner = K.key_rows(count, 1), K.key_rows(count, 1, 0x6ECCB0)
    d_outer, d_inner, d_loc = ctx.to_device(outer), ctx.to_device(inner), ctx.alloc(32 * count)
    d_loc2, d_key, d_nib = ctx.alloc(32 * count), ctx.alloc(32 * count), ctx.alloc(64 * count)
    assert mp2.storage_slot_keys_dev(ctx, slot, None, d_outer, 1, off, count, d_loc, None, None) == 0
    assert mp2.storage_slot_keys_dev(ctx, 0, d_loc, d_inner, 1, 0, count, d_loc2, d_key, d_nib, overflow=False) is None
    loc, key, nib = d_loc2.download((count, 32), np.uint8), d_key.download((count, 32), np.uint8), d_nib.download((count, 64), np.uint8)
    for i in range(count):
        s = K.node_mapping(K.node_struct(K.mapping(bytes(outer[i, 0]), slot), off), bytes(inner[i, 0]))
        assert (bytes(loc[i]), bytes(key[i]), list(nib[i])) == (K.location(s), K.mpt_key(s), K.mpt_nibbles(s)), i
    assert np.array_equal(d_outer.download(outer.shape, np.uint8), outer) and np.array_equal(d_inner.download(inner.shape, np.uint8), inner)
    for d in (d_outer, d_inner, d_loc, d_loc2, d_key, d_nib):
        d.free()


def test_slot_keys_outputs_are_optional_and_refusals_write_nothing(ctx, mp2):
    lib, p = mp2.load(), mp2._p
    count = 65
    keys = K.key_rows(count, 2)
    want = want_slot_keys(5, None, keys, 2, 1, count)
    for pick in range(3):
        outs = [np.full((count, w), 0x77, dtype=np.uint8) if j == pick else None for j, w in enumerate((32, 32, 64))]
        assert lib.mp2g_storage_slot_keys(ctx, 5, None, p(keys), 2, 1, count, *(None if o is None else p(o) for o in outs), None) == 0
        assert np.array_equal(outs[pick], want[pick])
    over = ctypes.c_uint32(9)
    assert lib.mp2g_storage_slot_keys(ctx, 5, None, p(keys), 2, 1, count, None, None, None, ctypes.byref(over)) == 0 and over.value == 0
    # the guard after `count` rows of every device output
    d_keys = ctx.to_device(keys)
    planted = [np.full((count + 2, w), 0x77, dtype=np.uint8) for w in (32, 32, 64)]
    d_outs = [ctx.to_device(a) for a in planted]
    assert mp2.storage_slot_keys_dev(ctx, 5, None, d_keys, 2, 1, count, *d_outs) == 0
    for d, a, w in zip(d_outs, planted, want):
        got = d.download(a.shape, np.uint8)
        assert np.array_equal(got[:count], w) and (got[count:] == 0x77).all()
    # refusals
    for d, a in zip(d_outs, planted):
        d.upload(a)
    loc = np.full((count, 32), 0x77, dtype=np.uint8)
    over = ctypes.c_uint32(9)
    for args, word in (((256, None, p(keys), 1), "slot"), ((MAX64, None, p(keys), 2), "slot"), ((0, None, p(keys), 3), "n_keys"), ((0, None, None, 1), "keys")):
        assert lib.mp2g_storage_slot_keys(ctx, *args, 0, count, p(loc), None, None, ctypes.byref(over)) != 0
        assert word in lib.mp2g_last_error().decode() and (loc == 0x77).all() and over.value == 9
    for args, word in (((256, None, d_keys, 1), "slot"), ((0, None, d_keys, 3), "n_keys"), ((0, None, None, 2), "keys"),
                       ((0, None, ctypes.c_void_p(d_keys.ptr.value + 4), 1), "keys is not 8-byte aligned"),
                       ((0, ctypes.c_void_p(d_keys.ptr.value + 2), d_keys, 1), "parents is not 8-byte aligned")):
        assert lib.mp2g_storage_slot_keys_dev(ctx, *args, 0, count, *d_outs, ctypes.byref(over)) != 0
        assert word in lib.mp2g_last_error().decode() and over.value == 9
    assert lib.mp2g_storage_slot_keys_dev(ctx, 0, None, d_keys, 1, 0, count, ctypes.c_void_p(d_outs[0].ptr.value + 1), None, None, None) != 0
    for d, a in zip(d_outs, planted):
        assert np.array_equal(d.download(a.shape, np.uint8), a)
    # slot 256 is a simple slot's right, and any slot is fine under parents; count == 0 zeroes the counter
    assert lib.mp2g_storage_slot_keys(ctx, 256, None, None, 0, 0, 1, p(loc), None, None, None) == 0 and bytes(loc[0]) == bytes(30) + b"\x01\x00"
    assert lib.mp2g_storage_slot_keys_dev(ctx, MAX64, d_outs[0], d_keys, 1, 0, count, None, None, None, None) == 0
    assert lib.mp2g_storage_slot_keys(None, 0, None, None, 0, 0, 0, None, None, None, ctypes.byref(over)) == 0 and over.value == 0
    ctx.sync()
    for d in [d_keys] + d_outs:
        d.free()


# ---- leaves -----------------------------------------------------------------------------------------------------------------------------
def all_leaves():
    good, bad = K.good_leaves(), K.damaged_leaves()
    nodes = [g[1] for g in good] + [b[1] for b in bad]
    keys = [g[2] for g in good] + [b[2] for b in bad]
    return nodes, keys, [K.OK] * len(good) + [b[3] for b in bad]


def want_leaves(nodes, keys):
    dec = [K.decode_leaf(n, None if keys is None else k) for n, k in zip(nodes, keys if keys is not None else nodes)]
    hashes = np.frombuffer(b"".join(K.keccak256(bytes(n)) for n in nodes), dtype=np.uint8).reshape(len(nodes), 32)
    words = np.frombuffer(b"".join(d[1] for d in dec), dtype=np.uint8).reshape(len(nodes), 32)
    return hashes, words, np.array([d[2] for d in dec], dtype=np.uint32), np.array([d[0] for d in dec], dtype=np.uint32)


def test_leaf_lattice_and_one_damage_per_status(ctx, mp2):
    """every value form under every path length, the list header's boundary, and every damaged leaf; hashes are right for all"""
    nodes, keys, intended = all_leaves()
    assert len(nodes) > 50  # more than one wave would be 64: see test_leaves_device_form for the block's edge
    want = want_leaves(nodes, keys)
    assert want[3].tolist() == intended
    got = mp2.mpt_storage_leaves(ctx, nodes, keys)
    for g, w, name in zip(got, want, ("hashes", "words", "n_nibbles", "status")):
        assert np.array_equal(g, w), name
    # without keys nothing is a mismatch: those leaves are sound
    want = want_leaves(nodes, None)
    got = mp2.mpt_storage_leaves(ctx, nodes)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and K.KEY_MISMATCH not in got[3]


def test_leaves_device_form(ctx, mp2):
    """129 leaves (the lattice repeated): two blocks and a tail; guards after every output; inputs unchanged; outputs optional"""
    nodes, keys, _ = all_leaves()
    nodes, keys = (nodes * 3)[:129], (keys * 3)[:129]
    count = 129
    want = want_leaves(nodes, keys)
    rows, lens = mp2.rows_at_stride(nodes, 72, fill=0xA5)
    karr = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(count, 32)
    d_rows, d_lens, d_keys = ctx.to_device(rows), ctx.to_device(lens), ctx.to_device(karr)
    shapes = [((count + 2, 32), np.uint8), ((count + 2, 32), np.uint8), ((count + 2,), np.uint32), ((count + 2,), np.uint32)]
    planted = [np.full(s, 0x77, dtype=t) for s, t in shapes]
    d_outs = [ctx.to_device(a) for a in planted]
    mp2.mpt_storage_leaves_dev(ctx, d_rows, 72, d_lens, d_keys, count, *d_outs)
    for d, a, w, (s, t) in zip(d_outs, planted, want, shapes):
        got = d.download(s, t)
        assert np.array_equal(got[:count], w) and np.array_equal(got[count:], a[count:])
    assert np.array_equal(d_rows.download(rows.shape, np.uint8), rows) and np.array_equal(d_keys.download(karr.shape, np.uint8), karr)
    for pick in range(4):
        for d, a in zip(d_outs, planted):
            d.upload(a)
        mp2.mpt_storage_leaves_dev(ctx, d_rows, 72, d_lens, d_keys, count, *(d if j == pick else None for j, d in enumerate(d_outs)))
        for j, (d, a, w, (s, t)) in enumerate(zip(d_outs, planted, want, shapes)):
            assert np.array_equal(d.download(s, t)[:count], w if j == pick else a[:count])
    for d in [d_rows, d_lens, d_keys] + d_outs:
        d.free()


def test_hostile_length_bytes_stay_inside_the_row(ctx, mp2):
    """length bytes that point past the stride give MALFORMED, and the rows after the batch are not read: they differ between two
    runs and the outputs do not"""
    stride = 40
    key = K.leaf_key(7)
    good = K.leaf_node(K.bytes_to_nibbles(key)[64 - 6:], b"\x12\x34")
    hostile = [
        bytes([0xF8, 0xFF]) + bytes(38),                  # a list that claims 255 bytes
        bytes([0xC0 + 39, 0xB7]) + bytes(38),             # a path item that claims 55 bytes
        bytes([0xC0 + 39, 0x83, 0x20, 1, 2, 0xB7]) + bytes(34),  # a value item that claims 55 bytes
        bytes([0xC0 + 39, 0x83, 0x20, 1, 2, 0xB8, 0xFF]) + bytes(33),  # ... 255 bytes in the long form
        bytes([0xC0 + 39, 0x83, 0x20, 1, 2, 0xA2, 0xA0]) + bytes(33),  # an inner string of 32 bytes where 33 are left: 34-byte item
        good + bytes(40 - len(good)),
    ]
    assert all(len(h) == stride for h in hostile)
    rows = np.frombuffer(b"".join(hostile), dtype=np.uint8).reshape(len(hostile), stride)
    # the device form alone takes lengths above the stride: they are clamped to it
    lens = np.array([stride, stride, stride, stride + 100, stride, len(good)], dtype=np.uint32)
    want = want_leaves([bytes(r[:min(n, stride)]) for r, n in zip(rows, lens)], [key] * len(hostile))
    assert want[3].tolist() == [K.MALFORMED] * 4 + [K.BAD_VALUE, K.OK]
    outs = []
    for tail in (0x00, 0xFF):
        d_rows = ctx.to_device(np.concatenate([rows, np.full((8, stride), tail, dtype=np.uint8)]))
        d_lens, d_keys = ctx.to_device(lens), ctx.to_device(np.frombuffer(key * len(hostile), dtype=np.uint8))
        d_outs = [ctx.alloc(32 * len(hostile)), ctx.alloc(32 * len(hostile)), ctx.alloc(4 * len(hostile)), ctx.alloc(4 * len(hostile))]
        mp2.mpt_storage_leaves_dev(ctx, d_rows, stride, d_lens, d_keys, len(hostile), *d_outs)
        outs.append([d.download(w.shape, w.dtype) for d, w in zip(d_outs, want)])
        for d in [d_rows, d_lens, d_keys] + d_outs:
            d.free()
    for a, b, w in zip(outs[0], outs[1], want):
        assert np.array_equal(a, w) and np.array_equal(b, w)


def test_leaves_refusals_write_nothing(ctx, mp2):
    lib, p = mp2.load(), mp2._p
    rows, lens = mp2.rows_at_stride([K.good_leaves()[0][1], K.good_leaves()[1][1]], 16)
    outs = [np.full((2, 32), 0x77, dtype=np.uint8), np.full((2, 32), 0x77, dtype=np.uint8), np.full(2, 0x77, dtype=np.uint32), np.full(2, 0x77, dtype=np.uint32)]
    d_rows, d_lens, d_out = ctx.to_device(rows), ctx.to_device(lens), ctx.to_device(outs[0])
    long_lens = np.array([3, 17], dtype=np.uint32)
    for args, word in (((p(rows), 0, p(lens)), "stride"), ((p(rows), 12, p(lens)), "stride"), ((p(rows), 65544, p(lens)), "stride"),
                       ((None, 16, p(lens)), "nodes"), ((p(rows), 16, None), "lens"), ((p(rows), 16, p(long_lens)), "lens: entry 1")):
        assert lib.mp2g_mpt_storage_leaves(ctx, *args, None, 2, *(p(o) for o in outs)) != 0
        assert word in lib.mp2g_last_error().decode() and all((o == 0x77).all() for o in outs)
    for args, word in (((d_rows, 20, d_lens), "stride"), ((None, 16, d_lens), "nodes"), ((d_rows, 16, None), "lens"),
                       ((ctypes.c_void_p(d_rows.ptr.value + 4), 16, d_lens), "nodes is not 8-byte aligned")):
        assert lib.mp2g_mpt_storage_leaves_dev(ctx, *args, None, 2, d_out, None, None, None) != 0
        assert word in lib.mp2g_last_error().decode()
    assert lib.mp2g_mpt_storage_leaves_dev(ctx, d_rows, 16, d_lens, None, 2, ctypes.c_void_p(d_out.ptr.value + 4), None, None, None) != 0
    assert b"hashes is not 8-byte aligned" in lib.mp2g_last_error()
    assert lib.mp2g_mpt_storage_leaves_dev(ctx, d_rows, 16, d_lens, None, 2, None, ctypes.c_void_p(d_out.ptr.value + 4), None, None) != 0
    assert b"words is not 8-byte aligned" in lib.mp2g_last_error()
    assert lib.mp2g_mpt_storage_leaves_dev(ctx, d_rows, 16, d_lens, None, 2, None, None, ctypes.c_void_p(d_out.ptr.value + 2), None) != 0
    assert b"not 4-byte aligned" in lib.mp2g_last_error()
    assert np.array_equal(d_out.download((2, 32), np.uint8), outs[0])
    assert lib.mp2g_mpt_storage_leaves_dev(ctx, None, 16, None, None, 0, None, None, None, None) == 0
    for d in (d_rows, d_lens, d_out):
        d.free()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_storage_leaf_words_end_to_end(ctx, mp2):
    """a synthetic mapping of 129 entries whose values hold three columns: from the raw leaf nodes and the mapping keys to the values
    digests on the device, against leaf_mapping_values_digests over the words and keys the host knows"""
    count, slot, key_id = 129, 4, 0x4B4559
    layouts = [(12, 0, 160), (5, 3, 13), (0, 4, 4)]
    info = [X.ColumnInfo(slot, 2001 + c, *lay, 0) for c, lay in enumerate(layouts)]
    ids = [c.identifier for c in info]
    words = LD.words(count)
    keys = [bytes(k[0]).lstrip(b"\0") for k in LD.keys(count, 1)]  # as a caller holds them: not padded
    nodes = []
    for i in range(count):
        mpt = K.mpt_key(K.mapping(keys[i], slot))
        # what a trie stores: the value without its leading zero bytes, under the tail of the key that its depth leaves
        nodes.append(K.leaf_node(K.bytes_to_nibbles(mpt)[i % 7:], bytes(words[i]).lstrip(b"\0")))
    hashes, got_words, (w, wei, (sum_w, sum_wei)) = X.storage_leaf_words(ctx, nodes, slot, [keys], info, ids, [key_id])
    assert np.array_equal(got_words, words)
    assert [bytes(h) for h in hashes] == [K.keccak256(n) for n in nodes]
    want_w, want_wei, (want_sum_w, want_sum_wei) = X.leaf_mapping_values_digests(ctx, info, ids, words, keys, 0, key_id)
    assert np.array_equal(w, want_w) and np.array_equal(wei, want_wei)
    assert np.array_equal(sum_w, want_sum_w) and np.array_equal(sum_wei, want_sum_wei)
    # a node under another leaf's key is refused, not digested
    with pytest.raises(ValueError, match="node 0 .* status 4"):
        X.storage_leaf_words(ctx, nodes[1:2] + nodes[1:], slot, [keys], info, ids, [key_id])
