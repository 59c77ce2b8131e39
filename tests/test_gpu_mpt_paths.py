"""mp2g_mpt_open_nodes[_dev], mp2g_mpt_verify_paths[_dev] (csrc/mpt.hip, csrc/mpt_api.hip) and extraction.py's MptProofSet /
verify_mpt_proofs / account_storage_roots / storage_proof_words against the restatement of tests/mpt_cases.py (open_node, walk),
bit for bit over every case and damage table, and end to end: the recorded eth_getProof answer from the state root's account leaf
down to the slot's word, and a built mapping against leaf_mapping_values_digests over words and keys the host knows."""
import ctypes
import importlib

import numpy as np
import pytest

import keccak_cases as K
import leaf_digest_cases as LD
import mpt_cases as M

pytestmark = pytest.mark.gpu

X = importlib.import_module("mapreduce-plonky2_amd.extraction")
OUTPUTS = ("status", "fail_level", "words", "val_off", "val_len", "consumed")
GUARD = 2  # rows after the last one of every device output, planted with 0x77 and found so
BATCHES = [b.name for b in M.batches()]


def batch(name):
    return M.batches()[BATCHES.index(name)]


def out_shapes(count, max_depth, extra=GUARD):
    return {"status": ((count + extra,), np.uint32), "fail_level": ((count + extra,), np.uint32), "words": ((count + extra, 32), np.uint8),
            "val_off": ((count + extra,), np.uint32), "val_len": ((count + extra,), np.uint32), "consumed": ((count + extra, max_depth), np.uint8)}


class DeviceTable:
    """a node table on the device with stage 1's outputs, guards planted after their n_nodes rows"""

    def __init__(self, ctx, mp2, nodes, lens=None, stride=M.STRIDE, tail_rows=0, tail=0):
        self.ctx, self.mp2, self.stride = ctx, mp2, stride
        self.rows, own = mp2.rows_at_stride(nodes, stride, fill=0xA5)
        self.lens = own if lens is None else np.array(lens, dtype=np.uint32)
        self.n = len(nodes)
        self.d_rows = ctx.to_device(np.concatenate([self.rows, np.full((tail_rows, stride), tail, dtype=np.uint8)]) if tail_rows else self.rows)
        self.d_lens = ctx.to_device(self.lens)
        self.planted = [np.full((self.n + GUARD, 32), 0x77, dtype=np.uint8), np.full(self.n + GUARD, 0x77777777, dtype=np.uint32)]
        self.d_hashes, self.d_info = (ctx.to_device(a) for a in self.planted)

    def open(self, hashes=True, info=True):
        self.mp2.mpt_open_nodes_dev(self.ctx, self.d_rows, self.stride, self.d_lens, self.n, self.d_hashes if hashes else None,
                                    self.d_info if info else None)
        return self.d_hashes.download(self.planted[0].shape, np.uint8), self.d_info.download(self.planted[1].shape, np.uint32)

    def unchanged(self):
        return np.array_equal(self.d_rows.download(self.rows.shape, np.uint8), self.rows) and \
            np.array_equal(self.d_lens.download(self.lens.shape, np.uint32), self.lens)

    def free(self):
        for d in (self.d_rows, self.d_lens, self.d_hashes, self.d_info):
            d.free()


def walk_dev(ctx, mp2, table, paths, depths, keys, roots, root_stride, mode, pick=OUTPUTS):
    """mp2g_mpt_verify_paths_dev over an opened table: ({name: what the buffer holds after the call, guards included}, whether the
    inputs are as they were); only the outputs named in `pick` are given to the call"""
    count, max_depth = paths.shape
    shapes = out_shapes(count, max_depth)
    d_in = [ctx.to_device(a) for a in (paths, depths, keys)] + [None if roots is None else ctx.to_device(roots)]
    d_out = {name: ctx.to_device(np.full(s, 0x77, dtype=np.uint8).view(t) if t == np.uint8 else np.full(s, 0x77777777, dtype=t))
             for name, (s, t) in shapes.items()}
    mp2.mpt_verify_paths_dev(ctx, table.d_rows, table.stride, table.d_lens, table.d_hashes, table.d_info, table.n, d_in[0], d_in[1], max_depth,
                             d_in[2], count, d_in[3], root_stride, mode, *(d_out[name] if name in pick else None for name in OUTPUTS))
    got = {name: d_out[name].download(*shapes[name]) for name in OUTPUTS}
    same = all(np.array_equal(d.download(a.shape, a.dtype), a) for d, a in zip(d_in, (paths, depths, keys, roots)) if d is not None)
    for d in d_in + list(d_out.values()):
        if d is not None:
            d.free()
    return got, same


def planted(a):
    return (a == (0x77 if a.dtype == np.uint8 else 0x77777777)).all()


def check_walk(got, want, mode, pick=OUTPUTS, what=""):
    count = len(want["status"])
    for name in OUTPUTS:
        written = name in pick and not (name == "words" and mode == M.RAW)  # RAW writes no word
        assert planted(got[name][count:]), (what, name, "guard")
        if written:
            assert np.array_equal(got[name][:count], want[name]), (what, name)
        else:
            assert planted(got[name][:count]), (what, name, "not asked for")


# ---- both stages over every table, host and device forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BATCHES)
def test_batches_host_form(ctx, mp2, name):
    b = batch(name)
    hashes, info, want = b.want()
    got_hashes, got_info = mp2.mpt_open_nodes(ctx, b.nodes, M.STRIDE)
    assert np.array_equal(got_hashes, hashes) and np.array_equal(got_info, info)
    got = mp2.mpt_verify_paths(ctx, b.nodes, b.paths, b.depths, b.key_rows(), b.root_rows(), b.mode, stride=M.STRIDE)
    for out in OUTPUTS:
        assert np.array_equal(got[out], want[out]), out
    assert list(zip(got["status"].tolist(), got["fail_level"].tolist())) == b.intended


@pytest.mark.parametrize("name", BATCHES)
def test_batches_device_form(ctx, mp2, name):
    """counts 1 (the recorded proofs), 65 (the chain) and 129; guards after every output; inputs unchanged"""
    b = batch(name)
    hashes, info, want = b.want()
    t = DeviceTable(ctx, mp2, b.nodes)
    got_hashes, got_info = t.open()
    assert np.array_equal(got_hashes[:t.n], hashes) and np.array_equal(got_info[:t.n], info)
    assert planted(got_hashes[t.n:]) and planted(got_info[t.n:])
    got, same = walk_dev(ctx, mp2, t, b.paths, b.depths, b.key_rows(), b.root_rows(), 32, b.mode)
    check_walk(got, want, b.mode, what=name)
    assert same and t.unchanged()
    t.free()


def test_counts_cover_the_block_edges():
    assert {batch(n).count for n in BATCHES} >= {1, 65, 129} and max(len(batch(n).nodes) for n in BATCHES) > 128


def test_node_table(ctx, mp2):
    """sound nodes by their fields and one damage per reason, in both forms; at the smallest stride that holds them all"""
    table = M.node_table()
    nodes, want = [n for _, n, _ in table], [i for _, _, i in table]
    hashes, info = mp2.mpt_open_nodes(ctx, nodes)
    assert info.tolist() == want and [bytes(h) for h in hashes] == [K.keccak256(n) for n in nodes]
    t = DeviceTable(ctx, mp2, nodes)
    got_hashes, got_info = t.open()
    assert got_info[:t.n].tolist() == want and np.array_equal(got_hashes[:t.n], hashes) and t.unchanged()
    t.free()


def test_each_output_alone(ctx, mp2):
    b = batch("damaged paths")
    hashes, info, want = b.want()
    t = DeviceTable(ctx, mp2, b.nodes)
    got_hashes, got_info = t.open(info=False)
    assert np.array_equal(got_hashes[:t.n], hashes) and planted(got_info)
    t.d_hashes.upload(t.planted[0])
    got_hashes, got_info = t.open(hashes=False)
    assert planted(got_hashes) and np.array_equal(got_info[:t.n], info)
    t.open()
    for name in OUTPUTS:
        got, _ = walk_dev(ctx, mp2, t, b.paths, b.depths, b.key_rows(), b.root_rows(), 32, b.mode, pick=(name,))
        check_walk(got, want, b.mode, pick=(name,), what=name)
    t.free()
    # the host form: every output may be NULL
    lib, p = mp2.load(), mp2._p
    rows, lens = mp2.rows_at_stride(b.nodes, M.STRIDE)
    keys, roots = b.key_rows(), b.root_rows()
    for pick in range(len(OUTPUTS)):
        outs = [np.zeros(s, dtype=d) if j == pick else None for j, (s, d) in enumerate(out_shapes(b.count, b.max_depth, 0).values())]
        assert lib.mp2g_mpt_verify_paths(ctx, p(rows), M.STRIDE, p(lens), len(lens), p(b.paths), p(b.depths), b.max_depth, p(keys), b.count,
                                         p(roots), 32, b.mode, *(None if o is None else p(o) for o in outs)) == 0
        assert np.array_equal(outs[pick], want[OUTPUTS[pick]]), OUTPUTS[pick]


def test_one_root_no_root_and_raw_words(ctx, mp2):
    b = batch("129 random keys")
    want = b.want()[2]
    t = DeviceTable(ctx, mp2, b.nodes)
    t.open()
    got, _ = walk_dev(ctx, mp2, t, b.paths, b.depths, b.key_rows(), b.root_rows()[:1].copy(), 0, b.mode)
    check_walk(got, want, b.mode, what="one root")
    got, _ = walk_dev(ctx, mp2, t, b.paths, b.depths, b.key_rows(), b.root_rows()[:1].copy(), 0, M.RAW)
    check_walk(got, dict(want, words=None), M.RAW, what="raw")
    t.free()
    d = batch("damaged paths")
    want = d.want(False)[2]
    assert M.ROOT_MISMATCH not in want["status"] and M.HASH_MISMATCH in want["status"]
    got = mp2.mpt_verify_paths(ctx, d.nodes, d.paths, d.depths, d.key_rows(), None, d.mode, stride=M.STRIDE)
    assert all(np.array_equal(got[name], want[name]) for name in OUTPUTS)
    t = DeviceTable(ctx, mp2, d.nodes)
    t.open()
    got, _ = walk_dev(ctx, mp2, t, d.paths, d.depths, d.key_rows(), None, 0, d.mode)
    check_walk(got, want, d.mode, what="no roots")
    # a depth above max_depth reaches the device form alone: BAD_PATH at level 0, nothing consumed
    depths = d.depths.copy()
    depths[0] = d.max_depth + 1
    got, _ = walk_dev(ctx, mp2, t, d.paths, depths, d.key_rows(), None, 0, d.mode)
    assert (got["status"][0], got["fail_level"][0]) == (M.BAD_PATH, 0) and (got["consumed"][0] == 0xFF).all() and not got["words"][0].any()
    assert np.array_equal(got["status"][1:d.count], want["status"][1:])
    t.free()


def test_hostile_length_bytes_stay_inside_the_row(ctx, mp2):
    """length bytes, and device lengths, that point past the stride: the node is MALFORMED and a path through it BAD_NODE; the rows
    after the table are not read: they differ between two runs and the outputs do not"""
    rows, lens = M.hostile_rows()
    n = len(rows)
    clamped = [r[:min(length, M.HOSTILE_STRIDE)] for r, length in zip(rows, lens)]
    want_info = [M.open_node(c) for c in clamped]
    assert want_info[:-1] == [M.invalid(M.MALFORMED)] * (n - 1)
    paths, depths = np.arange(n, dtype=np.uint32).reshape(n, 1), np.ones(n, dtype=np.uint32)
    keys = np.frombuffer(K.leaf_key(7) * n, dtype=np.uint8).reshape(n, 32)
    runs = []
    for tail in (0x00, 0xFF):
        t = DeviceTable(ctx, mp2, list(rows), lens=lens, stride=M.HOSTILE_STRIDE, tail_rows=8, tail=tail)
        hashes, info = t.open()
        got, _ = walk_dev(ctx, mp2, t, paths, depths, keys, None, 0, M.WORD)
        runs.append([hashes, info] + [got[name] for name in OUTPUTS])
        t.free()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    hashes, info, status = runs[0][0], runs[0][1], runs[0][2]
    assert info[:n].tolist() == want_info and [bytes(h) for h in hashes[:n]] == [K.keccak256(c) for c in clamped]
    assert status[:n].tolist() == [M.BAD_NODE] * (n - 1) + [M.KEY_LENGTH]


def test_refusals_write_nothing(ctx, mp2):
    lib = mp2.load()
    b = batch("extensions")
    t = DeviceTable(ctx, mp2, b.nodes)
    off = lambda d, k: ctypes.c_void_p(d.ptr.value + k)
    for args, word in (((t.d_rows, 20, t.d_lens), "stride"), ((None, M.STRIDE, t.d_lens), "nodes"), ((t.d_rows, M.STRIDE, None), "lens"),
                       ((off(t.d_rows, 4), M.STRIDE, t.d_lens), "nodes is not 8-byte aligned"), ((t.d_rows, M.STRIDE, off(t.d_lens, 2)), "lens is not 4-byte aligned")):
        assert lib.mp2g_mpt_open_nodes_dev(ctx, *args, t.n, t.d_hashes, t.d_info) != 0
        assert word in lib.mp2g_last_error().decode(), word
    assert lib.mp2g_mpt_open_nodes_dev(ctx, t.d_rows, M.STRIDE, t.d_lens, t.n, off(t.d_hashes, 4), t.d_info) != 0 and b"hashes is not 8-byte" in lib.mp2g_last_error()
    assert lib.mp2g_mpt_open_nodes_dev(ctx, t.d_rows, M.STRIDE, t.d_lens, t.n, t.d_hashes, off(t.d_info, 1)) != 0 and b"info is not 4-byte" in lib.mp2g_last_error()
    ctx.sync()
    assert planted(t.d_hashes.download(t.planted[0].shape, np.uint8)) and planted(t.d_info.download(t.planted[1].shape, np.uint32))
    t.open()
    shapes = out_shapes(b.count, b.max_depth)
    seeds = {name: (np.full(s, 0x77, dtype=d) if d == np.uint8 else np.full(s, 0x77777777, dtype=d)) for name, (s, d) in shapes.items()}
    d_out = {name: ctx.to_device(a) for name, a in seeds.items()}
    d_paths, d_depths, d_keys, d_roots = (ctx.to_device(a) for a in (b.paths, b.depths, b.key_rows(), b.root_rows()))
    good = dict(nodes=t.d_rows, stride=M.STRIDE, lens=t.d_lens, hashes=t.d_hashes, info=t.d_info, paths=d_paths, depths=d_depths,
                max_depth=b.max_depth, keys=d_keys, roots=d_roots, root_stride=32, mode=b.mode, **d_out)
    changes = [(dict(paths=None), "paths"), (dict(depths=None), "depths"), (dict(keys=None), "mpt_keys"), (dict(hashes=None), "hashes"),
               (dict(info=None), "info"), (dict(max_depth=0), "max_depth"), (dict(max_depth=66), "max_depth"), (dict(root_stride=16), "root_stride"),
               (dict(mode=3), "mode"), (dict(stride=12), "stride"), (dict(nodes=off(t.d_rows, 4)), "nodes is not 8-byte"),
               (dict(hashes=off(t.d_hashes, 4)), "hashes is not 8-byte"), (dict(roots=off(d_roots, 4)), "roots is not 8-byte"),
               (dict(words=off(d_out["words"], 4)), "words is not 8-byte"), (dict(paths=off(d_paths, 2)), "paths is not 4-byte"),
               (dict(status=off(d_out["status"], 2)), "status is not 4-byte"), (dict(val_len=off(d_out["val_len"], 1)), "val_len is not 4-byte")]
    for change, word in changes:
        a = dict(good, **change)
        assert lib.mp2g_mpt_verify_paths_dev(ctx, a["nodes"], a["stride"], a["lens"], a["hashes"], a["info"], t.n, a["paths"], a["depths"], a["max_depth"],
                                             a["keys"], b.count, a["roots"], a["root_stride"], a["mode"], *(a[name] for name in OUTPUTS)) != 0, change
        assert word in lib.mp2g_last_error().decode(), (change, lib.mp2g_last_error())
    ctx.sync()
    for name, d in d_out.items():
        assert np.array_equal(d.download(*shapes[name]), seeds[name]), name
    # the host form names the first depth above max_depth and writes nothing
    rows, lens = mp2.rows_at_stride(b.nodes, M.STRIDE)
    status, p = np.full(b.count, 0x77777777, dtype=np.uint32), mp2._p
    deep = b.depths.copy()
    deep[3] = b.max_depth + 1
    assert lib.mp2g_mpt_verify_paths(ctx, p(rows), M.STRIDE, p(lens), len(lens), p(b.paths), p(deep), b.max_depth, p(b.key_rows()), b.count, None, 0,
                                     b.mode, p(status), None, None, None, None, None) != 0
    assert b"depths: entry 3" in lib.mp2g_last_error() and planted(status)
    # count == 0 launches nothing
    assert lib.mp2g_mpt_verify_paths_dev(ctx, t.d_rows, M.STRIDE, t.d_lens, t.d_hashes, t.d_info, t.n, d_paths, d_depths, b.max_depth, d_keys, 0, None, 0,
                                         b.mode, *(d_out[name] for name in OUTPUTS)) == 0
    ctx.sync()
    assert all(np.array_equal(d.download(*shapes[name]), seeds[name]) for name, d in d_out.items())
    for d in [d_paths, d_depths, d_keys, d_roots] + list(d_out.values()):
        d.free()
    t.free()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_recorded_answer_from_the_state_root_to_the_word(ctx, mp2):
    """state root -> account leaf -> storageHash, left on the device and used there as the root of the storage walk -> 0x22b8"""
    answer, _ = M.recorded()
    account = [M.unhex(n) for n in answer["accountProof"]]
    storage = [M.unhex(n) for n in answer["storageProof"][0]["proof"]]
    address = M.unhex(answer["address"])
    d_roots, roots = X.account_storage_roots(ctx, [account], [address], K.keccak256(account[0]))
    assert bytes(roots[0]) == M.unhex(answer["storageHash"])
    slot = X.StorageSlot.simple(8)
    out = X.verify_mpt_proofs(ctx, X.MptProofSet.from_proofs([storage]), [slot.mpt_key(ctx)], d_roots)
    assert out["status"].tolist() == [0] and bytes(out["words"][0]) == K.left_pad32(b"\x22\xb8") and out["consumed"][0].tolist() == [0, 1, 2, 3, 4]
    # the order the reference's circuits use, and a wrong state root
    out = X.verify_mpt_proofs(ctx, X.MptProofSet.from_proofs([storage[::-1]], leaf_first=True), [slot.mpt_key(ctx)], d_roots)
    assert out["status"].tolist() == [0]
    d_roots.free()
    with pytest.raises(ValueError, match=f"account proof 0 .* status {M.ROOT_MISMATCH} at level 0"):
        X.account_storage_roots(ctx, [account], [address], K.keccak256(account[1]))
    with pytest.raises(ValueError, match=f"account proof 0 .* status {M.HASH_MISMATCH} at level 1"):
        X.account_storage_roots(ctx, [account], [address[::-1]], K.keccak256(account[0]))


def test_storage_proof_words_end_to_end(ctx, mp2):
    """a built mapping of 129 entries whose values hold three columns: from the eth_getProof proofs and the mapping keys to the
    values digests on the device, against leaf_mapping_values_digests over the words and keys the host knows"""
    count, slot, key_id = 129, 4, 0x4B4559
    layouts = [(12, 0, 160), (5, 3, 13), (0, 4, 4)]
    info = [X.ColumnInfo(slot, 2001 + c, *lay, 0) for c, lay in enumerate(layouts)]
    ids = [c.identifier for c in info]
    words = LD.words(count)
    keys = [bytes(k[0]).lstrip(b"\0") for k in K.key_rows(count, 1)]  # distinct, and as a caller holds them: not padded
    mpt_keys = [K.mpt_key(K.mapping(k, slot)) for k in keys]
    trie = M.Trie({m: M.storage_value(bytes(w)) for m, w in zip(mpt_keys, words)})
    proofs = [trie.proofs[m] for m in mpt_keys]
    got_words, (w, wei, (sum_w, sum_wei)) = X.storage_proof_words(ctx, proofs, trie.root, slot, [keys], info, ids, [key_id])
    assert np.array_equal(got_words, words)
    want_w, want_wei, (want_sum_w, want_sum_wei) = X.leaf_mapping_values_digests(ctx, info, ids, words, keys, 0, key_id)
    assert np.array_equal(w, want_w) and np.array_equal(wei, want_wei)
    assert np.array_equal(sum_w, want_sum_w) and np.array_equal(sum_wei, want_sum_wei)
    # the root as it lies on the device
    d_root = ctx.to_device(np.frombuffer(trie.root, dtype=np.uint8))
    assert np.array_equal(X.storage_proof_words(ctx, proofs, d_root, slot, [keys], info, ids, [key_id])[0], words)
    d_root.free()
    # one proof's branch swapped for a sound branch of another proof: refused, not digested
    victim = next(i for i, p in enumerate(proofs) if len(p) >= 3)
    donor = next(p for p in proofs if len(p) >= 3 and p[1] != proofs[victim][1])
    swapped = list(proofs)
    swapped[victim] = [proofs[victim][0], donor[1]] + proofs[victim][2:]
    with pytest.raises(ValueError, match=f"storage proof {victim} .* status {M.HASH_MISMATCH} at level 1"):
        X.storage_proof_words(ctx, swapped, trie.root, slot, [keys], info, ids, [key_id])
