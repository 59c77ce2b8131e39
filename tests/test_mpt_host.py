"""csrc/mpt.cuh compiled for the host into tools/hosttest/mpt_host_test (its own main, no GPU, no library), once with -O2 and once
under -fsanitize=address,undefined: the node opener and the walk that the kernels of csrc/mpt.hip compile, against the
restatement of tests/mpt_cases.py over every case and damage table and the hostile-length rows. The program keeps every node in a
heap block of its own size, so a read past a node's row is an error under the sanitizers, not luck."""
import subprocess

import numpy as np
import pytest

import hosttest
import mpt_cases as M

FLAGS = {"O2": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}


@pytest.fixture(scope="module", params=sorted(FLAGS))
def exe(request, tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("mpt_" + request.param), "mpt_host_test", flags=FLAGS[request.param])


def run(exe, tmp, nodes, lens, stride, paths, depths, keys, roots, root_stride, mode, info=None):
    """nodes: byte strings (cut or padded to the stride); lens may exceed the stride; roots: None or uint8 [1 or count][32]"""
    rows = np.zeros((len(nodes), stride), dtype=np.uint8)
    for r, n in zip(rows, nodes):
        r[:min(len(n), stride)] = np.frombuffer(bytes(n)[:stride], dtype=np.uint8)
    count, max_depth = paths.shape
    head = np.array([len(nodes), stride, count, max_depth, root_stride, mode, roots is not None, info is not None], dtype=np.uint32)
    req, res = tmp / "request.bin", tmp / "result.bin"
    req.write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in (head, np.array(lens, dtype=np.uint32), rows, paths.astype(np.uint32),
                                                                       np.asarray(depths, dtype=np.uint32), keys)
                             + (() if roots is None else (roots,)) + (() if info is None else (info.astype(np.uint32),))))
    r = subprocess.run([exe, str(req), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw, off, out = res.read_bytes(), 0, []
    for shape, dtype in (((len(nodes), 32), np.uint8), ((len(nodes),), np.uint32), ((count,), np.uint32), ((count,), np.uint32),
                         ((count, 32), np.uint8), ((count,), np.uint32), ((count,), np.uint32), ((count, max_depth), np.uint8)):
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out.append(np.frombuffer(raw[off:off + size], dtype=dtype).reshape(shape))
        off += size
    assert off == len(raw)
    return out[0], out[1], dict(zip(("status", "fail_level", "words", "val_off", "val_len", "consumed"), out[2:]))


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "hashes")
    assert np.array_equal(got[1], want[1]), (what, "info")
    for name in want[2]:
        assert np.array_equal(got[2][name], want[2][name]), (what, name)


def test_every_batch(exe, tmp_path):
    for b in M.batches():
        lens = [len(n) for n in b.nodes]
        same(run(exe, tmp_path, b.nodes, lens, M.STRIDE, b.paths, b.depths, b.key_rows(), b.root_rows(), 32, b.mode), b.want(), b.name)
    b = M.batches()[0]
    lens = [len(n) for n in b.nodes]
    # one root for all, and no root: nothing is a ROOT_MISMATCH then, and what the first level hashes to goes unchecked
    same(run(exe, tmp_path, b.nodes, lens, M.STRIDE, b.paths, b.depths, b.key_rows(), b.root_rows()[:1], 0, b.mode), b.want(), "one root")
    d = next(b for b in M.batches() if b.name == "damaged paths")
    want = d.want(False)
    assert M.ROOT_MISMATCH not in want[2]["status"] and M.HASH_MISMATCH in want[2]["status"]
    same(run(exe, tmp_path, d.nodes, [len(n) for n in d.nodes], M.STRIDE, d.paths, d.depths, d.key_rows(), None, 0, d.mode), want, "no roots")


def test_node_table_at_the_smallest_stride_of_each_node(exe, tmp_path):
    """every node alone in a row that ends where it ends (rounded up to 8 bytes)"""
    no_paths, no_keys = np.zeros((0, 1), dtype=np.uint32), np.zeros((0, 32), dtype=np.uint8)
    for label, node, info in M.node_table():
        stride = max(8, (len(node) + 7) // 8 * 8)
        hashes, got, _ = run(exe, tmp_path, [node], [len(node)], stride, no_paths, [], no_keys, None, 0, M.RAW)
        assert got.tolist() == [info] and bytes(hashes[0]) == M.K.keccak256(node), label


def test_hostile_lengths_stay_inside_the_row(exe, tmp_path):
    """length bytes, and lengths, that point past the stride: MALFORMED, BAD_NODE on the way, and no read outside a node's block"""
    rows, lens = M.hostile_rows()
    n = len(rows)
    clamped = [r[:min(length, M.HOSTILE_STRIDE)] for r, length in zip(rows, lens)]
    paths = np.arange(n, dtype=np.uint32).reshape(n, 1)
    keys = np.frombuffer(bytes([0x12, 0x34, 0x56]) * (32 * n // 3 + 1), dtype=np.uint8)[:32 * n].reshape(n, 32)
    hashes, info, out = run(exe, tmp_path, rows, lens, M.HOSTILE_STRIDE, paths, [1] * n, keys, None, 0, M.WORD)
    assert info.tolist() == [M.open_node(c) for c in clamped] and [bytes(h) for h in hashes] == [M.K.keccak256(c) for c in clamped]
    assert out["status"].tolist() == [M.BAD_NODE] * (n - 1) + [M.KEY_LENGTH]  # the sound leaf has 6 nibbles at level 0


def test_truncated_tables(exe, tmp_path):
    """every node of the sound batch cut to 1, 2 and 40 bytes: MALFORMED, so every path is BAD_NODE at its root"""
    b = M.batches()[0]
    for cut in (1, 2, 40):
        nodes = [n[:cut] for n in b.nodes]
        hashes, info, out = run(exe, tmp_path, nodes, [len(n) for n in nodes], M.STRIDE, b.paths, b.depths, b.key_rows(), None, 0, b.mode)
        assert info.tolist() == [M.open_node(n) for n in nodes] and (out["status"] == M.BAD_NODE).all() and not out["fail_level"].any()


def test_info_words_that_are_not_the_nodes(exe, tmp_path):
    """the walk trusts no bit of an info word for a read (the _dev form takes the words from its caller): every path of the
    recorded storage proof and of the extension tries walked with each node's word replaced by another node's, by words of every
    kind with all other bits set, and with the nodes' lengths cut under the words. What the statuses are is not the point: every
    walk ends, and under the sanitizers none reads outside a node's block."""
    for b in (M.batches()[1], M.batches()[4], M.batches()[7]):
        info = b.want()[1]
        lens = [len(n) for n in b.nodes]
        foreign = [np.roll(info, 1), np.roll(info, -1), info[::-1].copy()] + [np.full(len(info), 0xFFFFFF80 | k | hl << 5, dtype=np.uint32)
                                                                               for k in (1, 2, 3) for hl in (1, 3)]
        for words in foreign:
            for cut in (None, 3, 34):
                out = run(exe, tmp_path, b.nodes, lens if cut is None else [min(n, cut) for n in lens], M.STRIDE, b.paths, b.depths, b.key_rows(),
                          None, 0, b.mode, info=words)[2]
                assert (out["status"] <= M.BAD_VALUE).all() and (out["fail_level"] < b.max_depth).all()
