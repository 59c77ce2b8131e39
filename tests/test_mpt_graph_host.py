"""csrc/mpt_graph.cuh compiled for the host into tools/hosttest/mpt_graph_host_test (its own main, no GPU, no library), once with -O2
and once under -fsanitize=address,undefined: the passes that the kernels of csrc/mpt_digest.hip compile, with the plain policy,
against the restatement of tests/mpt_digest_cases.py over every case, forwards and backwards over the proofs, and over hostile
paths and info words. The program keeps every array in a heap block of its own size, so an index past a table is an error under the
sanitizers, not luck. Points are opaque tokens there: the test checks the shape and which leaves feed which node, not the curve."""
import subprocess

import numpy as np
import pytest

import hosttest
import mpt_cases as M
import mpt_digest_cases as D

FLAGS = {"O2": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}


@pytest.fixture(scope="module", params=sorted(FLAGS))
def exe(request, tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("mpt_graph_" + request.param), "mpt_graph_host_test", flags=FLAGS[request.param])


def tokens(count):
    return np.random.default_rng(0x70CE).integers(0, 1 << 64, size=(count, 20), dtype=np.uint64)


def run(exe, tmp, infos, paths, depths, keys, status, max_depth, backwards=False):
    n, count = len(infos), len(depths)
    head = np.array([n, count, max_depth, status is not None, backwards], dtype=np.uint32)
    parts = [head, np.asarray(infos, dtype=np.uint32), np.asarray(paths, dtype=np.uint32).reshape(count, max_depth), np.asarray(depths, dtype=np.uint32),
             np.asarray(keys, dtype=np.uint8).reshape(count, 32)] + ([] if status is None else [np.asarray(status, dtype=np.uint32)]) + [tokens(count)]
    req, res = tmp / "request.bin", tmp / "result.bin"
    req.write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in parts))
    r = subprocess.run([exe, str(req), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw, off, out = res.read_bytes(), 0, {}
    for name, shape, dtype in (("acc", (n, 20), np.uint64), ("n_leaves", (n,), np.uint32), ("state", (n,), np.uint32), ("via", (n,), np.uint32),
                               ("parent", (n,), np.uint32), ("entered", (n,), np.uint8), ("totals", (3,), np.uint32)):
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[name] = np.frombuffer(raw[off:off + size], dtype=dtype).reshape(shape)
        off += size
    assert off == len(raw)
    return out


def token_sums(c, sh):
    """the word-by-word sum of the tokens of the leaves below every OK node, along the restatement's child table"""
    tok, acc = tokens(c.count), np.zeros((len(c.nodes), 20), dtype=np.uint64)
    for x in sorted((x for x in sh["ref"] if x not in sh["conflict"]), key=lambda x: -sh["ref"][x][2]):
        if c.infos[x] & 3 == M.LEAF:
            acc[x] = tok[sh["via"][x]]
        else:
            for s in range(16):
                if (x, s) in sh["child"]:
                    acc[x] += acc[sh["child"][(x, s)]]
    return acc


@pytest.mark.parametrize("name", D.names())
def test_every_case_forwards_and_backwards(exe, tmp_path, name):
    c = D.case(name)
    sh, want = c.want()
    for backwards in (False, True):
        got = run(exe, tmp_path, c.infos, c.paths, c.depths, c.key_rows(), c.status(), c.max_depth, backwards)
        for out in D.SHAPE_OUTPUTS + ("totals",):
            assert np.array_equal(got[out], want[out]), (name, out, backwards)
        assert np.array_equal(got["acc"], token_sums(c, sh)), (name, "which leaves feed which node", backwards)


def test_no_nodes(exe, tmp_path):
    e = D.no_node_case()
    got = run(exe, tmp_path, [], e["paths"], e["depths"], e["keys"], None, 3)
    assert got["totals"].tolist() == e["totals"]


def test_hostile_paths_and_info_words(exe, tmp_path):
    """indices past the table, depths past the row, info words that are not the nodes' (every kind with all other bits set, nibble
    counts up to 127): every pass ends, and under the sanitizers none reads or writes outside a block"""
    c = D.case("damaged paths among good ones, no status")
    n = len(c.nodes)
    rng = np.random.default_rng(0xBAD)
    wild = c.paths.copy()
    wild[::5] = rng.integers(0, 2 * n, size=wild[::5].shape, dtype=np.uint32)
    wild[3::7, 0] = 0xFFFFFFFF
    depths = c.depths.copy()
    depths[1::9] = rng.integers(0, 2 ** 32, size=depths[1::9].shape, dtype=np.uint32)
    for words in [np.array(c.infos, dtype=np.uint32)] + D.hostile_info_words(c.infos):
        for paths, dep in ((c.paths, c.depths), (wild, depths)):
            got = run(exe, tmp_path, words, paths, dep, c.key_rows(), None, c.max_depth)
            assert (got["state"] <= D.CONFLICT).all() and ((got["via"] < c.count) | (got["via"] == D.NO_NODE)).all()
            assert ((got["parent"] < n) | (got["parent"] == D.NO_NODE)).all() and int(got["n_leaves"].max(initial=0)) <= c.count
            want = D.shape([int(w) for w in words], paths, dep, c.keys, None, c.max_depth)
            assert got["totals"][0] == want["n_rejected"] and got["totals"][1] == len(want["conflict"])
