"""The MPT subtree-digest entry points are declared in include/mp2g.h with the widths the Python host binds them with, the library
exports them, the header's constants are the Python ones and those of the checker's restatement, refusals need no device and write
nothing, and the host-side names are importable (no GPU needed)."""
import ctypes
import importlib
import re

import numpy as np
import pytest

import mpt_cases as M
import mpt_digest_cases as D

ABI = importlib.import_module("mapreduce-plonky2_amd._abi")
V, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
PROTOTYPES = {
    "mp2g_mpt_subtree_digests_dev": (I, [V, V, U32, V, V, U32, V, V, U32, V, V, V, V, V, V, V, V]),
    "mp2g_mpt_subtree_digests": (I, [V, V, U32, V, U32, V, V, U32, V, U32, V, U32, U32, V, V, V, V, V, V, V, V, V, V]),
}


def test_prototypes_declared(mp2):
    table = ABI.prototypes(mp2.HEADER_PATH)
    for name, proto in PROTOTYPES.items():
        assert name in table, name
        assert table[name] == proto, name


def test_symbols_exported_and_bound(mp2):
    lib = mp2.load()
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.restype == restype and list(f.argtypes) == argtypes, name


def test_constants_match_the_header_and_the_restatement(mp2):
    text = open(mp2.HEADER_PATH).read()
    for value, name in enumerate(("UNREACHED", "OK", "CONFLICT")):
        assert re.search(rf"MP2G_MPT_SUBTREE_{name} = {value}\b", text) and getattr(mp2, "MPT_SUBTREE_" + name) == value == getattr(D, name), name
    assert "#define MP2G_MPT_NO_NODE 0xffffffffu" in text and mp2.MPT_NO_NODE == D.NO_NODE == 0xFFFFFFFF
    assert mp2.MPT_SUBTREE_OUTPUTS == D.SHAPE_OUTPUTS
    assert "the per-node DV / N sums of the reference's branch circuit." not in text  # the out-of-scope note is gone


def test_refusals_need_no_device_and_write_nothing(mp2):
    """every argument is judged before the context is touched; host memory stands in for device memory: nothing is dereferenced"""
    lib, p = mp2.load(), mp2._p
    n, count, depth = 3, 2, 2
    info, paths, depths, keys = np.zeros(n, dtype=np.uint32), np.zeros((count, depth), dtype=np.uint32), np.ones(count, dtype=np.uint32), np.zeros((count, 32), dtype=np.uint8)
    status, leaf, acc = np.zeros(count, dtype=np.uint32), np.zeros((count + n, 20), dtype=np.uint64), np.zeros((n, 20), dtype=np.uint64)
    outs = [np.full(n, 0x77777777, dtype=np.uint32) for _ in range(4)] + [np.full(n, 0x77, dtype=np.uint8)]
    totals = np.full(3, 0x77777777, dtype=np.uint32)
    off = lambda a, k: ctypes.c_void_p(a.ctypes.data + k)
    good = dict(info=p(info), n=n, paths=p(paths), depths=p(depths), max_depth=depth, keys=p(keys), status=p(status), count=count, leaf=p(leaf),
                acc=p(acc), n_leaves=p(outs[0]), state=p(outs[1]), via=p(outs[2]), parent=p(outs[3]), entered=p(outs[4]))
    changes = [(dict(info=None), "info"), (dict(paths=None), "paths"), (dict(depths=None), "depths"), (dict(keys=None), "mpt_keys"),
               (dict(leaf=None), "leaf_frac"), (dict(max_depth=0), "max_depth"), (dict(max_depth=66), "max_depth"),
               (dict(leaf=off(leaf, 4)), "leaf_frac is not 8-byte"), (dict(acc=off(acc, 4)), "acc_frac is not 8-byte"),
               (dict(info=off(info, 2)), "info is not 4-byte"), (dict(paths=off(paths, 1)), "paths is not 4-byte"),
               (dict(depths=off(depths, 2)), "depths is not 4-byte"), (dict(status=off(status, 2)), "status is not 4-byte"),
               (dict(n_leaves=off(outs[0], 2)), "n_leaves is not 4-byte"), (dict(state=off(outs[1], 1)), "state is not 4-byte"),
               (dict(via=off(outs[2], 2)), "via is not 4-byte"), (dict(parent=off(outs[3], 2)), "parent is not 4-byte"),
               (dict(acc=off(leaf, 160 * (count - 1))), "leaf_frac and acc_frac overlap"), (dict(acc=p(leaf)), "overlap")]
    for change, word in changes:
        a = dict(good, **change)
        assert lib.mp2g_mpt_subtree_digests_dev(None, a["info"], a["n"], a["paths"], a["depths"], a["max_depth"], a["keys"], a["status"], a["count"],
                                                a["leaf"], a["acc"], a["n_leaves"], a["state"], a["via"], a["parent"], a["entered"], p(totals)) != 0, change
        assert word in lib.mp2g_last_error().decode(), (change, lib.mp2g_last_error())
    # sound arguments and no context: refused as well, by name
    a = good
    assert lib.mp2g_mpt_subtree_digests_dev(None, a["info"], n, a["paths"], a["depths"], depth, a["keys"], None, count, a["leaf"], a["acc"], a["n_leaves"],
                                            a["state"], a["via"], a["parent"], a["entered"], p(totals)) != 0 and b"ctx" in lib.mp2g_last_error()
    assert all((o == 0x77777777).all() or (o == 0x77).all() for o in outs) and (totals == 0x77777777).all() and not acc.any()
    # the host form: what the calls it is composed of refuse
    rows, lens = mp2.rows_at_stride([M.node_table()[0][1], M.node_table()[5][1]])
    stride = rows.shape[1]
    leaf_w, roots = np.zeros((count, 5), dtype=np.uint64), np.zeros((1, 32), dtype=np.uint8)
    h_status, w, wei = np.full(count, 0x77777777, dtype=np.uint32), np.full((2, 5), 0x77, dtype=np.uint64), np.full((2, 11), 0x77, dtype=np.uint64)
    houts = [np.full(2, 0x77777777, dtype=np.uint32) for _ in range(4)] + [np.full(2, 0x77, dtype=np.uint8)]
    good = dict(nodes=p(rows), stride=stride, lens=p(lens), n=2, paths=p(paths), depths=p(depths), max_depth=depth, keys=p(keys), count=count,
                roots=p(roots), root_stride=0, mode=0, leaf_w=p(leaf_w))
    long_lens, deep = np.array([3, stride + 1], dtype=np.uint32), np.array([1, 3], dtype=np.uint32)
    for change, word in ((dict(stride=12), "stride"), (dict(nodes=None), "nodes"), (dict(lens=None), "lens"), (dict(lens=p(long_lens)), "lens: entry 1"),
                         (dict(paths=None), "paths"), (dict(depths=None), "depths"), (dict(keys=None), "mpt_keys"), (dict(max_depth=0), "max_depth"),
                         (dict(max_depth=66), "max_depth"), (dict(root_stride=8), "root_stride"), (dict(mode=3), "mode"),
                         (dict(depths=p(deep)), "depths: entry 1 is 3"), (dict(leaf_w=None), "leaf_w")):
        a = dict(good, **change)
        assert lib.mp2g_mpt_subtree_digests(None, a["nodes"], a["stride"], a["lens"], a["n"], a["paths"], a["depths"], a["max_depth"], a["keys"], a["count"],
                                            a["roots"], a["root_stride"], a["mode"], a["leaf_w"], p(h_status), p(w), p(wei), *(p(o) for o in houts),
                                            p(totals)) != 0, change
        assert word in lib.mp2g_last_error().decode(), (change, lib.mp2g_last_error())
    assert (h_status == 0x77777777).all() and (w == 0x77).all() and (wei == 0x77).all() and all((o == 0x77777777).all() or (o == 0x77).all() for o in houts)
    assert (totals == 0x77777777).all()
    # nothing to do is not an error, and needs no context either: no node rejects every proof
    assert lib.mp2g_mpt_subtree_digests_dev(None, None, 0, p(paths), p(depths), depth, p(keys), None, count, None, None, None, None, None, None, None,
                                            p(totals)) == 0 and totals.tolist() == [count, 0, 0]
    assert lib.mp2g_mpt_subtree_digests_dev(None, None, 0, None, None, 1, None, None, 0, None, None, None, None, None, None, None, None) == 0
    assert lib.mp2g_mpt_subtree_digests(None, None, 8, None, 0, p(paths), p(depths), depth, p(keys), 0, None, 0, 0, None, None, None, None, None, None, None,
                                        None, None, p(totals)) == 0 and totals.tolist() == [0, 0, 0]


def test_host_names(mp2):
    X = importlib.import_module("mapreduce-plonky2_amd.extraction")
    for name in ("mpt_subtree_digests", "mpt_subtree_digests_dev"):
        assert callable(getattr(mp2, name)), name
    for name in ("mpt_subtree_digests", "values_extraction_public_inputs", "storage_proof_tree", "storage_proof_words"):
        assert callable(getattr(X, name)), name
    assert X.PUBLIC_INPUT_LEN == 96
    # a proof set by position: the same bytes under two parents are two entries; by bytes they are one
    a, b, c, d = b"root", b"left", b"right", b"leaf"
    s = X.MptProofSet.from_proofs([[a, b, d], [a, c, d], [a, b, d]], by_position=True)
    assert s.nodes == [a, b, d, c, d] and s.paths.tolist() == [[0, 1, 2], [0, 3, 4], [0, 1, 2]]
    assert X.MptProofSet.from_proofs([[a, b, d], [a, c, d]]).nodes == [a, b, d, c]
    with pytest.raises(ValueError, match="one MPT key per proof"):
        X.MptProofSet.from_proofs([[a]], by_position=True, mpt_keys=[], node_info={})
    with pytest.raises(ValueError, match="both the MPT keys and the nodes' info words"):
        X.MptProofSet.from_proofs([[a]], by_position=True, mpt_keys=[bytes(32)])
