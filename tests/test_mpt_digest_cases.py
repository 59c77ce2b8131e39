"""The case tables of tests/mpt_digest_cases.py held to what they intend, on the CPU alone: the bottom-up restatement against the
oracle's sum over the leaves below every node's position, the leaf counts, the key pointer, the conflict cases flagging exactly the
nodes they are about, and the shapes the cases claim (no GPU needed; nothing here calls the library's kernels)."""
import importlib

import numpy as np
import pytest

import ec_cases as EC
import keccak_cases as K
import mpt_cases as M
import mpt_digest_cases as D

X = importlib.import_module("mapreduce-plonky2_amd.extraction")


@pytest.mark.parametrize("name", D.names())
def test_sums_are_the_leaves_below_each_position(name):
    c = D.case(name)
    sh, out = c.want()
    if c.intended_conflicts is None:
        return
    intended = {int(c.paths[row, level]) for row, level in c.intended_conflicts}
    assert sh["conflict"] == intended, (name, sorted(sh["conflict"]))
    assert out["totals"].tolist() == [c.count - len(sh["occ"]), len(intended), 1 + max((o[2] for o in sh["ref"].values()), default=-1)]
    for x in range(len(c.nodes)):
        if x not in sh["ref"]:
            assert out["state"][x] == D.UNREACHED and out["n_leaves"][x] == 0 and not out["w"][x].any()
            continue
        if x in intended:
            assert out["state"][x] == D.CONFLICT and out["n_leaves"][x] == 0 and not out["w"][x].any()
            continue
        # the leaves below x: one per leaf node, taken from the lowest proof through it, of the proofs that pass through x
        below = {}
        for i in sorted(sh["occ"]):
            if any(o[0] == x for o in sh["occ"][i]):
                below.setdefault(sh["occ"][i][-1][0], i)
        entered = int(out["entered"][x])
        prefix = K.bytes_to_nibbles(c.keys[sh["via"][x]])[:entered]
        assert all(K.bytes_to_nibbles(c.keys[i])[:entered] == prefix for i in below.values()), (name, x)
        w, wei = EC.orc_sum(c.points[sorted(below.values())])
        assert np.array_equal(out["w"][x], w) and np.array_equal(out["weierstrass"][x], wei), (name, x)
        assert out["n_leaves"][x] == len(below) and out["state"][x] == D.OK, (name, x)
    roots = [x for x, o in sh["ref"].items() if o[1] == D.NO_NODE]
    ok_leaves = {o[-1][0] for o in sh["occ"].values() if o[-1][0] not in sh["conflict"]}
    if not intended:
        assert sum(int(out["n_leaves"][x]) for x in roots) == len(ok_leaves), name


@pytest.mark.parametrize("name", D.names())
def test_public_input_rows(name):
    """H, K, T, DV, DM, N where public_inputs.rs:23-36 puts them; T counts from the leaf's end and is p - 1 at a root"""
    c = D.case(name)
    sh, out = c.want()
    n = len(c.nodes)
    dm = np.arange(11, dtype=np.uint64) + 5
    hashes = np.frombuffer(b"".join(c.hashes), dtype=np.uint8).reshape(n, 32)
    rows = X.values_extraction_public_inputs(hashes, c.infos, c.key_rows(), out, dm)
    assert rows.shape == (n, 96) and rows.dtype == np.uint64
    for x in range(n):
        assert rows[x, :8].tolist() == [int.from_bytes(c.hashes[x][4 * j:4 * j + 4], "little") for j in range(8)]
        assert np.array_equal(rows[x, 73:84], out["weierstrass"][x]) and np.array_equal(rows[x, 84:95], dm) and rows[x, 95] == out["n_leaves"][x]
        if x not in sh["ref"]:
            assert not rows[x, 8:73].any()
            continue
        _, parent, _, entered, _ = sh["ref"][x]
        assert rows[x, 8:72].tolist() == K.bytes_to_nibbles(c.keys[sh["via"][x]])
        # 63 minus the nibbles of the node and of everything below it on the way to the leaf
        assert int(rows[x, 72]) == (63 - (64 - entered)) % D.P
        if parent == D.NO_NODE:
            assert int(rows[x, 72]) == D.P - 1
    assert np.array_equal(X.values_extraction_public_inputs(hashes, c.infos, c.key_rows(), out)[:, 84:95], np.tile(EC.NEUTRAL_WEI, (n, 1)))


def test_the_cases_are_the_shapes_they_claim():
    widths = lambda c: np.bincount([o[2] for o in c.want()[0]["ref"].values()]).tolist()
    assert widths(D.case("300 keys, wide levels")) == D.WIDE_LEVELS
    assert widths(D.case("a 65-node path")) == [1] + [2] * 64 and D.case("a 65-node path").max_depth == 65
    assert D.case("129 random keys").infos[0] >> 8 & 0xFFFF == 0xFFFF  # a full 16-child root
    assert len(D.case("one proof of depth 1").nodes) == 1
    sh, out = D.case("P and -P under one branch").want()
    assert not out["w"][0].any() and out["n_leaves"][0] == 2 and out["state"][0] == D.OK  # neutral by cancellation, not by conflict
    sh, out = D.case("P and P under one branch").want()
    assert np.array_equal(out["w"][0], EC.orc_sum(np.stack([EC.base_points(1)[0]] * 2))[0])
    ext = {c.name: sorted({i >> 8 & 0x7F for i in c.infos if i & 3 == M.EXTENSION}) for c in D.cases() if c.name.startswith("extension trie")}
    assert sorted(sum(ext.values(), [])) == [1, 1, 2, 2, 62, 63]
    third = D.case("every third proof of the random trie")
    assert third.count == 43 and len(third.nodes) == len(D.case("129 random keys").nodes) and (third.want()[1]["state"] == D.UNREACHED).any()
    assert third.want()[1]["n_leaves"][0] == 43
    twice = D.case("a proof listed twice")
    assert twice.want()[1]["n_leaves"].tolist() == [2, 1, 1] and twice.want()[1]["via"].tolist() == [0, 0, 1]
    forest = D.case("two tries in one table").want()
    assert len([x for x, o in forest[0]["ref"].items() if o[1] == D.NO_NODE]) == 2 and not forest[0]["conflict"]
    assert (D.case("no proof").want()[1]["state"] == D.UNREACHED).all() and D.case("no proof").want()[1]["totals"].tolist() == [0, 0, 0]


def test_twins_and_copies():
    by_bytes, by_position, copies = D.case("twin leaves, nodes by bytes"), D.case("twin leaves, nodes by position"), D.case("one node under two indices")
    assert len(by_bytes.nodes) == 3 and len(by_position.nodes) == 4
    sh, out = by_bytes.want()
    assert out["state"].tolist() == [D.CONFLICT, D.CONFLICT, D.OK] and out["n_leaves"].tolist() == [0, 0, 1]
    sh, out = by_position.want()
    assert not sh["conflict"] and out["n_leaves"].tolist() == [3, 1, 1, 1]
    # the twins' digests differ although their nodes are the same bytes: the point is the proof's, not the node's
    assert by_position.nodes[1] == by_position.nodes[2] and not np.array_equal(out["w"][1], out["w"][2])
    sh, out = copies.want()
    assert out["state"].tolist() == [D.CONFLICT, D.OK, D.OK, D.OK] and sh["child"][(0, 3)] == 1 and copies.nodes[1] == copies.nodes[2]
    # the library's own proof sets name the nodes as the cases do
    words = lambda c: {n: M.open_node(n) for n in c.nodes}
    assert X.MptProofSet.from_proofs(by_bytes.proofs).nodes == by_bytes.nodes
    s = X.MptProofSet.from_proofs(by_position.proofs, by_position=True, mpt_keys=by_position.keys, node_info=words(by_position))
    assert s.nodes == by_position.nodes and np.array_equal(s.paths, by_position.paths) and np.array_equal(s.depths, by_position.depths)
    # without the keys the twins have one parent and the same bytes: one entry, and the conflict is reported
    assert X.MptProofSet.from_proofs(by_position.proofs, by_position=True).nodes == by_bytes.nodes
    with pytest.raises(ValueError, match="both the MPT keys and the nodes' info words"):
        X.MptProofSet.from_proofs(by_position.proofs, by_position=True, mpt_keys=by_position.keys)
    # held to a definition of its own: a node's position is the key's nibbles before it. An index of the set names one
    # (position, bytes) and every (position, bytes) one index
    for c in (by_position, D.case("129 random keys"), D.case("a 65-node path"), D.case("two tries in one table")) + \
            tuple(c for c in D.cases() if c.name.startswith("extension trie")):
        s = X.MptProofSet.from_proofs(c.proofs, by_position=True, mpt_keys=c.keys, node_info=words(c))
        named = {}
        for i, proof in enumerate(c.proofs):
            nib, ptr = K.bytes_to_nibbles(c.keys[i]), 0
            for level, node in enumerate(proof):
                named.setdefault(int(s.paths[i, level]), set()).add((proof[0], tuple(nib[:ptr]), node))
                ptr += D.own_nibbles(M.open_node(node))
        assert all(len(v) == 1 for v in named.values()) and len({next(iter(v)) for v in named.values()}) == len(named) == len(s.nodes), c.name
        assert all(s.nodes[x] == next(iter(v))[2] for x, v in named.items())
        if c is not by_position:
            assert s.nodes == c.nodes and np.array_equal(s.paths, c.paths)  # a real trie: position and bytes name the same nodes


def test_what_the_shape_refuses_without_a_status():
    real, blind = D.case("damaged paths among good ones, real status"), D.case("damaged paths among good ones, no status")
    _, labels = D._mixed_rows()
    assert blind.status() is None and not real.want()[0]["conflict"]
    assert sorted(real.want()[0]["occ"]) == [i for i in range(real.count) if real.real_status()[i] == M.OK]
    occ = blind.want()[0]["occ"]
    for label in D.MIXED_REJECTED_WITHOUT_STATUS:
        assert labels.index(label) not in occ, label
    for label in D.MIXED_ACCEPTED_WITHOUT_STATUS:
        assert labels.index(label) in occ, label
    assert all(i in occ for i, label in enumerate(labels) if label.startswith("good"))
    hostile = D.case("a status that claims OK for hostile paths")
    sh, out = hostile.want()
    assert sorted(sh["occ"]) == list(range(hostile.count - 4)) and out["totals"][0] == 4 and not sh["conflict"]
    assert hostile.paths[hostile.count - 4, 1] == len(hostile.nodes) and hostile.depths[-2:].tolist() == [0, hostile.max_depth + 1]


def test_acceptance_trusts_no_info_word():
    """whatever the info words claim, acceptance ends, names no node past the table and lets ptr pass 64 nowhere"""
    c = D.case("extension trie 2: " + M.EXTENSION_SHAPES[2][0])
    for words in D.hostile_info_words(c.infos):
        sh = D.shape([int(w) for w in words], c.paths, c.depths, c.keys, None, c.max_depth)
        for occ in sh["occ"].values():
            assert all(o[0] < len(c.nodes) and o[3] <= 64 for o in occ)
