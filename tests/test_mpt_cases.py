"""The checker's own restatement of the MPT inclusion-proof rules (tests/mpt_cases.py: open_node, walk, the trie builder) held to
the recorded proofs with the figures known of them, to every proof of every built trie, to the status and level every damage is
made for, and to the leaf decode of tests/keccak_cases.py. No GPU and no library: nothing here calls the code under test."""
import keccak_cases as K
import mpt_cases as M


def test_recorded_storage_proof():
    answer, _ = M.recorded()
    mode, row = M.recorded_rows()["storage"]
    b = M.Batch("storage", mode, [row])
    _, info, out = b.want()
    assert [len(n) for n in b.nodes] == [532, 532, 532, 436, 37]
    assert [M.kind(i) for i in info] == [M.BRANCH] * 4 + [M.LEAF]
    assert [int(i) >> 8 & 0xFFFF for i in info[:4]] == [0xFFFF, 0xFFFF, 0xFFFF, 0x7F9F] and int(info[4]) >> 8 & 0x7F == 60
    assert [b.nodes[k][:3].hex() for k in range(3)] == ["f90211"] * 3
    assert b.keys[0] == K.keccak256(bytes(31) + b"\x08") and b.roots[0] == M.unhex(answer["storageHash"])
    assert out["status"].tolist() == [M.OK] and bytes(out["words"][0]) == K.left_pad32(b"\x22\xb8")
    assert out["consumed"][0].tolist() == [0, 1, 2, 3, 4]
    assert M.unhex(answer["storageProof"][0]["value"]) == b"\x22\xb8"


def test_recorded_account_proof():
    answer, _ = M.recorded()
    mode, row = M.recorded_rows()["account"]
    b = M.Batch("account", mode, [row])
    _, info, out = b.want()
    assert len(b.nodes) == 9 and [len(n) for n in b.nodes[6:]] == [372, 83, 104]
    assert [M.kind(i) for i in info] == [M.BRANCH] * 8 + [M.LEAF] and int(info[8]) >> 8 & 0x7F == 56
    leaf = b.nodes[8]
    value = bytes.fromhex("f8440180a0") + M.unhex(answer["storageHash"]) + b"\xa0" + M.unhex(answer["codeHash"])
    assert leaf.endswith(value) and (int(out["val_off"][0]), int(out["val_len"][0])) == (len(leaf) - len(value), len(value))
    assert out["status"].tolist() == [M.OK] and bytes(out["words"][0]) == M.unhex(answer["storageHash"])
    assert out["consumed"][0].tolist() == list(range(9))


def test_recorded_three_nodes():
    rows = M.recorded_rows()
    raw, word = M.Batch("raw", *[rows["three raw"][0], [rows["three raw"][1]]]), M.Batch("word", *[rows["three word"][0], [rows["three word"][1]]])
    _, info, out = raw.want()
    assert [M.kind(i) for i in info] == [M.EXTENSION, M.BRANCH, M.LEAF] and [int(info[0]) >> 8 & 0x7F, int(info[2]) >> 8 & 0x7F] == [1, 62]
    assert out["status"].tolist() == [M.OK] and out["consumed"][0].tolist() == [0, 1, 2] and not out["words"].any()
    assert (int(out["val_off"][0]), int(out["val_len"][0])) == (len(raw.nodes[2]) - 32, 32)
    out = word.want()[2]
    assert (out["status"].tolist(), out["fail_level"].tolist()) == ([M.BAD_VALUE], [2]) and (out["val_off"][0], out["val_len"][0]) == (0, 0)


def test_every_batch_gives_what_it_intends():
    for b in M.batches():
        out = b.want()[2]
        got = list(zip(out["status"].tolist(), out["fail_level"].tolist()))
        assert got == b.intended, (b.name, [(l, g, w) for l, g, w in zip(b.labels, got, b.intended) if g != w])
        for i, (status, level) in enumerate(got):
            reached = b.depths[i] if status == M.OK else (level + 1 if 1 <= b.depths[i] <= b.max_depth else 0)
            row = out["consumed"][i].tolist()
            assert all(c <= 64 for c in row[:reached]) and row[:reached] == sorted(row[:reached]) and set(row[reached:]) <= {0xFF}, (b.name, i)
            if status != M.OK:
                assert not out["words"][i].any() and out["val_off"][i] == 0 and out["val_len"][i] == 0
    assert {s for b in M.batches() for s, _ in b.intended} == set(range(11))  # every path status occurs


def test_built_tries_have_the_shapes_they_are_made_for():
    for name, trie, shape in M.extension_tries():
        proof = trie.proofs[trie.keys[0]]
        infos = [M.open_node(n) for n in proof]
        assert [(M.kind(i), None if M.kind(i) == M.BRANCH else i >> 8 & 0x7F) for i in infos] == shape, name
        assert all(len(n) >= 32 for n in proof)
    t = M.random_trie()
    assert len(t.keys) == 129 and M.open_node(t.root_node) == M.BRANCH | 3 << 5 | 0xFFFF << 8 and len(t.root_node) == 532
    assert len({len(p) for p in t.proofs.values()}) >= 2  # lanes of one wave at different depths
    c = M.chain_trie()
    depths = sorted(len(p) for p in c.proofs.values())
    assert len(c.keys) == 65 and depths[-2:] == [65, 65] and depths[0] == 2
    b = next(b for b in M.batches() if b.name == "a 65-node path")
    assert b.max_depth == M.MAX_DEPTH and 64 in b.want()[2]["consumed"].max(axis=1, initial=0, where=b.want()[2]["consumed"] != 0xFF).tolist()
    e = M.embedded_trie()
    infos = [M.open_node(n) for n in e.proofs[e.keys[0]]]
    assert M.invalid(M.EMBEDDED_CHILD) in infos and {len(p) for p in e.proofs.values()} == {2, 3}


def test_node_table():
    table = M.node_table()
    for label, node, info in table:
        assert M.open_node(node) == info, label
    assert {M.reason(info) for _, _, info in table if M.kind(info) == M.INVALID} == {1, 2, 3, 4, 5}  # every node reason occurs
    assert {M.kind(info) for _, _, info in table} == {0, 1, 2, 3}
    # the mask trick: the child at nibble k lies where the info word says
    _, node, info = table[0]
    for k in (1, 4, 15):
        off = M.branch_child_offset(info, k)
        assert node[off - 1] == 0xA0 and node[off:off + 32] == M.child(k)[1:]


def test_hostile_rows():
    rows, lens = M.hostile_rows()
    infos = [M.open_node(r[:min(n, M.HOSTILE_STRIDE)]) for r, n in zip(rows, lens)]
    assert infos[:-1] == [M.invalid(M.MALFORMED)] * (len(rows) - 1) and M.kind(infos[-1]) == M.LEAF


def test_leaf_rules_agree_with_the_leaf_opener():
    """a node is a leaf under the rules of mp2g_mpt_open_nodes exactly when mp2g_mpt_storage_leaves accepts its structure and its
    prefix; its value in WORD mode and its path against a key are then judged alike"""
    for label, node, key, *_ in list(K.good_leaves()) + list(K.damaged_leaves()):
        status, word, n_nibbles = K.decode_leaf(node, key)
        info = M.open_node(node)
        assert (M.kind(info) == M.LEAF) == (status in (K.OK, K.BAD_VALUE, K.KEY_MISMATCH)), label
        if M.kind(info) != M.LEAF:
            continue
        # as the last node of a path whose earlier levels consumed what the leaf's path leaves of the key
        nib = info >> 8 & 0x7F
        _, v_off, v_len, _ = M._item(node, info >> 16, len(node))
        sound, got = M.leaf_value(node[v_off:v_off + v_len], M.WORD)
        matches = M.path_nibbles(node, info) == K.bytes_to_nibbles(key)[64 - nib:]
        mine = K.BAD_VALUE if not sound else (K.OK if matches else K.KEY_MISMATCH)
        assert mine == status, label
        if status == K.OK:
            assert (got, nib) == (word, n_nibbles), label


def test_the_empty_trie():
    assert M.Trie({}).root == K.keccak256(b"\x80") and M.Trie({}).proofs == {}
    assert M.Trie({}).root.hex() == "56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421"
