"""tests/leaf_digest_cases.py on the references alone (no GPU): the byte loop of extract_value against its two-shift form over the
whole layout lattice, the case tables, and the restated leaf digests against the oracle's row digest and against each other."""
import numpy as np
import pytest

import ec_cases as EC
import leaf_digest_cases as LD
import oracle as O


def test_byte_loop_equals_shift_form_over_the_lattice():
    lattice = LD.lattice()
    assert len(lattice) == 38016 and all(LD.valid_layout(*lay) for lay in lattice)
    rng = np.random.default_rng(0x1EAF10)
    values = [bytes(32), b"\xff" * 32, bytes(range(32))] + [rng.bytes(32) for _ in range(3)]
    n = 0
    for value in values:
        for lay in lattice:
            assert LD.extract_value(value, *lay) == LD.extract_value_shifts(value, *lay), (value.hex(), lay)
            n += 1
    assert n == 228096


def test_extract_value_by_hand():
    v = bytes(range(32))
    assert LD.extract_value(v, 0, 0, 256) == v
    assert LD.extract_value(v, 31, 0, 8) == bytes(31) + b"\x1f"
    assert LD.extract_value(v, 31, 8, 8) == bytes(32)            # the byte past the word
    assert LD.extract_value(b"\xff" * 32, 31, 7, 1) == bytes(31) + b"\x01"  # (0xff & 1) << 7 = 0x80, first bit of it
    assert LD.extract_value(b"\xff" * 32, 0, 4, 4) == bytes(31) + b"\x0f"
    assert LD.extract_value(b"\xab" * 32, 5, 3, 13) == bytes(30) + bytes([0x5D, 0x0B])  # 0xab 0xab << 3 = 0x5d 0x5d.., second byte >> 3


def test_every_case_is_valid():
    assert len(set(LD.LABELS)) == len(LD.LABELS)
    points = 0
    for c in LD.CASES:
        assert all(LD.valid_layout(*lay) for lay in c["layouts"]), c["label"]
        assert len(c["layouts"]) == len(c["col_ids"]) <= 32 and c["n_table_columns"] >= len(c["col_ids"])
        assert len(c["key_ids"]) <= 2 and c["keys"].shape == (len(c["words"]), len(c["key_ids"]), 32)
        assert all(int(i) < LD.P for i in c["col_ids"]) and all(int(i) < LD.P for i in c["key_ids"])
        points += len(c["words"]) * (len(c["col_ids"]) + len(c["key_ids"]) + 1)
    assert points < 8000  # the oracle is called once per point
    assert set(LD.LAYOUTS) <= set(LD.lattice()) and set(LD.sweep_layouts()) <= set(LD.lattice())
    assert {len(c["words"]) for c in LD.CASES} >= set(LD.COUNTS)
    assert {len(c["col_ids"]) for c in LD.CASES} >= set(LD.N_EXTRACTED)
    assert {(len(c["key_ids"]), c["evm_word"]) for c in LD.CASES} >= {(k, e) for k in (0, 1, 2) for e in LD.EVM_WORDS}
    assert {c["variant"] for c in LD.CASES} == {0, 1}
    assert any(c["n_table_columns"] == len(c["col_ids"]) for c in LD.CASES) and any(c["n_table_columns"] > len(c["col_ids"]) for c in LD.CASES)
    w = LD.words(8)
    assert not w[0].any() and (w[1] == 0xFF).all() and w[2].tolist() == list(range(32))
    k = LD.keys(10, 2)
    assert not k[0].any() and k[1, 0].tolist() == [0] * 31 + [1] and (k[2] == 0xFF).all() and np.array_equal(k[3, 0], k[3, 1]) and k[3, 0].any()
    assert len(LD.NEUTRAL) == 4


@pytest.mark.parametrize("variant", [0, 1])
def test_the_hash_of_no_keys(variant):
    assert not O.hash_no_pad_batch(np.zeros((3, 0), dtype=np.uint64), 4, variant).any()
    assert not LD.row_unique_data(np.zeros((3, 0, 32), dtype=np.uint8), variant).any()


@pytest.mark.parametrize("label", LD.NEUTRAL)
def test_neutral_cases(label):
    w, wei = LD.expected(label)
    assert not w.any() and all(np.array_equal(r, EC.NEUTRAL_WEI) for r in wei)


def orc_row_digest(variant, ids, vals, unique):
    w, wei = np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    ids, vals, unique = O.arr(ids), O.arr(vals, np.uint32), O.arr(unique, np.uint32)
    n_unique = unique.shape[1] if unique.size else 0
    O.lib().orc_row_digest_batch(variant, O.p(ids), O.sz(ids.size), O.p(vals), O.p(unique), O.sz(n_unique), O.sz(vals.shape[0]), O.p(w), O.p(wei))
    return w, wei


@pytest.mark.parametrize("variant", [0, 1])
def test_a_struct_over_two_words_is_the_row_digest(variant):
    """the leaf of EVM word 0 carries the key column, the leaf of word 1 does not; both have the row id of the whole row, so their
    sum is the row's digest with the key as a column and as the unique data"""
    w0, w1, k = LD.struct_leaves()
    n_table, kid = len(LD.STRUCT_INFO), [LD.STRUCT_KEY_ID]
    leaves = [LD.leaf_values_digests(variant, *LD.struct_columns(e), n_table, (w0, w1)[e], k, kid, e)[0] for e in (0, 1)]
    ids, vals, unique = LD.struct_rows()
    for r in range(LD.STRUCT_ROWS):
        got = EC.orc_sum(np.stack([leaves[0][r], leaves[1][r]]))
        want = orc_row_digest(variant, ids, vals[r:r + 1], unique[r:r + 1])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), r
    got = EC.orc_sum(np.concatenate(leaves))
    want = orc_row_digest(variant, ids, vals, unique)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("variant", [0, 1])
def test_a_single_leaf_with_all_columns_is_the_row_digest_without_unique_columns(variant):
    ids, lays, w = LD.identifiers(40)[:len(LD.LAYOUTS)], LD.LAYOUTS, LD.words(4)
    got_w, got_wei = LD.leaf_values_digests(variant, ids, lays, len(lays), w, LD.keys(4, 0), [], 0)
    for r in range(4):
        vals = np.array([[LD.pack_be(LD.extract_value(bytes(w[r]), *lay)) for lay in lays]], dtype=np.uint32)
        want = orc_row_digest(variant, ids, vals, np.zeros((1, 0, 8), dtype=np.uint32))
        assert np.array_equal(got_w[r], want[0]) and np.array_equal(got_wei[r], want[1]), r


@pytest.mark.parametrize("variant", [0, 1])
def test_mapping_metadata_minus_single_metadata_is_the_key_column(variant):
    single = LD.metadata_digest(LD.STRUCT_INFO, 0, [], variant)
    mapping = LD.metadata_digest(LD.STRUCT_INFO, LD.STRUCT_SLOT, [(LD.KEY_ID_PREFIX, LD.STRUCT_KEY_ID)], variant)
    diff = EC.orc_sum(np.stack([mapping[0], EC.negate(single[0])]))[0]
    assert np.array_equal(diff, LD.key_metadata_point(LD.KEY_ID_PREFIX, LD.STRUCT_SLOT, LD.STRUCT_KEY_ID, variant))
    assert int.from_bytes(LD.KEY_ID_PREFIX, "big") == 0x4B4559 and int.from_bytes(LD.OUTER_KEY_ID_PREFIX, "big") < 1 << 56
    both = LD.metadata_digest(LD.STRUCT_INFO, LD.STRUCT_SLOT, [(LD.OUTER_KEY_ID_PREFIX, 77), (LD.INNER_KEY_ID_PREFIX, 78)], variant)
    parts = [single[0], LD.key_metadata_point(LD.OUTER_KEY_ID_PREFIX, LD.STRUCT_SLOT, 77, variant),
             LD.key_metadata_point(LD.INNER_KEY_ID_PREFIX, LD.STRUCT_SLOT, 78, variant)]
    assert np.array_equal(EC.orc_sum(np.stack(parts))[0], both[0])
