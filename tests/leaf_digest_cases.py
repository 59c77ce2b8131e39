"""Case tables for the storage-leaf kernels (csrc/extraction.hip) and the checker's restatement of what the reference computes for
a table in contract storage (mp2-v1/src/values_extraction/mod.rs:298-496). No GPU is used here and nothing here calls the code
under test: tests/test_leaf_digest_cases.py checks the tables and the restatement on the references alone,
tests/test_gpu_leaf_digests.py feeds the same arrays to the device.

extract_value() is the byte loop as gadgets/column_gadget.rs:326-368 writes it; extract_value_shifts() is the two-shift form the
kernels use, on one Python integer. The digests come from the oracle's primitives, one call per point: orc_map_to_curve_batch,
orc_curve_sum, orc_scalar_mul, hash_no_pad_batch.

The builders are seeded and cached: every caller gets the same arrays and must leave them unchanged."""
import functools

import numpy as np

import ec_cases as EC
import oracle as O

P = O.P
KEY_ID_PREFIX, OUTER_KEY_ID_PREFIX, INNER_KEY_ID_PREFIX = b"\0KEY", b"\0OUT_KEY", b"\0\0IN_KEY"

# (byte offset, bit offset, length in bits). In the last two the byte after the field lies past the word and reads as zero.
LAYOUTS = [(0, 0, 256), (0, 0, 1), (0, 1, 255), (0, 4, 4), (5, 3, 13), (12, 0, 160), (16, 0, 128), (30, 0, 9), (31, 0, 8), (31, 7, 1),
           (31, 8, 8)]
COUNTS = [1, 127, 128, 129, 257]  # the 128-lane block's edge and a grid tail
EVM_WORDS = [0, 1, (1 << 32) - 1]
N_EXTRACTED = [0, 1, 16, 32]
SWEEP_LENGTHS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 128, 255, 256]  # the cut alone, at every (byte, bit) these lengths fit


# ---- the reference's byte loop and its shift form ---------------------------------------------------------------------------------
def first_bits(byte, n):
    return byte >> (8 - n)


def last_bits(byte, n):
    return byte & ((1 << n) - 1)


def left_pad32(b):
    assert len(b) <= 32
    return bytes(32 - len(b)) + bytes(b)


def valid_layout(byte_offset, bit_offset, length):
    """what extract_value's assertions and array bounds allow"""
    return 1 <= length <= 256 and 0 <= bit_offset <= 8 and byte_offset >= 0 and byte_offset + (length + 7) // 8 <= 32


def extract_value(value, byte_offset, bit_offset, length):
    """column_gadget.rs:326-368, line by line"""
    assert len(value) == 32 and bit_offset <= 8
    last_byte_offset = byte_offset + (length + 7) // 8 - 1
    result = []
    for i in range(byte_offset, last_byte_offset + 1):
        current_byte = value[i]
        next_byte = value[i + 1] if i < 31 else 0
        actual_byte = (last_bits(current_byte, 8 - bit_offset) << bit_offset) + first_bits(next_byte, bit_offset)
        assert actual_byte < 256
        result.append(actual_byte)
    length_mod_8 = length % 8
    if length_mod_8 > 0:
        result[-1] = first_bits(result[-1], length_mod_8)
    return left_pad32(bytes(result))


def extract_value_shifts(value, byte_offset, bit_offset, length):
    """((V << (8 byte + bit)) mod 2^256) >> (256 - 8 k), then the low byte >> (8 - length % 8) when length % 8 != 0"""
    k, m = (length + 7) // 8, length % 8
    w = ((int.from_bytes(value, "big") << (8 * byte_offset + bit_offset)) & ((1 << 256) - 1)) >> (256 - 8 * k)
    if m:
        w = (w & ~0xFF) | ((w & 0xFF) >> (8 - m))
    return w.to_bytes(32, "big")


def pack_be(b32):
    """pack(Endianness::Big): 8 u32 words, most significant first"""
    return [int.from_bytes(b32[4 * j:4 * j + 4], "big") for j in range(8)]


def lattice():
    """every valid (byte offset, bit offset, length)"""
    return [(b, bit, ln) for ln in range(1, 257) for b in range(0, 33 - (ln + 7) // 8) for bit in range(9)]


def sweep_layouts():
    return [lay for lay in lattice() if lay[2] in SWEEP_LENGTHS]


# ---- words and keys ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def words(count, seed=0x1EAF01):
    """uint8 [count][32]: all 0x00, all 0xff, the bytes 0..31, then seeded random words, repeating in that order of four"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    w[0::4], w[1::4], w[2::4] = 0, 0xFF, np.arange(32, dtype=np.uint8)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def keys(count, n_keys, seed=0x1EAF02):
    """uint8 [count][n_keys][32], left-padded: rows repeat the zero key, 31 zero bytes then 1, all 0xff, a short random key whose
    outer and inner copies are equal, and independent random keys"""
    rng = np.random.default_rng(seed + n_keys)
    k = rng.integers(0, 256, size=(count, n_keys, 32), dtype=np.uint8)
    if n_keys:
        k[0::5] = 0
        k[1::5] = 0
        k[1::5, :, 31] = 1
        k[2::5] = 0xFF
        k[3::5, :, :12] = 0
        k[3::5] = k[3::5, :1]
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def identifiers(n, seed=0x1EAF03):
    ids = O.rand_field((n,), seed)
    ids[0] = P - 1  # the largest canonical identifier
    ids.setflags(write=False)
    return ids


def layouts_of(n):
    """n layouts: the lattice of LAYOUTS first, then seeded valid ones"""
    out = list(LAYOUTS[:n])
    rng = np.random.default_rng(0x1EAF04)
    while len(out) < n:
        ln = int(rng.integers(1, 257))
        out.append((int(rng.integers(0, 33 - (ln + 7) // 8)), int(rng.integers(0, 9)), ln))
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def row_unique_data(key_rows, variant):
    """H(pack(key_0) || pack(key_1)) per leaf (mod.rs:298-314, :499-510); key_rows uint8 [count][n_keys][32]"""
    count, n_keys = key_rows.shape[:2]
    limbs = np.array([[x for k in row for x in pack_be(bytes(k))] for row in key_rows], dtype=np.uint64).reshape(count, 8 * n_keys)
    return O.hash_no_pad_batch(limbs, 4, variant)


def row_ids(key_rows, num_actual_columns, variant):
    """compute_row_id (mod.rs:512-523) per leaf, as Python integers"""
    u = row_unique_data(key_rows, variant)
    h = O.hash_no_pad_batch(np.concatenate([u, np.full((len(u), 1), num_actual_columns, dtype=np.uint64)], axis=1), 4, variant)
    return [int(r[0]) + (int(r[1]) << 64) for r in h]


def leaf_values_digests(variant, col_ids, layouts, n_table_columns, word_rows, key_rows, key_ids, evm_word):
    """(encodings [count][5], Weierstrass [count][11]) of compute_leaf_{single,mapping,mapping_of_mappings}_values_digest
    (mod.rs:327-341, :374-406, :450-496) of every leaf; the kind is the number of keys"""
    count, n_keys = len(word_rows), len(key_ids)
    assert key_rows.shape == (count, n_keys, 32) and len(col_ids) == len(layouts)
    per_leaf = len(col_ids) + (n_keys if evm_word == 0 else 0)
    ins = []
    for i in range(count):
        value = bytes(word_rows[i])
        ins += [[int(cid)] + pack_be(extract_value(value, *lay)) for cid, lay in zip(col_ids, layouts)]
        if evm_word == 0:
            ins += [[int(kid)] + pack_be(bytes(key_rows[i, j])) for j, kid in enumerate(key_ids)]
    pts = EC.orc_map(np.array(ins, dtype=np.uint64), variant)[0] if ins else np.zeros((0, 5), dtype=np.uint64)
    ks = row_ids(key_rows, n_table_columns + n_keys, variant)
    w, wei = np.zeros((count, 5), dtype=np.uint64), np.zeros((count, 11), dtype=np.uint64)
    for i in range(count):
        s = EC.orc_sum(pts[i * per_leaf:(i + 1) * per_leaf])[0]
        w[i], wei[i] = EC.orc_mul(s, ks[i])
    return w, wei


def column_metadata_points(table_info, variant):
    """ColumnInfo::digest of every column (column_info.rs:95-118); table_info rows (slot, identifier, byte, bit, length, evm_word)"""
    if not table_info:
        return np.zeros((0, 5), dtype=np.uint64)
    md = O.hash_no_pad_batch(np.array([[s, w, b, bit, ln] for s, _, b, bit, ln, w in table_info], dtype=np.uint64), 4, variant)
    return EC.orc_map(np.concatenate([md, np.array([[i] for _, i, *_ in table_info], dtype=np.uint64)], axis=1), variant)[0]


def key_metadata_point(prefix, slot, key_id, variant):
    """D(H(prefix, slot) || key_id), prefix read as a big-endian integer (mod.rs:356-369, :427-440)"""
    md = O.hash_no_pad_batch(np.array([[int.from_bytes(prefix, "big"), slot]], dtype=np.uint64), 4, variant)
    return EC.orc_map(np.concatenate([md, np.array([[key_id]], dtype=np.uint64)], axis=1), variant)[0][0]


def metadata_digest(table_info, slot, key_columns, variant):
    """compute_leaf_{single,mapping,mapping_of_mappings}_metadata_digest (mod.rs:316-325, :343-372, :408-445); key_columns
    [(prefix, key_id)]"""
    pts = [column_metadata_points(table_info, variant)] + [key_metadata_point(p, slot, k, variant)[None] for p, k in key_columns]
    return EC.orc_sum(np.concatenate(pts))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _case(label, variant, n_extracted, n_table_columns, count, n_keys, evm_word):
    return {"label": label, "variant": variant, "col_ids": identifiers(40)[:n_extracted], "layouts": layouts_of(n_extracted),
            "n_table_columns": n_table_columns, "words": words(count), "keys": keys(count, n_keys),
            "key_ids": identifiers(40)[38:38 + n_keys][::-1], "evm_word": evm_word}


def _cases():
    out = []
    # the block edge and the grid tail: one odd field and one mapping key
    for variant, counts in ((0, COUNTS), (1, [1, 129])):
        for count in counts:
            c = _case(f"v{variant} count {count}", variant, 1, 3, count, 1, 0)
            c["layouts"] = [(5, 3, 13)]
            out.append(c)
    # every layout of the lattice as one leaf's columns, every kind of leaf, every evm_word; n_table_columns equal to and above
    for variant in (0, 1):
        for n_keys in (0, 1, 2):
            for evm_word in EVM_WORDS:
                n_table = len(LAYOUTS) if evm_word == 0 else 40
                out.append(_case(f"v{variant} lattice, {n_keys} keys, evm_word {evm_word}", variant, len(LAYOUTS), n_table, 8, n_keys, evm_word))
    # the number of extracted columns; without columns the digest is neutral unless key columns join it
    for variant in (0, 1):
        for n in N_EXTRACTED:
            out.append(_case(f"v{variant} {n} extracted, mapping, evm_word 0", variant, n, max(n, 1), 5, 1, 0))
        out.append(_case(f"v{variant} 0 extracted, no keys", variant, 0, 0, 5, 0, 0))
        out.append(_case(f"v{variant} 0 extracted, 2 keys, evm_word 1", variant, 0, 7, 5, 2, 1))
        out.append(_case(f"v{variant} 32 extracted, single", variant, 32, 33, 3, 0, 0))
    return out


CASES = _cases()
LABELS = [c["label"] for c in CASES]
NEUTRAL = [c["label"] for c in CASES if not len(c["col_ids"]) and (c["evm_word"] != 0 or not len(c["key_ids"]))]


@functools.lru_cache(maxsize=None)
def expected(label):
    c = CASES[LABELS.index(label)]
    out = leaf_values_digests(c["variant"], c["col_ids"], c["layouts"], c["n_table_columns"], c["words"], c["keys"], c["key_ids"], c["evm_word"])
    for a in out:
        a.setflags(write=False)
    return out


# ---- a struct spread over two EVM words under one mapping key ---------------------------------------------------------------------
STRUCT_SLOT, STRUCT_KEY_ID = 9, 0x4B4559
# (slot, identifier, byte offset, bit offset, length, evm_word): two fields in word 0, three in word 1
STRUCT_INFO = [(STRUCT_SLOT, 1001, 12, 0, 160, 0), (STRUCT_SLOT, 1002, 0, 0, 96, 0), (STRUCT_SLOT, 1003, 31, 0, 8, 1),
               (STRUCT_SLOT, 1004, 0, 4, 4, 1), (STRUCT_SLOT, 1005, 5, 3, 13, 1)]
STRUCT_ROWS = 6


def struct_columns(evm_word):
    cols = [c for c in STRUCT_INFO if c[5] == evm_word]
    return np.array([c[1] for c in cols], dtype=np.uint64), [c[2:5] for c in cols]


def struct_leaves():
    """(words of EVM word 0, words of EVM word 1 [rows][32], keys [rows][1][32])"""
    return words(STRUCT_ROWS, 0x1EAF05), words(STRUCT_ROWS, 0x1EAF06), keys(STRUCT_ROWS, 1, 0x1EAF07)


def struct_rows():
    """the reassembled table: (col_ids [6], values uint32 [rows][6][8], unique uint32 [rows][1][8]): the five fields, then the key
    column; the key is the row's unique data"""
    w0, w1, k = struct_leaves()
    vals = np.zeros((STRUCT_ROWS, 6, 8), dtype=np.uint32)
    for r in range(STRUCT_ROWS):
        for c, info in enumerate(STRUCT_INFO):
            vals[r, c] = pack_be(extract_value(bytes((w0, w1)[info[5]][r]), *info[2:5]))
        vals[r, 5] = pack_be(bytes(k[r, 0]))
    ids = np.array([c[1] for c in STRUCT_INFO] + [STRUCT_KEY_ID], dtype=np.uint64)
    return ids, vals, np.ascontiguousarray(vals[:, 5:6])
