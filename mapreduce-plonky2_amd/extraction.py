"""Tables that live in contract storage: the values digest of every MPT storage leaf and the metadata digest of its table
(mp2-v1/src/values_extraction/mod.rs:298-496), mirrored over the C ABI. The names and orderings are the reference's:

  ColumnInfo                          gadgets/column_info.rs:17-35 (slot, identifier, byte_offset, bit_offset, length, evm_word)
  left_pad32                          mp2-common/src/eth.rs:93-95
  filter_table_column_identifiers     gadgets/column_gadget.rs:372-389
  extracted_first                     the stable sort of ColumnGadgetData::new / ColumnsMetadata::new (column_gadget.rs:273-298,
                                      metadata_gadget.rs:50-77): the extracted columns first, each part in table order
  leaf_*_values_digests               mod.rs:327-341, :374-406, :450-496, batched over the leaves of one (slot, evm_word): one launch
                                      (csrc/extraction.hip), the cut of the columns out of the EVM words included
  leaf_*_metadata_digest              mod.rs:316-325, :343-372, :408-445: per table, not per leaf, so they are composed from
                                      hash_no_pad_batch, map_to_curve_batch and curve_sum and have no kernel of their own

A leaf's `value` is its 32-byte EVM word (MAPPING_LEAF_VALUE_LEN); a mapping key is any byte string of at most 32 bytes."""
from dataclasses import dataclass

import numpy as np

from . import POSEIDON2, curve_sum, leaf_values_digests, map_to_curve_batch
from .identifiers import INNER_KEY_ID_PREFIX, KEY_ID_PREFIX, OUTER_KEY_ID_PREFIX

MAX_FIELD_PER_EVM = 32  # the columns one launch takes (MP2G_LEAF_MAX_COLS); the reference's const generic of the same name


@dataclass(frozen=True)
class ColumnInfo:
    slot: int
    identifier: int
    byte_offset: int
    bit_offset: int
    length: int
    evm_word: int

    def layout(self):
        return (self.byte_offset, self.bit_offset, self.length)


def left_pad32(b):
    b = bytes(b)
    if len(b) > 32:
        raise ValueError("more than 32 bytes")
    return b"\0" * (32 - len(b)) + b


def filter_table_column_identifiers(table_info, slot, evm_word):
    """the identifiers of the columns of (slot, evm_word), in table order"""
    return [c.identifier for c in table_info if c.slot == slot and c.evm_word == evm_word]


def extracted_first(table_info, extracted_column_identifiers):
    """(table_info with the extracted columns moved to the front, their number): sort_by_key(!contains) is stable"""
    ids = set(int(i) for i in extracted_column_identifiers)
    front = [c for c in table_info if c.identifier in ids]
    return front + [c for c in table_info if c.identifier not in ids], len(extracted_column_identifiers)


def _values_digests(ctx, table_info, extracted_column_identifiers, values, keys, key_ids, evm_word, variant):
    """ColumnGadgetData::digest reads the first num_extracted_columns = len(extracted_column_identifiers) entries of the sorted
    table_info, whatever they are"""
    info, n = extracted_first(table_info, extracted_column_identifiers)
    if n > len(info):
        raise ValueError("more extracted identifiers than columns")
    front = info[:n]
    return leaf_values_digests(ctx, [c.identifier for c in front], [c.layout() for c in front], len(table_info), values, keys, key_ids,
                               evm_word, variant)


def _keys(*key_lists):
    """[count][n_keys][32] from one list of byte strings per key column"""
    rows = list(zip(*key_lists))
    return np.frombuffer(b"".join(left_pad32(k) for row in rows for k in row), dtype=np.uint8).reshape(len(rows), len(key_lists), 32)


def leaf_single_values_digests(ctx, table_info, extracted_column_identifiers, values, variant=POSEIDON2):
    """compute_leaf_single_values_digest of every value [count][32]: (encodings [count][5], Weierstrass [count][11], (encoding,
    Weierstrass) of their sum)"""
    return _values_digests(ctx, table_info, extracted_column_identifiers, values, None, (), 0, variant)


def leaf_mapping_values_digests(ctx, table_info, extracted_column_identifiers, values, mapping_keys, evm_word, key_id, variant=POSEIDON2):
    """compute_leaf_mapping_values_digest of every (value, mapping key)"""
    return _values_digests(ctx, table_info, extracted_column_identifiers, values, _keys(mapping_keys), (key_id,), evm_word, variant)


def leaf_mapping_of_mappings_values_digests(ctx, table_info, extracted_column_identifiers, values, evm_word, outer_keys, outer_key_id,
                                            inner_keys, inner_key_id, variant=POSEIDON2):
    """compute_leaf_mapping_of_mappings_values_digest of every (value, outer key, inner key)"""
    return _values_digests(ctx, table_info, extracted_column_identifiers, values, _keys(outer_keys, inner_keys),
                           (outer_key_id, inner_key_id), evm_word, variant)


# ---- metadata: one digest per table ---------------------------------------------------------------------------------------------
def _metadata_digest(ctx, table_info, slot, keys, variant):
    """sum over the table's columns of D(H(slot, evm_word, byte_offset, bit_offset, length) || identifier) (column_info.rs:95-118,
    metadata_gadget.rs:126-130) plus D(H(prefix, slot) || key_id) per key column; (encoding, Weierstrass)"""
    points = []
    if table_info:
        md = ctx.hash_no_pad_batch([[c.slot, c.evm_word, c.byte_offset, c.bit_offset, c.length] for c in table_info], 4, variant)
        ids = np.array([[c.identifier] for c in table_info], dtype=np.uint64)
        points.append(map_to_curve_batch(ctx, np.concatenate([md, ids], axis=1), variant))
    if keys:
        md = ctx.hash_no_pad_batch([[int.from_bytes(prefix, "big"), slot] for prefix, _ in keys], 4, variant)
        ids = np.array([[key_id] for _, key_id in keys], dtype=np.uint64)
        points.append(map_to_curve_batch(ctx, np.concatenate([md, ids], axis=1), variant))
    pts = np.concatenate(points) if points else np.zeros((0, 5), dtype=np.uint64)
    return curve_sum(ctx, pts, weierstrass=True)


def leaf_single_metadata_digest(ctx, table_info, variant=POSEIDON2):
    return _metadata_digest(ctx, table_info, 0, [], variant)


def leaf_mapping_metadata_digest(ctx, table_info, slot, key_id, variant=POSEIDON2):
    return _metadata_digest(ctx, table_info, slot, [(KEY_ID_PREFIX, key_id)], variant)


def leaf_mapping_of_mappings_metadata_digest(ctx, table_info, slot, outer_key_id, inner_key_id, variant=POSEIDON2):
    return _metadata_digest(ctx, table_info, slot, [(OUTER_KEY_ID_PREFIX, outer_key_id), (INNER_KEY_ID_PREFIX, inner_key_id)], variant)
