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

  StorageSlot, bytes_to_nibbles       mp2-common/src/eth.rs:158-300, mpt_sequential/utils.rs:13-20: simple / mapping / node slots; location,
                                      mpt_key and mpt_nibbles are Keccak-256 and go through the library (csrc/storage.hip)
  storage_leaf_words                  from raw MPT leaf nodes and mapping keys to the leaves' words and values digests, on the device

A leaf's `value` is its 32-byte EVM word (MAPPING_LEAF_VALUE_LEN); a mapping key is any byte string of at most 32 bytes."""
from dataclasses import dataclass

import numpy as np

from . import (POSEIDON2, curve_sum, leaf_values_digests, leaf_values_digests_dev, map_to_curve_batch, mpt_storage_leaves_dev,
               rows_at_stride, storage_slot_keys, storage_slot_keys_dev)
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


# ---- storage slots: where a leaf lives in the trie (mp2-common/src/eth.rs:158-300) ------------------------------------------------
def bytes_to_nibbles(b):
    """mpt_sequential/utils.rs:13-20: two nibbles per byte, the high one first"""
    return [n for x in bytes(b) for n in (x >> 4, x & 15)]


class StorageSlot:
    """StorageSlot / StorageSlotNode: Simple(slot), Mapping(key, slot), Node(Mapping(parent, key)), Node(Struct(parent, evm_offset)).
    What is plain bookkeeping is plain Python; location, mpt_key and mpt_nibbles are Keccak-256 and take a Context."""
    SIMPLE, MAPPING, NODE_MAPPING, NODE_STRUCT = range(4)

    def __init__(self, kind, parent=None, key=b"", number=0):
        self.kind, self.parent, self.key, self.number = kind, parent, bytes(key), int(number)

    @classmethod
    def simple(cls, slot):
        return cls(cls.SIMPLE, number=slot)

    @classmethod
    def mapping(cls, key, slot):
        return cls(cls.MAPPING, key=key, number=slot)

    @classmethod
    def node_mapping(cls, parent, key):
        """StorageSlotNode::new_mapping (eth.rs:175-185): the parent of a mapping entry must be of mapping type"""
        if parent.kind not in (cls.MAPPING, cls.NODE_MAPPING):
            raise ValueError("The parent of a Slot mapping entry must be type of mapping")
        return cls(cls.NODE_MAPPING, parent=parent, key=key)

    @classmethod
    def node_struct(cls, parent, evm_offset):
        return cls(cls.NODE_STRUCT, parent=parent, number=evm_offset)

    def __eq__(self, other):
        return isinstance(other, StorageSlot) and (self.kind, self.parent, self.key, self.number) == (other.kind, other.parent, other.key, other.number)

    def __hash__(self):
        return hash((self.kind, self.parent, self.key, self.number))

    def slot(self):
        """`as u8`, as the reference has it (eth.rs:217-223)"""
        return self.parent.slot() if self.parent is not None else self.number & 0xFF

    def evm_offset(self):
        return self.number if self.kind == self.NODE_STRUCT else 0

    def is_simple_slot(self):
        return self.kind == self.SIMPLE if self.parent is None else self.parent.is_simple_slot()

    def mapping_keys(self):
        """the mapping keys from the outer one to the inner one"""
        own = [self.key] if self.kind in (self.MAPPING, self.NODE_MAPPING) else []
        return (self.parent.mapping_keys() if self.parent is not None else []) + own

    def _keys(self, ctx):
        """(location, mpt_key, nibbles) of this slot, one library call per level of nesting"""
        if self.kind == self.SIMPLE:
            loc, key, nib, over = storage_slot_keys(ctx, self.number, count=1)
        elif self.kind == self.MAPPING:
            loc, key, nib, over = storage_slot_keys(ctx, self.number, [left_pad32(self.key)], 1)
        elif self.kind == self.NODE_MAPPING:
            loc, key, nib, over = storage_slot_keys(ctx, 0, [left_pad32(self.key)], 1, parents=[self.parent.location(ctx)])
        else:
            loc, key, nib, over = storage_slot_keys(ctx, 0, evm_offset=self.number, parents=[self.parent.location(ctx)])
        if over:
            raise OverflowError("parent location + evm_offset leaves 256 bits")  # the reference's checked_add(..).unwrap()
        return bytes(loc[0]), bytes(key[0]), [int(n) for n in nib[0]]

    def location(self, ctx):
        return self._keys(ctx)[0]

    def mpt_key(self, ctx):
        return self._keys(ctx)[1]

    def mpt_nibbles(self, ctx):
        return self._keys(ctx)[2]


def storage_leaf_words(ctx, nodes, slot, mapping_keys, table_info, extracted_column_identifiers, key_ids, evm_word=0, variant=POSEIDON2):
    """From the raw MPT leaf nodes of one (slot, evm_word) of a table and their mapping keys to the leaves' words and values digests
    without a host computation: storage_slot_keys_dev (the MPT key of every leaf: slot, then one list of byte strings per mapping
    level in `mapping_keys`, then + evm_word for a struct's field), mpt_storage_leaves_dev (every node hashed, opened and held
    against its key), leaf_values_digests_dev over the words it left on the device. Returns (node hashes [count][32], words
    [count][32], (encodings [count][5], Weierstrass [count][11], (encoding, Weierstrass) of the sum)); a node that is not the leaf
    of its key raises ValueError with the first such leaf's index and status."""
    count, n_keys = len(nodes), len(mapping_keys)
    if len(key_ids) != n_keys or any(len(k) != count for k in mapping_keys):
        raise ValueError("one key identifier per mapping level and one key per node and level are needed")
    info, n = extracted_first(table_info, extracted_column_identifiers)
    front = info[:n]
    rows, lens = rows_at_stride(nodes)
    d_keys = ctx.to_device(_keys(*mapping_keys)) if n_keys else None
    d_nodes, d_lens = ctx.to_device(rows), ctx.to_device(lens)
    d_mpt, d_hashes, d_words, d_status = ctx.alloc(32 * count), ctx.alloc(32 * count), ctx.alloc(32 * count), ctx.alloc(4 * count)
    bufs = [b for b in (d_keys, d_nodes, d_lens, d_mpt, d_hashes, d_words, d_status) if b is not None]
    try:
        if storage_slot_keys_dev(ctx, slot, None, d_keys, n_keys, evm_word, count, None, d_mpt, None):
            raise OverflowError("location + evm_word leaves 256 bits")
        mpt_storage_leaves_dev(ctx, d_nodes, rows.shape[1], d_lens, d_mpt, count, d_hashes, d_words, None, d_status)
        status = d_status.download((count,), np.uint32)
        if status.any():
            bad = int(np.flatnonzero(status)[0])
            raise ValueError(f"node {bad} is not the leaf of its key: status {int(status[bad])}")
        digests = leaf_values_digests_dev(ctx, variant, [c.identifier for c in front], [c.layout() for c in front], len(table_info), d_words,
                                          d_keys, key_ids, evm_word, count, None, each=True, total=True)
        return d_hashes.download((count, 32), np.uint8), d_words.download((count, 32), np.uint8), digests
    finally:
        for b in bufs:
            b.free()
