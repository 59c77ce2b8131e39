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
  MptProofSet, verify_mpt_proofs      eth.rs:345-399 verify_storage_proof / verify_state_proof, mpt_sequential/utils.rs:69-121: whole
                                      eth_getProof paths, every distinct node hashed and opened once, every path walked to its root
                                      (csrc/mpt.hip)
  account_storage_roots               state root -> account leaf -> storage root, left on the device
  storage_proof_words                 storage_leaf_words through whole proofs under a storage root
  mpt_subtree_digests                 values_extraction/branch.rs:77-112, extension.rs:53-61: DV and N of every node of the trie the
                                      proofs show, summed up the trie on the device (csrc/mpt_digest.hip)
  values_extraction_public_inputs     values_extraction/public_inputs.rs:23-36: H, K, T, DV, DM, N of every node
  storage_proof_tree                  storage_proof_words carried on to every node's public inputs

A leaf's `value` is its 32-byte EVM word (MAPPING_LEAF_VALUE_LEN); a mapping key is any byte string of at most 32 bytes."""
from dataclasses import dataclass

import numpy as np

from . import (MPT_MAX_DEPTH, MPT_NODE_BRANCH, MPT_NO_NODE, MPT_PATH_OUTPUTS, MPT_SUBTREE_OUTPUTS, MPT_VALUE_ACCOUNT, MPT_VALUE_RAW, MPT_VALUE_WORD, POSEIDON2,
               DeviceBuffer, curve_emit_dev, curve_sum, keccak256_batch_dev, leaf_values_digests, leaf_values_digests_dev, map_to_curve_batch,
               mpt_open_nodes_dev, mpt_storage_leaves_dev, mpt_subtree_digests_dev, mpt_verify_paths_dev, rows_at_stride, storage_slot_keys,
               storage_slot_keys_dev)
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


# ---- whole proofs: from the leaf up to the storage root, from the account up to the state root ------------------------------------
class MptProofSet:
    """The proofs of one trie (the `proof` lists of eth_getProof answers) as the library takes them: `nodes`, every distinct node
    once, and paths [count][max_depth] of indices into it with depths [count], the root first."""

    def __init__(self, nodes, paths, depths):
        self.nodes, self.paths, self.depths = nodes, paths, depths

    @classmethod
    def from_proofs(cls, proofs, leaf_first=False, by_position=False, mpt_keys=None, node_info=None):
        """proofs: one list of node byte strings per proof, root first as eth_getProof orders them; leaf_first=True takes the
        order the reference's circuits use (the leaf first, the root last). Nodes are deduplicated by their bytes. With
        by_position=True a node is identified by (its parent's index, its slot below that parent, its bytes): the table is then a
        tree by construction, which mpt_subtree_digests needs. The slot is include/mp2g.h's: the key's nibble at the parent's
        `entered` below a branch, 0 below an extension and at the root. It needs mpt_keys (one 32-byte key per proof) and node_info
        ({node bytes: its info word}, as mpt_open_nodes gives them for the table by bytes: no node is parsed here). Without them
        the slot is 0 everywhere: two leaves with equal tails and values below two nibbles of one branch share their parent and
        their bytes, the table then holds them once, and the subtree call reports the conflict."""
        depths = np.array([len(p) for p in proofs], dtype=np.uint32)
        max_depth = max(1, int(depths.max(initial=1)))
        if max_depth > MPT_MAX_DEPTH:
            raise ValueError(f"a proof of {max_depth} nodes is deeper than a 64-nibble key allows ({MPT_MAX_DEPTH})")
        if (mpt_keys is None) != (node_info is None):
            raise ValueError("the slots need both the MPT keys and the nodes' info words")
        if mpt_keys is not None and len(mpt_keys) != len(proofs):
            raise ValueError("one MPT key per proof is needed")
        index, nodes = {}, []
        paths = np.zeros((len(proofs), max_depth), dtype=np.uint32)
        for i, proof in enumerate(proofs):
            nib = bytes_to_nibbles(bytes(mpt_keys[i])) if by_position and mpt_keys is not None else None
            parent, ptr, slot = None, 0, 0
            for level, node in enumerate(reversed(proof) if leaf_first else proof):
                node = bytes(node)
                name = (parent, slot, node) if by_position else node
                if name not in index:
                    index[name] = len(nodes)
                    nodes.append(node)
                paths[i, level] = parent = index[name]
                if nib is not None:
                    word = int(node_info[node])
                    branch = word & 3 == MPT_NODE_BRANCH
                    slot = nib[ptr] if branch and ptr < 64 else 0
                    ptr += 1 if branch else word >> 8 & 0x7F
        return cls(nodes, paths, depths)

    def __len__(self):
        return len(self.depths)


def _device_bytes32(ctx, a, count, bufs):
    """a DeviceBuffer as it is; otherwise `a` ([count][32], or one 32-byte string for all) uploaded and noted in bufs for freeing.
    Returns (buffer, row stride)"""
    if isinstance(a, DeviceBuffer):
        return a, 32
    rows = np.frombuffer(bytes(a), dtype=np.uint8).reshape(1, 32) if isinstance(a, (bytes, bytearray)) else \
        np.ascontiguousarray(np.asarray([np.frombuffer(bytes(r), dtype=np.uint8) for r in a]), dtype=np.uint8).reshape(-1, 32)
    if rows.shape[0] not in (1, count):
        raise ValueError("one 32-byte row, or one per proof, is needed")
    bufs.append(ctx.to_device(rows))
    return bufs[-1], 32 if rows.shape[0] == count else 0


def verify_mpt_proofs(ctx, proof_set, mpt_keys, roots, value=MPT_VALUE_WORD, d_words=None, root_stride=32):
    """Every proof of proof_set walked from its root to its leaf under mpt_keys [count][32]: mpt_open_nodes_dev over the distinct
    nodes, then mpt_verify_paths_dev. roots: None (not checked), one 32-byte string, [count][32], or a DeviceBuffer of [count][32]
    (the words an ACCOUNT walk left; with root_stride=0 its first 32 bytes are the one root of all); mpt_keys may be a DeviceBuffer
    too. value: MPT_VALUE_WORD / _ACCOUNT / _RAW. With d_words (a DeviceBuffer of 32 * count bytes) the words also stay on the
    device. Returns the outputs by name (MPT_PATH_OUTPUTS) as arrays; nothing is raised for a failing proof: see its status and
    fail_level."""
    count, max_depth = len(proof_set), proof_set.paths.shape[1]
    shapes = {"status": ((count,), np.uint32), "fail_level": ((count,), np.uint32), "words": ((count, 32), np.uint8),
              "val_off": ((count,), np.uint32), "val_len": ((count,), np.uint32), "consumed": ((count, max_depth), np.uint8)}
    if not count:
        return {name: np.zeros(s, dtype=t) for name, (s, t) in shapes.items()}
    rows, lens = rows_at_stride(proof_set.nodes)
    n_nodes = len(lens)
    bufs = []
    try:
        for a in (rows, lens, proof_set.paths, proof_set.depths):
            bufs.append(ctx.to_device(a))
        d_nodes, d_lens, d_paths, d_depths = bufs
        d_keys, _ = _device_bytes32(ctx, mpt_keys, count, bufs)
        if isinstance(roots, DeviceBuffer):
            d_roots = roots
        else:
            d_roots, root_stride = (None, 0) if roots is None else _device_bytes32(ctx, roots, count, bufs)
        bufs += [ctx.alloc(32 * max(n_nodes, 1)), ctx.alloc(4 * max(n_nodes, 1))]
        d_hashes, d_info = bufs[-2:]
        outs = {name: (d_words if name == "words" and d_words is not None else ctx.alloc(int(np.prod(s)) * np.dtype(t).itemsize))
                for name, (s, t) in shapes.items()}
        bufs += [b for b in outs.values() if b is not d_words]
        if value == MPT_VALUE_RAW:
            outs["words"].upload(np.zeros((count, 32), dtype=np.uint8))
        mpt_open_nodes_dev(ctx, d_nodes, rows.shape[1], d_lens, n_nodes, d_hashes, d_info)
        mpt_verify_paths_dev(ctx, d_nodes, rows.shape[1], d_lens, d_hashes, d_info, n_nodes, d_paths, d_depths, max_depth, d_keys, count,
                             d_roots, root_stride, value, *(outs[name] for name in MPT_PATH_OUTPUTS))
        return {name: outs[name].download(*shapes[name]) for name in MPT_PATH_OUTPUTS}
    finally:
        for b in bufs:
            b.free()


def _first_failure(out, what):
    if out["status"].any():
        bad = int(np.flatnonzero(out["status"])[0])
        raise ValueError(f"{what} {bad} does not verify: status {int(out['status'][bad])} at level {int(out['fail_level'][bad])}")


def account_storage_roots(ctx, account_proofs, addresses, state_root):
    """ProofQuery::verify_state_proof (eth.rs:376-399) of every (accountProof, 20-byte address) under one state root, on the device:
    the keys are keccak256(address) (keccak256_batch_dev), the leaves are judged as accounts. Returns (a DeviceBuffer of the
    storage roots [count][32], which the caller frees and may pass as `roots` / `storage_root` of the storage walks, the same as an
    array); raises ValueError naming the first failing proof, its status and level."""
    count = len(account_proofs)
    if len(addresses) != count or any(len(a) != 20 for a in addresses):
        raise ValueError("one 20-byte address per account proof is needed")
    rows, _ = rows_at_stride([bytes(a) for a in addresses], 24)
    d_addr, d_keys, d_roots = ctx.to_device(rows), ctx.alloc(32 * count), ctx.alloc(32 * count)
    try:
        keccak256_batch_dev(ctx, d_addr, 24, None, 20, count, d_keys)
        out = verify_mpt_proofs(ctx, MptProofSet.from_proofs(account_proofs), d_keys, state_root, MPT_VALUE_ACCOUNT, d_words=d_roots)
        _first_failure(out, "account proof")
    except BaseException:
        d_roots.free()
        raise
    finally:
        d_addr.free()
        d_keys.free()
    return d_roots, out["words"]


def storage_proof_words(ctx, proofs, storage_root, slot, mapping_keys, table_info, extracted_column_identifiers, key_ids, evm_word=0,
                        variant=POSEIDON2):
    """What storage_leaf_words does, through whole proofs: from the eth_getProof storage proofs of one (slot, evm_word) of a table
    and their mapping keys to the leaves' words and values digests without a host computation. storage_slot_keys_dev (the MPT key
    of every leaf), mpt_open_nodes_dev and mpt_verify_paths_dev (every distinct node hashed and opened once, every path walked from
    storage_root, 32 bytes or a DeviceBuffer that starts with them, down to its leaf), leaf_values_digests_dev over the words left
    on the device. Returns (words [count][32], (encodings [count][5], Weierstrass [count][11], (encoding, Weierstrass) of the
    sum)); raises ValueError naming the first failing proof, its status and level."""
    count, n_keys = len(proofs), len(mapping_keys)
    if len(key_ids) != n_keys or any(len(k) != count for k in mapping_keys):
        raise ValueError("one key identifier per mapping level and one key per proof and level are needed")
    info, n = extracted_first(table_info, extracted_column_identifiers)
    front = info[:n]
    d_keys = ctx.to_device(_keys(*mapping_keys)) if n_keys else None
    d_mpt, d_words = ctx.alloc(32 * count), ctx.alloc(32 * count)
    bufs = [b for b in (d_keys, d_mpt, d_words) if b is not None]
    try:
        if storage_slot_keys_dev(ctx, slot, None, d_keys, n_keys, evm_word, count, None, d_mpt, None):
            raise OverflowError("location + evm_word leaves 256 bits")
        out = verify_mpt_proofs(ctx, MptProofSet.from_proofs(proofs), d_mpt, storage_root, MPT_VALUE_WORD, d_words=d_words, root_stride=0)
        _first_failure(out, "storage proof")
        digests = leaf_values_digests_dev(ctx, variant, [c.identifier for c in front], [c.layout() for c in front], len(table_info), d_words,
                                          d_keys, key_ids, evm_word, count, None, each=True, total=True)
        return out["words"], digests
    finally:
        for b in bufs:
            b.free()


# ---- every node of the trie: the public inputs of the values-extraction proofs ---------------------------------------------------
GOLDILOCKS_P = 0xFFFFFFFF00000001
NEUTRAL_WEIERSTRASS = (0,) * 10 + (1,)
PUBLIC_INPUT_LEN = 96  # H 8, K 64, T 1, DV 11, DM 11, N 1 (public_inputs.rs:23-36)


def mpt_subtree_digests(ctx, proof_set, mpt_keys, d_status, d_leaf_frac, d_info=None, points=True):
    """DV and N of every node of the trie the proofs of proof_set show (mpt_subtree_digests_dev). mpt_keys [count][32] (an array or
    a DeviceBuffer); d_status: the statuses verify over the same set left on the device, or None (every proof counts as OK);
    d_leaf_frac: the leaves' digests by proof, as leaf_values_digests_dev leaves them in d_frac_out (None without `points`);
    d_info: stage 1's info words when they are on the device already, otherwise the nodes are opened here. A per-node digest
    needs node = position: build the set with by_position=True, or read the CONFLICT states. Returns the outputs by name: w
    [n_nodes][5], weierstrass [n_nodes][11] (None without `points`), n_leaves, state, via, parent (uint32), entered (uint8),
    totals (rejected proofs, conflict nodes, levels), and hashes / info when the nodes were opened here."""
    count, max_depth, n = len(proof_set), proof_set.paths.shape[1], len(proof_set.nodes)
    out = {"w": None, "weierstrass": None, "hashes": None, "info": None}
    shapes = {"n_leaves": np.uint32, "state": np.uint32, "via": np.uint32, "parent": np.uint32, "entered": np.uint8}
    bufs = []
    try:
        d_paths = d_depths = d_keys = None
        if count:
            d_paths, d_depths = ctx.to_device(proof_set.paths), ctx.to_device(proof_set.depths)
            bufs += [d_paths, d_depths]
            d_keys = _device_bytes32(ctx, mpt_keys, count, bufs)[0]
        if d_info is None and n:
            rows, lens = rows_at_stride(proof_set.nodes)
            d_nodes, d_lens, d_hashes, d_info = ctx.to_device(rows), ctx.to_device(lens), ctx.alloc(32 * max(n, 1)), ctx.alloc(4 * max(n, 1))
            bufs += [d_nodes, d_lens, d_hashes, d_info]
            mpt_open_nodes_dev(ctx, d_nodes, rows.shape[1], d_lens, n, d_hashes, d_info)
            out["hashes"], out["info"] = d_hashes.download((n, 32), np.uint8), d_info.download((n,), np.uint32)
        d_acc = ctx.alloc(160 * max(n, 1)) if points else None
        d_out = {name: ctx.alloc(np.dtype(t).itemsize * max(n, 1)) for name, t in shapes.items()}
        bufs += [b for b in [d_acc] + list(d_out.values()) if b is not None]
        out["totals"] = mpt_subtree_digests_dev(ctx, d_info, n, d_paths, d_depths, max_depth, d_keys, d_status, count,
                                                d_leaf_frac if points else None, d_acc, *(d_out[name] for name in MPT_SUBTREE_OUTPUTS))
        for name, t in shapes.items():
            out[name] = d_out[name].download((n,), t)
        if points:
            out["w"], out["weierstrass"] = curve_emit_dev(ctx, d_acc, n)
        return out
    finally:
        for b in bufs:
            b.free()


def values_extraction_public_inputs(hashes, info, keys, out, dm=None):
    """The 96 public inputs (public_inputs.rs:23-36) every node's values-extraction proof exposes, [n_nodes][96] uint64: H, the node's
    hash as eight little-endian u32; K, the 64 nibbles of the key of proof via[x]; T, the key pointer after the node, which counts
    from the leaf's end (mpt_sequential/key.rs:18-55: 63 at the start, minus the nibbles of the node and of everything below it, so
    entered - 1, and p - 1 at a root); DV, the node's values digest (Weierstrass, 11 limbs); DM, the table's metadata digest `dm`
    (11 limbs; None: the neutral point); N, the leaves below the node. hashes [n_nodes][32] and keys [count][32] are those of the
    walk, `out` what mpt_subtree_digests returned. info [n_nodes] is held against the table's size and otherwise not read: T
    follows from `entered` alone. An UNREACHED node's K and T are zero."""
    hashes, keys = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32), np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32)
    n = hashes.shape[0]
    if len(info) != n or any(len(out[name]) != n for name in ("weierstrass", "n_leaves", "via", "entered")):
        raise ValueError("one hash, info word and output row per node are needed")
    rows = np.zeros((n, PUBLIC_INPUT_LEN), dtype=np.uint64)
    rows[:, :8] = hashes.view("<u4")
    reached = np.flatnonzero(out["via"] != MPT_NO_NODE)
    k = keys[out["via"][reached]]
    rows[reached, 8:72:2], rows[reached, 9:72:2] = k >> 4, k & 15
    rows[reached, 72] = (out["entered"][reached].astype(np.uint64) + np.uint64(GOLDILOCKS_P - 1)) % np.uint64(GOLDILOCKS_P)
    rows[:, 73:84] = out["weierstrass"]
    rows[:, 84:95] = np.asarray(NEUTRAL_WEIERSTRASS if dm is None else dm, dtype=np.uint64)
    rows[:, 95] = out["n_leaves"]
    return rows


def storage_proof_tree(ctx, proofs, storage_root, slot, mapping_keys, table_info, extracted_column_identifiers, key_ids, evm_word=0,
                       variant=POSEIDON2, dm=None):
    """storage_proof_words carried on to every node of the trie: the MPT keys, the nodes opened and the paths walked from
    storage_root (32 bytes or a DeviceBuffer that starts with them), the leaves' values digests, and from them the digest and the
    leaf count of every node the proofs show (mpt_subtree_digests). Every hash, walk and sum runs on the device. The host does the
    bookkeeping between them: it downloads the MPT keys and the info words of the distinct nodes and indexes the proofs by
    position with them (MptProofSet.from_proofs(by_position=True, mpt_keys=..., node_info=...)). Returns (words [count][32], the
    leaves' digests as storage_proof_words returns them, the per-node outputs of mpt_subtree_digests by name with hashes and info, the
    public-input rows [n_nodes][96] of values_extraction_public_inputs under the metadata digest `dm`); raises ValueError naming
    the first failing proof, its status and level."""
    count, n_keys = len(proofs), len(mapping_keys)
    if len(key_ids) != n_keys or any(len(k) != count for k in mapping_keys):
        raise ValueError("one key identifier per mapping level and one key per proof and level are needed")
    info, n = extracted_first(table_info, extracted_column_identifiers)
    front = info[:n]
    d_keys = ctx.to_device(_keys(*mapping_keys)) if n_keys else None
    d_mpt, d_words, d_frac = ctx.alloc(32 * max(count, 1)), ctx.alloc(32 * max(count, 1)), ctx.alloc(160 * max(count, 1))
    bufs = [b for b in (d_keys, d_mpt, d_words, d_frac) if b is not None]
    try:
        if storage_slot_keys_dev(ctx, slot, None, d_keys, n_keys, evm_word, count, None, d_mpt, None):
            raise OverflowError("location + evm_word leaves 256 bits")
        mpt_keys = d_mpt.download((count, 32), np.uint8)
        # every distinct node is hashed and opened once, over the table by bytes; the table by position repeats those rows
        by_bytes = MptProofSet.from_proofs(proofs)
        rows, lens = rows_at_stride(by_bytes.nodes)
        n_bytes = len(lens)
        bufs += [ctx.to_device(rows), ctx.to_device(lens), ctx.alloc(32 * max(n_bytes, 1)), ctx.alloc(4 * max(n_bytes, 1))]
        mpt_open_nodes_dev(ctx, bufs[-4], rows.shape[1], bufs[-3], n_bytes, bufs[-2], bufs[-1])
        hashes, words = bufs[-2].download((n_bytes, 32), np.uint8), bufs[-1].download((n_bytes,), np.uint32)
        ps = MptProofSet.from_proofs(proofs, by_position=True, mpt_keys=mpt_keys, node_info=dict(zip(by_bytes.nodes, words.tolist())))
        where = {node: j for j, node in enumerate(by_bytes.nodes)}
        src = np.array([where[node] for node in ps.nodes], dtype=np.int64)
        rows, lens, hashes, words = rows[src], lens[src], hashes[src], words[src]
        n_nodes, max_depth = len(lens), ps.paths.shape[1]
        for a in (rows, lens, ps.paths, ps.depths, hashes, words):
            bufs.append(ctx.to_device(a))
        d_nodes, d_lens, d_paths, d_depths, d_hashes, d_info = bufs[-6:]
        d_root, _ = _device_bytes32(ctx, storage_root, count, bufs)
        bufs += [ctx.alloc(4 * max(count, 1)), ctx.alloc(4 * max(count, 1))]
        d_status, d_level = bufs[-2:]
        mpt_verify_paths_dev(ctx, d_nodes, rows.shape[1], d_lens, d_hashes, d_info, n_nodes, d_paths, d_depths, max_depth, d_mpt, count, d_root, 0,
                             MPT_VALUE_WORD, d_status, d_level, d_words)
        _first_failure({"status": d_status.download((count,), np.uint32), "fail_level": d_level.download((count,), np.uint32)}, "storage proof")
        digests = leaf_values_digests_dev(ctx, variant, [c.identifier for c in front], [c.layout() for c in front], len(table_info), d_words,
                                          d_keys, key_ids, evm_word, count, d_frac, each=True, total=True)
        tree = mpt_subtree_digests(ctx, ps, d_mpt, d_status, d_frac, d_info=d_info)
        tree["hashes"], tree["info"] = hashes, words
        return d_words.download((count, 32), np.uint8), digests, tree, values_extraction_public_inputs(tree["hashes"], tree["info"], mpt_keys, tree, dm)
    finally:
        for b in bufs:
            b.free()
