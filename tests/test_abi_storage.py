"""The Keccak-256 entry points are declared in include/mp2g.h with the widths the Python host binds them with, the library exports
them, and the host-side names of the reference are importable (no GPU needed)."""
import ctypes
import importlib

import pytest

ABI = importlib.import_module("mapreduce-plonky2_amd._abi")
V, U32, U64, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
PROTOTYPES = {
    "mp2g_keccak256_batch": (I, [V, V, U32, V, U32, U32, V]),
    "mp2g_keccak256_batch_dev": (I, [V, V, U32, V, U32, U32, V]),
    "mp2g_storage_slot_keys": (I, [V, U64, V, V, U32, U32, U32, V, V, V, V]),
    "mp2g_storage_slot_keys_dev": (I, [V, U64, V, V, U32, U32, U32, V, V, V, V]),
    "mp2g_mpt_storage_leaves": (I, [V, V, U32, V, V, U32, V, V, V, V]),
    "mp2g_mpt_storage_leaves_dev": (I, [V, V, U32, V, V, U32, V, V, V, V]),
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


def test_status_codes_match_the_header(mp2):
    text = open(mp2.HEADER_PATH).read()
    for name, value in (("OK", 0), ("MALFORMED", 1), ("NOT_A_LEAF", 2), ("BAD_VALUE", 3), ("KEY_MISMATCH", 4)):
        assert f"MP2G_MPT_LEAF_{name} = {value}" in text and getattr(mp2, "MPT_LEAF_" + name) == value


def test_refusals_need_no_device(mp2):
    """every argument is judged before the context is touched"""
    lib = mp2.load()
    buf = ctypes.create_string_buffer(64)
    for stride in (0, 12, 65544):
        assert lib.mp2g_keccak256_batch(None, buf, stride, None, 0, 1, buf) != 0
        assert b"stride" in lib.mp2g_last_error()
    assert lib.mp2g_keccak256_batch(None, buf, 8, None, 9, 1, buf) != 0 and b"len" in lib.mp2g_last_error()
    assert lib.mp2g_storage_slot_keys(None, 256, None, buf, 1, 0, 1, None, None, None, None) != 0 and b"slot" in lib.mp2g_last_error()
    assert lib.mp2g_storage_slot_keys(None, 0, None, buf, 3, 0, 1, None, None, None, None) != 0 and b"n_keys" in lib.mp2g_last_error()
    assert lib.mp2g_keccak256_batch(None, None, 8, None, 0, 0, None) == 0 and lib.mp2g_mpt_storage_leaves(None, None, 8, None, None, 0, None, None, None, None) == 0


def test_host_names(mp2):
    X = importlib.import_module("mapreduce-plonky2_amd.extraction")
    S = X.StorageSlot
    m = S.mapping(b"\x01\x02", 0x105)
    inner = S.node_mapping(m, b"\x03")
    field = S.node_struct(inner, 2)
    assert (m.slot(), inner.slot(), field.slot(), S.simple(7).slot()) == (5, 5, 5, 7)  # `as u8`
    assert (m.evm_offset(), inner.evm_offset(), field.evm_offset()) == (0, 0, 2)
    assert S.simple(7).is_simple_slot() and S.node_struct(S.simple(7), 1).is_simple_slot() and not field.is_simple_slot()
    assert S.simple(7).mapping_keys() == [] and field.mapping_keys() == [b"\x01\x02", b"\x03"]
    assert S.mapping(b"\x01\x02", 0x105) == m and S.mapping(b"\x01", 0x105) != m
    with pytest.raises(ValueError):
        S.node_mapping(S.simple(7), b"\x03")
    with pytest.raises(ValueError):
        S.node_mapping(S.node_struct(m, 1), b"\x03")
    assert X.bytes_to_nibbles(b"\xab\x0f") == [0xA, 0xB, 0x0, 0xF]
    for name in ("location", "mpt_key", "mpt_nibbles"):
        assert callable(getattr(S, name)), name
    assert callable(X.storage_leaf_words)
    for name in ("keccak256_batch", "keccak256_batch_dev", "storage_slot_keys", "storage_slot_keys_dev", "mpt_storage_leaves",
                 "mpt_storage_leaves_dev"):
        assert callable(getattr(mp2, name)), name
    rows, lens = mp2.rows_at_stride([b"", b"abc", bytes(9)])
    assert rows.shape == (3, 16) and lens.tolist() == [0, 3, 9] and bytes(rows[1]) == b"abc" + bytes(13)
