"""The storage-leaf entry points are declared in include/mp2g.h with the widths the Python host binds them with, the library exports
them, and the host-side names of the reference are importable (no GPU needed)."""
import ctypes
import importlib

ABI = importlib.import_module("mapreduce-plonky2_amd._abi")
V, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
PROTOTYPES = {
    "mp2g_extract_values": (I, [V, V, V, U32, U32, V]),
    "mp2g_extract_values_dev": (I, [V, V, V, U32, U32, V]),
    "mp2g_leaf_values_digests": (I, [V, I, V, V, U32, U32, V, V, V, U32, U32, U32, V, V, V, V]),
    "mp2g_leaf_values_digests_dev": (I, [V, I, V, V, U32, U32, V, V, V, U32, U32, U32, V, V, V, V, V]),
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


def test_host_names(mp2):
    X = importlib.import_module("mapreduce-plonky2_amd.extraction")
    info = [X.ColumnInfo(3, 11, 0, 0, 8, 0), X.ColumnInfo(4, 12, 1, 0, 8, 0), X.ColumnInfo(3, 13, 0, 0, 256, 1), X.ColumnInfo(3, 14, 2, 0, 16, 0)]
    assert X.filter_table_column_identifiers(info, 3, 0) == [11, 14]
    assert X.filter_table_column_identifiers(info, 3, 1) == [13]
    assert X.filter_table_column_identifiers(info, 5, 0) == []
    ordered, n = X.extracted_first(info, [14, 12])
    assert n == 2 and [c.identifier for c in ordered] == [12, 14, 11, 13]  # stable: table order inside each part
    assert X.left_pad32(b"\x01\x02") == bytes(30) + b"\x01\x02" and X.left_pad32(b"") == bytes(32)
    for name in ("leaf_single_values_digests", "leaf_mapping_values_digests", "leaf_mapping_of_mappings_values_digests",
                 "leaf_single_metadata_digest", "leaf_mapping_metadata_digest", "leaf_mapping_of_mappings_metadata_digest"):
        assert callable(getattr(X, name)), name
    for name in ("extract_values", "extract_values_dev", "leaf_values_digests", "leaf_values_digests_dev"):
        assert callable(getattr(mp2, name)), name
