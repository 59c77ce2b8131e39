"""The accumulated-digest entry points are declared in include/mp2g.h with the widths the Python host binds them with, the library
exports them, and the fused width is readable without a device (no GPU needed)."""
import ctypes
import importlib

ABI = importlib.import_module("mapreduce-plonky2_amd._abi")
V, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
PROTOTYPES = {
    "mp2g_curve_decode_dev": (I, [V, V, U32, V]),
    "mp2g_curve_emit_dev": (I, [V, V, V, U32, V, V]),
    "mp2g_tree_digests_dev": (I, [V, V, V, V]),
    "mp2g_tree_digests": (I, [V, V, V, V, V]),
    "mp2g_tree_digests_update_fused_width": (U32, []),
    "mp2g_tree_digests_update_dev": (I, [V, V, V, V, U32, V]),
    "mp2g_cells_tree_digests_dev": (I, [V, I, V, U32, V, U32, V, U32, V]),
    "mp2g_row_digests_dev": (I, [V, I, V, U32, V, V, U32, U32, U32, V, V, U32, V]),
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


def test_fused_width_without_a_device(mp2):
    assert mp2.load().mp2g_tree_digests_update_fused_width() == 128
    assert mp2.tree_digests_update_fused_width() == 128
