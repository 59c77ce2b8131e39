"""The Python host binds every libmp2gpu function to the prototype include/mp2g.h declares, once in load() (_abi.prototypes):
the table covers the header, the C++ front end reads the same signatures and structure layouts (tools/hosttest/abi_test.cpp, a
stand-alone program), a mistyped call is refused before the library is entered, and 64-bit scalars travel as bare Python ints. The
last test needs a GPU; the others do not."""
import ctypes
import importlib
import subprocess

import numpy as np
import pytest

import hosttest
import oracle as O
from test_abi_symbols import declared_symbols

STRUCTS = {"mp2g_fri_params": "FriParams", "mp2g_gate": "Gate", "mp2g_lookup": "Lookup", "mp2g_chain_patch": "ChainPatch",
           "mp2g_forest_circuit": "ForestCircuit"}
BIG_KEY, OLD_EPOCH = 2 ** 63 + 5, -(2 ** 40)


@pytest.fixture(scope="module")
def table(mp2):
    return importlib.import_module("mapreduce-plonky2_amd._abi").prototypes(mp2.HEADER_PATH)


def test_table_covers_the_header_and_is_bound(mp2, table):
    assert set(table) == set(declared_symbols(mp2.HEADER_PATH))
    lib = mp2.load()
    for name, (restype, argtypes) in table.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert table["mp2g_ntt"][1][5] is ctypes.c_uint64 and table["mp2g_d2d_2d"][1][2] is ctypes.c_size_t
    assert table["mp2g_forest_proved"][0] is ctypes.c_uint64 and table["mp2g_update_tree_epoch"][0] is ctypes.c_int64
    assert table["mp2g_last_error"] == (ctypes.c_char_p, []) and table["mp2g_ctx_stream"] == (ctypes.c_void_p, [ctypes.c_void_p])


def _kind(t):
    if t is None:
        return "v"
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return "p"
    return f"{ctypes.sizeof(t)}{'s' if t(-1).value < 0 else 'u'}"


def test_the_compiler_reads_the_same_signatures_and_layouts(mp2, table, tmp_path):
    names = sorted(table)
    (tmp_path / "abi_funcs.inc").write_text("".join(f"X({n})\n" for n in names))
    mirrors = {c: getattr(mp2, py) for c, py in STRUCTS.items()}
    (tmp_path / "abi_structs.inc").write_text("".join(f"S({c})\n" + "".join(f"M({c}, {f[0]})\n" for f in m._fields_) for c, m in mirrors.items()))
    exe = hosttest.build(tmp_path, "abi_test", flags=("-O2", "-I" + str(tmp_path)))
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    want = [" ".join(["F", n, str(len(table[n][1])), _kind(table[n][0])] + [_kind(t) for t in table[n][1]]) for n in names]
    for c, m in mirrors.items():
        want.append(f"S {c} {ctypes.sizeof(m)}")
        want += [f"M {c} {f[0]} {getattr(m, f[0]).offset} {getattr(m, f[0]).size}" for f in m._fields_]
    assert got == want


def test_a_header_the_table_cannot_type_or_the_library_cannot_serve_is_refused(mp2, tmp_path, monkeypatch):
    text = open(mp2.HEADER_PATH).read()
    tail = text.rindex("#ifdef __cplusplus")
    for decl, err, words in (("int mp2g_takes_a_double(mp2g_ctx* c, double x);", TypeError, ("mp2g_takes_a_double", "double x")),
                             ("float mp2g_returns_a_float(void);", TypeError, ("mp2g_returns_a_float", "float")),
                             ("int mp2g_not_in_the_library(uint32_t x);", mp2.Mp2gError, ("mp2g_not_in_the_library",))):
        h = tmp_path / "mp2g.h"
        h.write_text(text[:tail] + decl + "\n" + text[tail:])
        monkeypatch.setattr(mp2, "_lib", None)
        monkeypatch.setattr(mp2, "HEADER_PATH", str(h))
        with pytest.raises(err) as e:
            mp2.load()
        assert all(w in str(e.value) for w in words), str(e.value)
        assert mp2._lib is None
    monkeypatch.setattr(mp2, "HEADER_PATH", str(tmp_path / "absent.h"))
    with pytest.raises(mp2.Mp2gError, match="absent.h is missing"):
        mp2.load()


def test_a_mistyped_call_is_refused_before_the_library_is_entered(mp2):
    lib, h = mp2.load(), ctypes.c_void_p()
    with pytest.raises(TypeError):
        lib.mp2g_tree_shape_sbbst(3)  # one argument too few
    with pytest.raises(ctypes.ArgumentError):
        lib.mp2g_tree_shape_sbbst(3.0, ctypes.byref(h))  # uint32_t n
    assert h.value is None
    assert lib.mp2g_tree_shape_sbbst(np.uint32(3), ctypes.byref(h)) == 0
    s = mp2.TreeShape(h)
    assert (s.size, s.num_levels, s.num_roots) == (3, 2, 1)
    s.free()


def test_64_bit_scalars_survive_as_bare_ints(mp2):
    W = importlib.import_module("mapreduce-plonky2_amd.workplan")
    tree = W.UpdateTree.from_paths([[1, BIG_KEY]], epoch=OLD_EPOCH)
    assert tree.contains_key(BIG_KEY) and not tree.contains_key(BIG_KEY - 2 ** 63) and not tree.contains_key(BIG_KEY - 2 ** 32)
    assert tree.epoch == OLD_EPOCH
    assert tree.subtree_size(BIG_KEY) == 1 and tree.subtree_size(1) == 2 and tree.nodes() == [1, BIG_KEY]
    with pytest.raises(mp2.Mp2gError):
        tree.subtree_size(5)
    plan = tree.into_workplan()
    nxt = plan.next()
    assert nxt.ready and nxt.item.k == BIG_KEY
    with pytest.raises(mp2.Mp2gError):
        plan.done(5)
    plan.done(BIG_KEY)
    assert plan.next().item.k == 1
    plan.done(1)
    assert plan.completed()
    plan.free()
    m = W.UpdateTree.from_map(OLD_EPOCH, BIG_KEY, {BIG_KEY: (2 ** 40 + 1, None), 2 ** 40 + 1: (None, None)})
    assert m.epoch == OLD_EPOCH and m.root() == BIG_KEY and m.contains_key(2 ** 40 + 1) and not m.contains_key(1)
    m.free()


def test_a_device_buffer_is_its_address_as_a_parameter(mp2):
    d = mp2.DeviceBuffer.__new__(mp2.DeviceBuffer)  # no allocation: needs no GPU
    d.ctx, d.ptr = None, ctypes.c_void_p(2 ** 47 + 64)
    assert ctypes.c_void_p.from_param(d) is d.ptr
    d.ptr = None  # a freed buffer is NULL, as its .ptr was
    assert ctypes.c_void_p.from_param(d) is None


# ---- on the device --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wide_scalars_end_to_end(ctx, mp2):
    IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
    # a coset shift with every high bit set
    a = O.rand_field((2, 8), 0xAB1)
    assert np.array_equal(ctx.ntt(a, coset_shift=O.P - 1), O.fft(a, coset_shift=O.P - 1))
    # a 64-bit row-tree identifier: H(hL || hR || min || max || id || value || payload), leaves 0 and 2 under node 1
    shape = IX.TreeShape.sbbst(3)
    d = shape.describe()
    assert d["left"].tolist() == [-1, 0, -1] and d["right"].tolist() == [-1, 2, -1]
    v = np.random.default_rng(0xAB2).integers(0, 1 << 32, size=(3, 8), dtype=np.uint32)
    val = lambda i: [int(x) for x in v[i]]
    H = lambda words: [int(x) for x in O.hash_n_to_m_no_pad(np.array(words, dtype=np.uint64), 4, 0)]
    zero, ident = [0] * 4, 2 ** 63 + 1
    leaf = [H(zero + zero + val(i) + val(i) + [ident] + val(i) + zero) for i in (0, 2)]
    want = [leaf[0], H(leaf[0] + leaf[1] + val(0) + val(2) + [ident] + val(1) + zero), leaf[1]]
    got = IX.row_tree_hashes(ctx, shape, ident, v)
    assert got.tolist() == want
    assert not np.array_equal(got, IX.row_tree_hashes(ctx, shape, 1, v))
    # byte counts, offsets and pitches, every DeviceBuffer passed as itself
    src, dst = ctx.alloc(64), ctx.alloc(64)
    words = np.arange(1, 5, dtype=np.uint64)
    src.upload(np.zeros(8, dtype=np.uint64)).upload_at(words, 32)
    dst.upload(np.full(8, 7, dtype=np.uint64))
    ctx.d2d_2d(dst, 8, 16, src, 32, 16, 8, 2)
    assert src.download((8,)).tolist() == [0, 0, 0, 0, 1, 2, 3, 4]
    assert dst.download((8,)).tolist() == [7, 1, 7, 3, 7, 7, 7, 7]
    back = np.empty(8, dtype=np.uint64)
    mp2._ck(mp2.load().mp2g_d2h(ctx.h, mp2._p(back), dst, back.nbytes))
    assert back.tolist() == [7, 1, 7, 3, 7, 7, 7, 7]
    for x in (src, dst, shape):
        x.free()
