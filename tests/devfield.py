"""ctypes loader for tests/devfield/libmp2g_devfield.so: the device bodies of csrc's arithmetic headers behind element-wise kernels
(tests/devfield/field_dev.hip) -- test infrastructure only. Operations are looked up by the names the library itself reports."""
import ctypes
import os
import subprocess

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devfield")
LIB = os.path.join(DIR, "libmp2g_devfield.so")
_lib = None
_scalar_ops = {}
_vec_ops = {}


def build():
    """incremental `make`, serialised across processes as tests/oracle.py does: a stale or missing library is rebuilt, never skipped"""
    import fcntl
    with open(os.path.join(DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            subprocess.check_call(["make", "-s", "-C", DIR])
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(LIB)
        L.mp2gt_scalar_op_name.restype = ctypes.c_char_p
        L.mp2gt_vec_op_name.restype = ctypes.c_char_p
        for table, name_of in ((_scalar_ops, L.mp2gt_scalar_op_name), (_vec_ops, L.mp2gt_vec_op_name)):
            op = 0
            while name_of(op) is not None:
                table[name_of(op).decode()] = op
                op += 1
        _lib = L
    return _lib


def scalar_ops():
    lib()
    return dict(_scalar_ops)


def vec_ops():
    lib()
    return dict(_vec_ops)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check(status, what):
    if status != 0:
        raise RuntimeError("%s: HIP status %d" % (what, status))


def scalar(name, *cols):
    """(o0, o1) of the named scalar operation on up to three operand columns"""
    L = lib()
    n = len(cols[0])
    ins = [_u64(c) for c in cols] + [np.zeros(n, dtype=np.uint64)] * (3 - len(cols))
    assert all(c.shape == (n,) for c in ins)
    o0, o1 = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    _check(L.mp2gt_scalar(_scalar_ops[name], ctypes.c_size_t(n), _p(ins[0]), _p(ins[1]), _p(ins[2]), _p(o0), _p(o1)), name)
    return o0, o1


def cols(terms, f, a, b):
    """gl_cols::value() after `terms` add (f = 0) or add_scaled(.., f) calls per row of a, b"""
    a, b = _u64(a), _u64(b)
    n = a.shape[0]
    assert a.shape == b.shape == (n, terms)
    out = np.empty(n, dtype=np.uint64)
    _check(lib().mp2gt_cols(terms, f, ctypes.c_size_t(n), _p(a), _p(b), _p(out)), "gl_cols")
    return out


def vec(name, x, y=None, rc=None, k=0):
    """(out [n][width], flag [n]) of the named vector operation; y: second operand per case, rc: 12 shared round constants"""
    L = lib()
    op = _vec_ops[name]
    w = L.mp2gt_vec_op_width(op)
    x = _u64(x)
    n = x.shape[0]
    assert x.shape == (n, w)
    second, shared = None, 0
    if y is not None:
        second = _u64(y)
        assert second.shape == (n, w)
    elif rc is not None:
        second, shared = _u64(rc), 1
        assert second.shape == (12,)
    out, flag = np.empty((n, w), dtype=np.uint64), np.empty(n, dtype=np.uint64)
    _check(L.mp2gt_vec(op, ctypes.c_size_t(n), _p(x), _p(second) if second is not None else None, shared, ctypes.c_uint32(k),
                       _p(out), _p(flag)), name)
    return out, flag
