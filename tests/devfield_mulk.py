"""ctypes loader for tests/devfield_mulk/libmp2g_devfield_mulk.so: gl_mulw_k, the product of the permutations' S-boxes, behind an
element-wise kernel (tests/devfield_mulk/mulk_dev.hip) -- test infrastructure only, built like tests/devfield."""
import ctypes
import os
import subprocess

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devfield_mulk")
LIB = os.path.join(DIR, "libmp2g_devfield_mulk.so")
_lib = None


def build():
    """incremental `make`, serialised across processes as tests/devfield.py does: a stale or missing library is rebuilt, never skipped"""
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
        _lib = ctypes.CDLL(LIB)
    return _lib


def mulw_k(a, b):
    """(out, canon): gl_mulw_k(a, b) as the routine returns it, and its gl_canon, for every pair of the columns a, b"""
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    n = len(a)
    assert a.shape == b.shape == (n,)
    out, canon = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    status = lib().mp2gt_mulw_k(ctypes.c_size_t(n), p(a), p(b), p(out), p(canon))
    if status != 0:
        raise RuntimeError("mulw_k: HIP status %d" % status)
    return out, canon
