"""ctypes loader for tests/devfield_mulc/libmp2g_devfield_mulc.so: gl_mulc_addw over Poseidon2's internal diagonal behind an
element-wise kernel (tests/devfield_mulc/mulc_dev.hip) -- test infrastructure only, built like tests/devfield."""
import ctypes
import os
import subprocess

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devfield_mulc")
LIB = os.path.join(DIR, "libmp2g_devfield_mulc.so")
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
        _lib.mp2gt_mulc_narrow_mask.restype = ctypes.c_uint
    return _lib


def narrow_mask():
    return int(lib().mp2gt_mulc_narrow_mask())


def mulc_addw(a, c, k):
    """some u64 congruent to a d_k + c for every pair of the columns a, c"""
    a, c = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(c, dtype=np.uint64)
    n = len(a)
    assert a.shape == c.shape == (n,)
    out = np.empty(n, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    status = lib().mp2gt_mulc_addw(ctypes.c_size_t(n), p(a), p(c), ctypes.c_int(k), p(out))
    if status != 0:
        raise RuntimeError("mulc_addw(k=%d): HIP status %d" % (k, status))
    return out
