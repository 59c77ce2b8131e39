"""The portable (#else) bodies of csrc/gl.cuh, gl5.cuh and poseidon.cuh, compiled for the host into tools/hosttest/perm_host_test:
the program's own run (permutations against the C oracle, primitives against unsigned __int128), then every routine that has a host
body on the operand tables of tests/field_cases.py with the checks of tests/field_checks.py -- the tables and references that the
device bodies face in tests/test_gpu_field_device.py. Device-only routines (ntt_arith.cuh, poseidon_wave.cuh, two_to_one) have no
host body."""
import os
import subprocess

import numpy as np
import pytest

import field_cases as F
import field_checks as C
import hosttest
import oracle as O

DEVICE_ONLY = {n for n in F.OPS if n.startswith(("gl_mul_2p", "gl_sub_mul_", "gl_mul_w8_", "bfly_lo_"))}


class HostBackend:
    """the interface of tests/devfield.py on top of `perm_host_test REQUEST RESULT`"""

    def __init__(self, exe, tmp):
        self.exe, self.tmp = exe, str(tmp)

    def _run(self, shape, n, p0, p1, name, arrays, out_words):
        req, res = os.path.join(self.tmp, "request.bin"), os.path.join(self.tmp, "result.bin")
        with open(req, "wb") as f:
            f.write(np.array([shape, n, p0, p1], dtype=np.uint64).tobytes())
            f.write(name.encode().ljust(32, b"\0"))
            for a in arrays:
                f.write(np.ascontiguousarray(a, dtype=np.uint64).tobytes())
        r = subprocess.run([self.exe, req, res], capture_output=True, text=True)
        assert r.returncode == 0, "%s: %s" % (name, r.stderr)
        out = np.fromfile(res, dtype=np.uint64)
        assert out.size == out_words
        return out

    def scalar(self, name, *cols):
        n = len(cols[0])
        ins = list(cols) + [np.zeros(n, dtype=np.uint64)] * (3 - len(cols))
        out = self._run(0, n, 0, 0, name, ins, 2 * n)
        return out[:n], out[n:]

    def cols(self, terms, f, a, b):
        return self._run(1, a.shape[0], terms, f, "gl_cols", [a, b], a.shape[0])

    def vec(self, name, x, y=None, rc=None, k=0):
        n, w = x.shape
        second, mode = ([y], 1) if y is not None else (([rc], 2) if rc is not None else ([], 0))
        out = self._run(2, n, k, mode, name, [x] + second, n * w + n)
        return out[:n * w].reshape(n, w), out[n * w:]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    O.build()
    return hosttest.build(tmp_path_factory.mktemp("hosttest"), "perm_host_test", flags=("-O2", "-DMP2G_DEVCONST=static const"),
                          link=("-x", "none", O.LIB, "-Wl,-rpath," + os.path.dirname(os.path.abspath(O.LIB))), mp2g_h=False)


@pytest.fixture
def H(exe, tmp_path):
    return HostBackend(exe, tmp_path)


def test_program_self_check(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "host arithmetic ok", r.stdout + r.stderr


def test_device_only_routines_are_refused(H, tmp_path):
    """a routine without a host body is an error of the program, never an empty result"""
    req = tmp_path / "request.bin"
    req.write_bytes(np.array([0, 1, 0, 0], dtype=np.uint64).tobytes() + b"gl_mul_2p24".ljust(32, b"\0") + bytes(24))
    assert subprocess.run([H.exe, str(req), str(tmp_path / "result.bin")], capture_output=True).returncode == 2


@pytest.mark.parametrize("name", sorted(set(F.OPS) - DEVICE_ONLY))
def test_scalar_operation(H, name):
    C.scalar_operation(H, name)


@pytest.mark.parametrize("terms,f", F.COLS_SHAPES)
def test_gl_cols(H, terms, f):
    C.gl_cols(H, terms, f)


def test_gl2(H):
    C.gl2(H)


def test_gl5(H):
    C.gl5_mul_sqr(H)
    for k in C.GL5_SMALL_K:
        C.gl5_small(H, k)
    for k in C.GL5_KZ_K:
        C.gl5_mul_kz(H, k)
    C.gl5_frobenius_norm_sgn0(H)
    C.gl5_inv(H)


def test_gl5_sqrt_and_is_square(H):
    C.gl5_sqrt_and_is_square(H)


def test_poseidon_layers(H):
    C.p2_external_layers(H, wave=False)
    C.p2_internal_layers(H, wave=False)
    C.poseidon_mds_layers(H)


def test_permutations(H):
    C.permutations(H, device=False)
