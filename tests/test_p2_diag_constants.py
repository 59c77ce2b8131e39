"""The folded constants of Poseidon2's internal diagonal (POSEIDON2_DIAG_M1_SHL32, POSEIDON2_DIAG_NARROW: csrc/poseidon.cuh derives
them from perm_constants.h's POSEIDON2_DIAG_M1 at compile time; tools/hosttest/mulc_host_test --constants prints what the compiler
made of them) recomputed from the table they derive from, the column bounds that gl_mulc_addw's comment (csrc/gl.cuh) rests on, and
the routine's portable body (mulc_host_test REQUEST RESULT) against exact Python integers on the operands of tests/p2_diag_cases.py.
The device body faces the same operands in tests/test_gpu_p2_diag.py."""
import subprocess

import numpy as np
import pytest

import field_cases as F
import hosttest
import p2_diag_cases as C

P, M = F.P, F.M32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("hosttest"), "mulc_host_test", flags=("-O2", "-DMP2G_DEVCONST=static const"), mp2g_h=False)


@pytest.fixture(scope="module")
def compiled(exe):
    """(POSEIDON2_DIAG_M1_SHL32, POSEIDON2_DIAG_NARROW) as compiled into the program"""
    words = [int(x, 16) for x in subprocess.run([exe, "--constants"], capture_output=True, text=True, check=True).stdout.split()]
    assert len(words) == 13
    return words[:12], words[12]


def test_folded_constants(compiled):
    d, e = F.header_table("POSEIDON2_DIAG_M1"), compiled[0]
    assert e == [(x << 32) % P for x in d]
    assert all(0 < x < P for x in d + e)


def test_narrow_mask_and_column_bounds(compiled):
    d = F.header_table("POSEIDON2_DIAG_M1")
    e, mask = compiled
    assert mask == sum(1 << k for k in range(12) if (d[k] >> 32) + (e[k] >> 32) <= (1 << 32) - 3)
    for k in range(12):
        d0, d1, e0, e1 = d[k] & M, d[k] >> 32, e[k] & M, e[k] >> 32
        # the largest value of every column, all operands at their ends (a0 = a1 = c0 = c1 = M and full carry words)
        p0 = M * d0 + M
        p1 = M * d1 + (p0 >> 32) + M
        q0 = M * e0 + M
        addend = p1 + (q0 >> 32)
        q1 = M * e1 + addend
        assert p0 < 1 << 64 and p1 < 1 << 64 and q0 < 1 << 64 and addend < 1 << 64
        if (mask >> k) & 1:
            assert q1 < 1 << 64, "a narrow pair takes no carry"
        else:
            assert q1 < 1 << 65 and (q1 - (1 << 64)) + F.EPS < 1 << 64, "the carry's + EPS cannot wrap"


def test_column_cases_reach_the_33rd_bit(compiled):
    """the operands really put X on both sides of 2^96 for the three pairs that are not narrow"""
    d = F.header_table("POSEIDON2_DIAG_M1")
    mask = compiled[1]
    for k in range(12):
        e = (d[k] << 32) % P
        xs = [(a & M) * d[k] + (a >> 32) * e + c for a, c in C.column_cases(d[k])]
        if not (mask >> k) & 1:
            assert 1 << 96 in xs and (1 << 96) - 1 in xs and max(xs) > 1 << 96
        else:
            assert max(xs) < 1 << 96


@pytest.mark.parametrize("k", range(12))
def test_portable_body(exe, tmp_path, k):
    a, c = C.cases(k, n_uniform=1 << 12)
    req, res = tmp_path / "request.bin", tmp_path / "result.bin"
    req.write_bytes(np.array([len(a), k], dtype=np.uint64).tobytes() + a.tobytes() + c.tobytes())
    r = subprocess.run([exe, str(req), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(res, dtype=np.uint64)
    assert out.size == len(a)
    bad = C.bad_cases(k, a, c, out)
    assert not bad, "k=%d: %d wrong, first a=%#x c=%#x out=%#x" % (k, len(bad), int(a[bad[0]]), int(c[bad[0]]), int(out[bad[0]]))
