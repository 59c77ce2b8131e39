"""csrc/keccak.cuh compiled for the host into tools/hosttest/keccak_host_test (its own main, no GPU, no library): the permutation and
the sponge that the kernels of csrc/storage.hip compile, against the restatement of tests/keccak_cases.py over the length lattice,
with two different fillings of the bytes past every message's end."""
import subprocess

import numpy as np
import pytest

import hosttest
import keccak_cases as K


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("hosttest"), "keccak_host_test", mp2g_h=False)


def run(exe, tmp, msgs, stride, domain, fill):
    rows = np.full((len(msgs), stride), fill, dtype=np.uint8)
    for r, m in zip(rows, msgs):
        r[:len(m)] = np.frombuffer(m, dtype=np.uint8)
    req, res = tmp / "request.bin", tmp / "result.bin"
    req.write_bytes(np.array([len(msgs), stride, domain, 0], dtype=np.uint32).tobytes() + np.array([len(m) for m in msgs], dtype=np.uint32).tobytes()
                    + rows.tobytes())
    r = subprocess.run([exe, str(req), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(res, dtype=np.uint8).reshape(2, len(msgs), 32)


def test_length_lattice(exe, tmp_path):
    msgs = [K.message(n) for n in K.LENGTHS] + list(K.mixed_batch()[:32])
    want = [K.keccak256(m) for m in msgs]
    for fill in (0xA5, 0x5A):
        got, regs = run(exe, tmp_path, msgs, K.STRIDE, 0x01, fill)
        assert [bytes(g) for g in got] == want, fill
        for m, g, r in zip(msgs, got, regs):
            assert bytes(r) == (bytes(g) if len(m) in (32, 64) else bytes(32))  # the one-block form from registers


def test_rows_that_end_at_the_stride(exe, tmp_path):
    """len == stride and len just below it: the last word of the row is loaded, nothing past it"""
    for stride in (8, 136, 272):
        msgs = [K.message(n, 3) for n in range(max(0, stride - 9), stride + 1)]
        got, _ = run(exe, tmp_path, msgs, stride, 0x01, 0xEE)
        assert [bytes(g) for g in got] == [K.keccak256(m) for m in msgs], stride


def test_golden_answers_and_sha3_domain(exe, tmp_path):
    import hashlib
    msgs = [bytes.fromhex(k["message_hex"]) for k in K.GOLDEN["keccak256"]]
    got, regs = run(exe, tmp_path, msgs, 64, 0x01, 0xFF)
    assert [bytes(g).hex() for g in got] == [k["digest_hex"] for k in K.GOLDEN["keccak256"]]
    assert bytes(regs[2]).hex() == K.GOLDEN["keccak256"][2]["digest_hex"] and bytes(regs[3]).hex() == K.GOLDEN["keccak256"][3]["digest_hex"]
    msgs = [K.message(n, 5) for n in (0, 135, 136, 137, 300)]
    got, _ = run(exe, tmp_path, msgs, 304, 0x06, 0x11)
    assert [bytes(g) for g in got] == [hashlib.sha3_256(m).digest() for m in msgs]
