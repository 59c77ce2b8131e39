"""mp2g_keccak256_batch[_dev] (csrc/keccak.cuh, csrc/storage.hip, csrc/storage_api.hip) against the plain-Python sponge of
tests/keccak_cases.py, bit for bit: the length lattice around the 8-byte word and the 136-byte rate block, the counts around the
wave and the block, a wave whose lanes run different block counts, and the bytes a call must neither read into the result nor
write."""
import ctypes

import numpy as np
import pytest

import keccak_cases as K

pytestmark = pytest.mark.gpu


def rows_of(msgs, stride, fill):
    rows = np.full((len(msgs), stride), fill, dtype=np.uint8)
    for r, m in zip(rows, msgs):
        r[:len(m)] = np.frombuffer(m, dtype=np.uint8)
    return rows, np.array([len(m) for m in msgs], dtype=np.uint32)


def want_of(msgs):
    return np.frombuffer(b"".join(K.keccak256(m) for m in msgs), dtype=np.uint8).reshape(len(msgs), 32)


@pytest.mark.parametrize("count", K.COUNTS)
def test_uniform_length(ctx, mp2, count):
    """lens NULL: every message has `len` bytes; the bytes in [len, stride) are garbage of two kinds and change nothing"""
    lib = mp2.load()
    for n in K.LENGTHS:
        msgs = [K.message(n, i) for i in range(count)]
        want = want_of(msgs)
        for fill in (0xA5, 0x5A):
            rows, _ = rows_of(msgs, K.STRIDE, fill)
            out = np.zeros((count, 32), dtype=np.uint8)
            assert lib.mp2g_keccak256_batch(ctx, mp2._p(rows), K.STRIDE, None, n, count, mp2._p(out)) == 0, lib.mp2g_last_error()
            assert np.array_equal(out, want), (n, fill)


def test_mixed_lengths_host_form(ctx, mp2):
    msgs = list(K.mixed_batch())
    assert len(msgs) == 129 and {len(m) for m in msgs} == set(K.LENGTHS)
    assert np.array_equal(mp2.keccak256_batch(ctx, msgs), want_of(msgs))
    assert np.array_equal(mp2.keccak256_batch(ctx, msgs, stride=1024), want_of(msgs))


def test_mixed_lengths_device_form(ctx, mp2):
    """a wave with unequal block counts and a grid tail; a guard region after `count` rows of out stays untouched and so do the
    inputs; two garbage patterns past every message's end give the same digests"""
    msgs = list(K.mixed_batch())
    count, guard = len(msgs), 4
    want = want_of(msgs)
    for fill in (0xC3, 0x3C):
        rows, lens = rows_of(msgs, K.STRIDE, fill)
        rows = np.concatenate([rows, np.full((guard, K.STRIDE), fill ^ 0xFF, dtype=np.uint8)])
        planted = np.full((count + guard, 32), 0x77, dtype=np.uint8)
        d_rows, d_lens, d_out = ctx.to_device(rows), ctx.to_device(lens), ctx.to_device(planted)
        mp2.keccak256_batch_dev(ctx, d_rows, K.STRIDE, d_lens, 0, count, d_out)
        got = d_out.download((count + guard, 32), np.uint8)
        assert np.array_equal(got[:count], want) and (got[count:] == 0x77).all(), fill
        assert np.array_equal(d_rows.download(rows.shape, np.uint8), rows) and np.array_equal(d_lens.download((count,), np.uint32), lens)
        for d in (d_rows, d_lens, d_out):
            d.free()


def test_device_lengths_are_clamped_to_the_stride(ctx, mp2):
    stride = 144
    msgs = [K.message(stride, i) for i in range(65)]
    rows, _ = rows_of(msgs, stride, 0)
    lens = np.array([stride + 1 + 1000 * i for i in range(64)] + [0xFFFFFFFF], dtype=np.uint32)
    guard = np.full((2, stride), 0xEE, dtype=np.uint8)
    outs = []
    for g in (guard, guard ^ 0xFF):  # the rows after the batch differ between the two runs
        d_rows, d_lens, d_out = ctx.to_device(np.concatenate([rows, g])), ctx.to_device(lens), ctx.alloc(65 * 32)
        mp2.keccak256_batch_dev(ctx, d_rows, stride, d_lens, 0, 65, d_out)
        outs.append(d_out.download((65, 32), np.uint8))
        for d in (d_rows, d_lens, d_out):
            d.free()
    assert np.array_equal(outs[0], want_of(msgs)) and np.array_equal(outs[1], outs[0])


def test_golden_answers(ctx, mp2):
    msgs = [bytes.fromhex(k["message_hex"]) for k in K.GOLDEN["keccak256"]]
    got = mp2.keccak256_batch(ctx, msgs)
    assert [bytes(g).hex() for g in got] == [k["digest_hex"] for k in K.GOLDEN["keccak256"]]
    # pack(Endianness::Little): the digest read as eight little-endian u32 words
    assert got[0].view("<u4").tolist()[0] == int.from_bytes(bytes.fromhex("c5d24601"), "little")


def test_refusals_write_nothing(ctx, mp2):
    lib, p = mp2.load(), mp2._p
    rows, lens = rows_of([K.message(9), K.message(64)], 64, 0)
    planted = np.full((2, 32), 0x77, dtype=np.uint8)
    d_rows, d_lens, d_out = ctx.to_device(np.concatenate([rows, rows])), ctx.to_device(lens), ctx.to_device(planted)

    def refused(word, host_args, dev_args):
        out = planted.copy()
        if host_args is not None:
            assert lib.mp2g_keccak256_batch(ctx, *host_args(out)) != 0
            assert word in lib.mp2g_last_error().decode(), lib.mp2g_last_error()
            assert np.array_equal(out, planted)
        if dev_args is not None:
            assert lib.mp2g_keccak256_batch_dev(ctx, *dev_args) != 0
            assert word in lib.mp2g_last_error().decode(), lib.mp2g_last_error()
            assert np.array_equal(d_out.download((2, 32), np.uint8), planted)

    for stride in (0, 12, 60, 65544):
        refused("stride", lambda o: (p(rows), stride, p(lens), 0, 2, p(o)), (d_rows, stride, d_lens, 0, 2, d_out))
    refused("len", lambda o: (p(rows), 64, None, 65, 2, p(o)), (d_rows, 64, None, 65, 2, d_out))
    too_long = np.array([9, 65], dtype=np.uint32)
    refused("lens: entry 1", lambda o: (p(rows), 64, p(too_long), 0, 2, p(o)), None)
    refused("msgs", lambda o: (None, 64, p(lens), 0, 2, p(o)), (None, 64, d_lens, 0, 2, d_out))
    refused("out", None, (d_rows, 64, d_lens, 0, 2, None))
    assert lib.mp2g_keccak256_batch(ctx, p(rows), 64, p(lens), 0, 2, None) != 0 and b"out" in lib.mp2g_last_error()
    refused("msgs is not 8-byte aligned", None, (ctypes.c_void_p(d_rows.ptr.value + 4), 64, d_lens, 0, 2, d_out))
    refused("out is not 8-byte aligned", None, (d_rows, 64, d_lens, 0, 2, ctypes.c_void_p(d_out.ptr.value + 4)))
    refused("lens is not 4-byte aligned", None, (d_rows, 64, ctypes.c_void_p(d_lens.ptr.value + 2), 0, 2, d_out))
    # an aligned offset is taken, count == 0 launches nothing, and len == stride is a whole row
    mp2.keccak256_batch_dev(ctx, ctypes.c_void_p(d_rows.ptr.value + 64), 64, None, 64, 1, d_out)
    assert bytes(d_out.download((2, 32), np.uint8)[0]) == K.keccak256(K.message(64))
    assert lib.mp2g_keccak256_batch_dev(ctx, None, 64, None, 0, 0, None) == 0 and lib.mp2g_keccak256_batch(None, None, 64, None, 0, 0, None) == 0
    for d in (d_rows, d_lens, d_out):
        d.free()
