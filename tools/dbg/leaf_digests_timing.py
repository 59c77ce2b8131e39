"""time the values digests of the storage leaves of a mapping (mp2g_leaf_values_digests_dev: the cut of the columns out of the EVM
words, the digests and their sum in one call) beside the route that was there before it for the same data
(mp2g_row_digest_batch_dev over columns cut on the host beforehand, the key as a fifth column and as the unique column), in ONE
process, device resident, the two legs alternating:
    python tools/dbg/leaf_digests_timing.py [log_leaves [rounds]]
Both legs are asked for the encoding of the sum only, so both allocate their points' buffer, reduce it and end in a synchronise.
Device events (mp2g_timer_*) around every single call after a warm-up of both; median, minimum and maximum per leg. The two sums
are compared word for word before anything is timed (the same group element: evm_word == 0 and every table column extracted)."""
import importlib, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mp2 = importlib.import_module("mapreduce-plonky2_amd")
LOG = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
LAYOUT = [(12, 0, 160), (8, 0, 32), (5, 3, 13), (0, 0, 40)]  # an address, a u32, an odd bit field, five bytes
IDS, KEY_ID = np.array([101, 102, 103, 104], dtype=np.uint64), 105


def host_cut(words, byte, bit, length):
    """extract_value of every word [count][32] on the host, as 8 big-endian u32 words: the field's bits, byte-aligned from the left,
    the last byte moved down by 8 - length % 8, the bytes left-padded"""
    k, m = (length + 7) // 8, length % 8
    bits = np.unpackbits(words, axis=1)
    field = np.zeros((len(words), 8 * k), dtype=np.uint8)
    lo = 8 * byte + bit
    take = min(8 * k, 256 - lo)
    field[:, :take] = bits[:, lo:lo + take]
    b = np.packbits(field, axis=1)
    if m:
        b[:, -1] >>= 8 - m
    out = np.zeros((len(words), 32), dtype=np.uint8)
    out[:, 32 - k:] = b
    return out.view(">u4").astype(np.uint32)


def main():
    ctx = mp2.Context(0)
    n = 1 << LOG
    rng = np.random.default_rng(0x1EAF)
    words = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    keys = np.zeros((n, 1, 32), dtype=np.uint8)
    keys[:, 0, 12:] = rng.integers(0, 256, size=(n, 20), dtype=np.uint8)  # address keys, left-padded
    key_col = keys.reshape(n, 32).view(">u4").astype(np.uint32)
    values = np.stack([host_cut(words, *lay) for lay in LAYOUT] + [key_col], axis=1)  # [n][5][8]
    assert np.array_equal(values[:4096, :4], mp2.extract_values(ctx, words[:4096], LAYOUT)), "host cut != device cut"
    d_words, d_keys = ctx.to_device(words), ctx.to_device(keys)
    d_ids, d_values, d_unique = ctx.to_device(np.append(IDS, np.uint64(KEY_ID))), ctx.to_device(values), ctx.to_device(key_col)

    def leg_a():
        return mp2.leaf_values_digests_dev(ctx, 0, IDS, LAYOUT, 4, d_words, d_keys, [KEY_ID], 0, n, None, each=False, total=True)[2][0]

    def leg_b():
        return mp2.compute_table_row_digest_dev(ctx, d_ids, 5, d_values, d_unique, 1, n)

    a, b = leg_a(), leg_b()  # the warm-up, and the comparison
    assert np.array_equal(a, b), (a, b)
    print(f"2^{LOG} mapping leaves, 4 extracted columns + the key column, Poseidon2; sums equal: {a.tolist()}", flush=True)
    ta, tb = [], []
    for _ in range(ROUNDS):
        for leg, out in ((leg_a, ta), (leg_b, tb)):
            ctx.timer_start()
            leg()
            out.append(ctx.timer_stop())
    for name, t in (("A mp2g_leaf_values_digests_dev", ta), ("B mp2g_row_digest_batch_dev over host-cut columns", tb)):
        print(f"  {name}: median {statistics.median(t):.3f} ms, min {min(t):.3f}, max {max(t):.3f}  ({' '.join(f'{x:.3f}' for x in t)})", flush=True)
    print(f"  A - B (medians): {statistics.median(ta) - statistics.median(tb):+.3f} ms", flush=True)
    # the cut alone, into the cell format
    d_out = ctx.alloc(n * 4 * 32)
    mp2.extract_values_dev(ctx, d_words, LAYOUT, n, d_out)
    tc = []
    for _ in range(ROUNDS):
        ctx.timer_start()
        mp2.extract_values_dev(ctx, d_words, LAYOUT, n, d_out)
        tc.append(ctx.timer_stop())
    print(f"  mp2g_extract_values_dev, 4 columns: median {statistics.median(tc):.3f} ms, min {min(tc):.3f}, max {max(tc):.3f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
