"""time the three Keccak-256 kernels (csrc/storage.hip) at the sizes a storage table has, device resident, in ONE process:
    python tools/dbg/keccak_timing.py [log_leaves [rounds]]
  A  mp2g_storage_slot_keys_dev      2^log mapping leaves (one 20-byte key, slot 5): 2 permutations per leaf
  B  mp2g_mpt_storage_leaves_dev     2^log 69-byte leaf nodes (64-nibble path, 31-byte value) held against their keys: 1 permutation
  C  mp2g_keccak256_batch_dev        2^(log-4) 532-byte nodes (MAX_BRANCH_NODE_LEN): 4 permutations per node
Device events (mp2g_timer_*) around every single call after a warm-up of all three, the legs alternating; median, minimum and
maximum per leg, and the derived hashes/s and permutations/s. A few outputs of every leg are compared with the plain-Python sponge
of tests/keccak_cases.py before anything is timed. For scale, the host's hashlib.sha3_256 over the same bytes, one call per hash on
one core: the same permutation under another domain byte, so a fair per-hash CPU cost (the digests differ)."""
import hashlib, importlib, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
mp2 = importlib.import_module("mapreduce-plonky2_amd")
import keccak_cases as K
LOG = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
SLOT = 5


def main():
    ctx = mp2.Context(0)
    n, n_long = 1 << LOG, 1 << max(LOG - 4, 0)
    rng = np.random.default_rng(0x6ECCA6)
    keys = np.zeros((n, 1, 32), dtype=np.uint8)
    keys[:, 0, 12:] = rng.integers(0, 256, size=(n, 20), dtype=np.uint8)  # address keys, left-padded
    # 69-byte leaves: f8 43 | a1 20 <32 path bytes> | a0 9f <31 value bytes>, the path being the whole key
    paths = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    nodes = np.zeros((n, 72), dtype=np.uint8)
    nodes[:, :4] = (0xF8, 0x43, 0xA1, 0x20)
    nodes[:, 4:36] = paths
    nodes[:, 36:38] = (0xA0, 0x9F)
    nodes[:, 38:69] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
    nodes[:, 69:] = 0xA5
    lens = np.full(n, 69, dtype=np.uint32)
    long_nodes = rng.integers(0, 256, size=(n_long, 536), dtype=np.uint8)
    d_keys, d_nodes, d_lens, d_paths, d_long = (ctx.to_device(a) for a in (keys, nodes, lens, paths, long_nodes))
    d_loc, d_mpt, d_nib = ctx.alloc(32 * n), ctx.alloc(32 * n), ctx.alloc(64 * n)
    d_hash, d_words, d_nn, d_status = ctx.alloc(32 * n), ctx.alloc(32 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)
    d_long_out = ctx.alloc(32 * n_long)

    def leg_a():
        mp2.storage_slot_keys_dev(ctx, SLOT, None, d_keys, 1, 0, n, d_loc, d_mpt, d_nib, overflow=False)

    def leg_b():
        mp2.mpt_storage_leaves_dev(ctx, d_nodes, 72, d_lens, d_paths, n, d_hash, d_words, d_nn, d_status)

    def leg_c():
        mp2.keccak256_batch_dev(ctx, d_long, 536, None, 532, n_long, d_long_out)

    legs = (("A mp2g_storage_slot_keys_dev", leg_a, n, 2), ("B mp2g_mpt_storage_leaves_dev", leg_b, n, 1), ("C mp2g_keccak256_batch_dev", leg_c, n_long, 4))
    for _, leg, _, _ in legs:  # the warm-up, and the comparison
        leg()
    ctx.sync()
    loc, mpt, nib = (d.download((8, w), np.uint8) for d, w in ((d_loc, 32), (d_mpt, 32), (d_nib, 64)))
    for i in range(8):
        want = K.slot_keys(SLOT, None, [bytes(keys[i, 0])], 0)
        assert (bytes(loc[i]), bytes(mpt[i]), bytes(nib[i])) == want[:3], "slot keys != restatement"
        assert bytes(d_hash.download((8, 32), np.uint8)[i]) == K.keccak256(bytes(nodes[i, :69])), "leaf hash != restatement"
        assert bytes(d_words.download((8, 32), np.uint8)[i]) == b"\0" + bytes(nodes[i, 38:69]), "leaf word != the node's value"
        assert bytes(d_long_out.download((8, 32), np.uint8)[i]) == K.keccak256(bytes(long_nodes[i, :532])), "long hash != restatement"
    assert not d_status.download((n,), np.uint32).any() and (d_nn.download((n,), np.uint32) == 64).all()
    print(f"2^{LOG} mapping leaves / 69-byte leaf nodes, 2^{max(LOG - 4, 0)} 532-byte nodes; outputs equal the restatement on the first 8", flush=True)
    times = {name: [] for name, *_ in legs}
    for _ in range(ROUNDS):
        for name, leg, _, _ in legs:
            ctx.timer_start()
            leg()
            times[name].append(ctx.timer_stop())
    for name, _, count, perms in legs:
        t = times[name]
        med = statistics.median(t)
        print(f"  {name}: median {med:.3f} ms, min {min(t):.3f}, max {max(t):.3f}  ({' '.join(f'{x:.3f}' for x in t)})", flush=True)
        print(f"      {count * (2 if name[0] == 'A' else 1) / med / 1e3:.1f} M hashes/s, {count * perms / med / 1e3:.1f} M permutations/s (median)", flush=True)
    # the host, for scale: one core, one hashlib call per hash
    for name, msgs, per in (("A' hashlib.sha3_256, 2 x 64- and 32-byte messages per leaf", keys.reshape(n, 32), 2), ("B' hashlib.sha3_256, 69-byte nodes", nodes, 1),
                            ("C' hashlib.sha3_256, 532-byte nodes", long_nodes, 4)):
        rows = [bytes(r) for r in (msgs[:, :69] if per == 1 else (msgs[:, :532] if per == 4 else msgs))]
        t0 = time.perf_counter()
        if per == 2:
            pad = bytes(31) + bytes([SLOT])
            for r in rows:
                hashlib.sha3_256(hashlib.sha3_256(r + pad).digest()).digest()
        else:
            for r in rows:
                hashlib.sha3_256(r).digest()
        dt = time.perf_counter() - t0
        print(f"  {name}: {dt * 1e3:.1f} ms, {len(rows) * (2 if per == 2 else 1) / dt / 1e6:.2f} M hashes/s, {len(rows) * per / dt / 1e6:.2f} M permutations/s", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
