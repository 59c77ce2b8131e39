"""time the two MPT inclusion-proof kernels (csrc/mpt.hip) over the proofs of one table, device resident, in ONE process (run it under
a time limit: `timeout -k 10 300 python tools/dbg/mpt_timing.py [log_leaves [rounds]]`, log_leaves a multiple of 4):
  1  mp2g_mpt_open_nodes_dev       the distinct nodes of a 2^log-leaf trie: 2^log leaves of 66 to 69 bytes and (2^log - 1) / 15 full 532-byte
                                   branches, at stride 536: every node hashed (1 and 4 permutations) and opened
  2  mp2g_mpt_verify_paths_dev     the trie's 2^log paths of log / 4 branches and a leaf, over stage 1's hashes and info words
for scale, the parent commit's kernels in the same process:
  L  mp2g_mpt_storage_leaves_dev   the same leaves alone, hashed, opened and held against their keys
  K  mp2g_keccak256_batch_dev      the same node table, hashed only
The trie is regular (every key prefix of log / 4 nibbles occurs once, the other nibbles are random), so it is built level by level
with the library's own Keccak, whose digests the restatement of tests/keccak_cases.py then checks on a sample; the info words of a
sample of nodes and the whole walk of the first paths are compared with tests/mpt_cases.py before anything is timed. Device
events (mp2g_timer_*) around every single call after a warm-up of all legs, the legs alternating; median, minimum, maximum and the
raw times per leg."""
import ctypes, importlib, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
mp2 = importlib.import_module("mapreduce-plonky2_amd")
import keccak_cases as K
import mpt_cases as M
LOG = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
STRIDE = 536


def build(hash_rows):
    """(rows [n_nodes][536], lens, paths [n][levels + 1], keys [n][32], number of branches): branches first, level by level from the
    root; hash_rows(uint8 [m][len]) gives the Keccak-256 digests [m][32] of m nodes of one length"""
    levels, n = LOG // 4, 1 << LOG
    rng = np.random.default_rng(0x3B7)
    idx = np.arange(n, dtype=np.uint32)
    nib = rng.integers(0, 16, size=(n, 64), dtype=np.uint8)
    for j in range(levels):  # the prefix: leaf i's first log / 4 nibbles are i's, the high nibble first
        nib[:, j] = (idx >> (LOG - 4 * (j + 1))) & 15
    keys = nib[:, 0::2] << 4 | nib[:, 1::2]
    # the leaf's path: the key's nibbles after the prefix behind the hex-prefix flag (2 0 when they are even in number, 3 when odd)
    rest = nib[:, levels:]
    flag = np.full((n, 1), 3, dtype=np.uint8) if rest.shape[1] & 1 else np.tile(np.array([2, 0], dtype=np.uint8), (n, 1))
    hp = np.concatenate([flag, rest], axis=1)
    path = hp[:, 0::2] << 4 | hp[:, 1::2]
    value = rng.integers(1, 256, size=(n, 31), dtype=np.uint8)
    item0 = np.concatenate([np.full((n, 1), 0x80 + path.shape[1], dtype=np.uint8), path], axis=1)
    item1 = np.concatenate([np.full((n, 1), 0xA0, dtype=np.uint8), np.full((n, 1), 0x9F, dtype=np.uint8), value], axis=1)
    payload = np.concatenate([item0, item1], axis=1)
    assert 56 <= payload.shape[1] < 256
    leaves = np.concatenate([np.full((n, 1), 0xF8, dtype=np.uint8), np.full((n, 1), payload.shape[1], dtype=np.uint8), payload], axis=1)
    leaf_len = leaves.shape[1]
    level_rows, child = [], leaves
    for _ in range(levels):  # from the leaves' parents up to the root
        hashes = hash_rows(child)
        m = len(hashes) // 16
        br = np.zeros((m, 532), dtype=np.uint8)
        br[:, :3] = (0xF9, 0x02, 0x11)
        body = br[:, 3:531].reshape(m, 16, 33)
        body[:, :, 0] = 0xA0
        body[:, :, 1:] = hashes.reshape(m, 16, 32)
        br[:, 531] = 0x80
        level_rows.append(br)
        child = br
    branches = np.concatenate(level_rows[::-1])
    n_br = len(branches)
    rows = np.full((n_br + n, STRIDE), 0xA5, dtype=np.uint8)
    rows[:n_br, :532] = branches
    rows[n_br:, :leaf_len] = leaves
    lens = np.concatenate([np.full(n_br, 532, dtype=np.uint32), np.full(n, leaf_len, dtype=np.uint32)])
    paths = np.zeros((n, levels + 1), dtype=np.uint32)
    first = 0
    for lv in range(levels):  # the branch of level lv on leaf i's path is the one of i's first lv nibbles
        paths[:, lv] = first + (idx >> (LOG - 4 * lv))
        first += 1 << (4 * lv)
    paths[:, levels] = n_br + idx
    return rows, lens, paths, keys, n_br


def main():
    assert LOG % 4 == 0 and 4 <= LOG <= 24
    ctx = mp2.Context(0)
    rows, lens, paths, keys, n_br = build(lambda nodes: mp2.keccak256_batch(ctx, nodes))
    n, n_nodes, depth = 1 << LOG, len(lens), paths.shape[1]
    root = K.keccak256(bytes(rows[0, :532]))
    d_rows, d_lens, d_paths, d_keys = (ctx.to_device(a) for a in (rows, lens, paths, keys))
    d_depths, d_root = ctx.to_device(np.full(n, depth, dtype=np.uint32)), ctx.to_device(np.frombuffer(root, dtype=np.uint8))
    d_hashes, d_info, d_plain = ctx.alloc(32 * n_nodes), ctx.alloc(4 * n_nodes), ctx.alloc(32 * n_nodes)
    d_out = [ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(32 * n), ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(depth * n)]
    d_leaf = [ctx.alloc(32 * n), ctx.alloc(32 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)]
    leaf_rows = ctypes.c_void_p(d_rows.ptr.value + STRIDE * n_br)
    leaf_lens = ctypes.c_void_p(d_lens.ptr.value + 4 * n_br)

    def leg_1():
        mp2.mpt_open_nodes_dev(ctx, d_rows, STRIDE, d_lens, n_nodes, d_hashes, d_info)

    def leg_2():
        mp2.mpt_verify_paths_dev(ctx, d_rows, STRIDE, d_lens, d_hashes, d_info, n_nodes, d_paths, d_depths, depth, d_keys, n, d_root, 0,
                                 mp2.MPT_VALUE_WORD, *d_out)

    def leg_l():
        mp2.mpt_storage_leaves_dev(ctx, leaf_rows, STRIDE, leaf_lens, d_keys, n, *d_leaf)

    def leg_k():
        mp2.keccak256_batch_dev(ctx, d_rows, STRIDE, d_lens, 0, n_nodes, d_plain)

    legs = (("1 mp2g_mpt_open_nodes_dev", leg_1, n_nodes), ("2 mp2g_mpt_verify_paths_dev", leg_2, n), ("L mp2g_mpt_storage_leaves_dev", leg_l, n),
            ("K mp2g_keccak256_batch_dev", leg_k, n_nodes))
    for _, leg, _ in legs:  # the warm-up, and the comparison
        leg()
    ctx.sync()
    hashes, info = d_hashes.download((n_nodes, 32), np.uint8), d_info.download((n_nodes,), np.uint32)
    assert np.array_equal(hashes, d_plain.download((n_nodes, 32), np.uint8)), "stage 1's hashes != mp2g_keccak256_batch_dev"
    node = lambda i: bytes(rows[i, :lens[i]])
    sample = sorted({int(x) for x in paths[:4].ravel()} | {n_br - 1, n_nodes - 1})
    for i in sample:
        assert bytes(hashes[i]) == K.keccak256(node(i)) and int(info[i]) == M.open_node(node(i)), f"node {i} != restatement"
    status, level, words, val_off, val_len, consumed = (d.download(s, t) for d, (s, t) in zip(d_out, (
        ((n,), np.uint32), ((n,), np.uint32), ((n, 32), np.uint8), ((n,), np.uint32), ((n,), np.uint32), ((n, depth), np.uint8))))
    assert not status.any() and not level.any() and (consumed == np.arange(depth, dtype=np.uint8)).all(), "a proof of the built trie fails"
    table = {i: node(i) for i in sample}
    for i in range(4):
        want = M.walk(_Sparse(table, n_nodes), _Sparse({j: bytes(hashes[j]) for j in sample}, n_nodes), _Sparse({j: int(info[j]) for j in sample}, n_nodes),
                      [int(x) for x in paths[i]], depth, bytes(keys[i]), root, M.WORD, depth)
        assert (want["status"], want["word"], want["val_off"], want["val_len"]) == (0, bytes(words[i]), int(val_off[i]), int(val_len[i])), "walk != restatement"
    assert np.array_equal(words, d_leaf[1].download((n, 32), np.uint8)) and not d_leaf[3].download((n,), np.uint32).any(), "words != mp2g_mpt_storage_leaves_dev"
    print(f"2^{LOG} proofs of {depth} nodes over {n_nodes} distinct nodes ({n_br} 532-byte branches, {n} {int(lens[-1])}-byte leaves); outputs equal the "
          f"restatement on {len(sample)} nodes and 4 walks, every proof OK", flush=True)
    times = {name: [] for name, *_ in legs}
    for _ in range(ROUNDS):
        for name, leg, _ in legs:
            ctx.timer_start()
            leg()
            times[name].append(ctx.timer_stop())
    for name, _, count in legs:
        t = times[name]
        med = statistics.median(t)
        print(f"  {name}: median {med:.3f} ms, min {min(t):.3f}, max {max(t):.3f}, {count / med / 1e3:.1f} M items/s  ({' '.join(f'{x:.3f}' for x in t)})", flush=True)
    ctx.close()


class _Sparse:
    """a list of which only a sample is held"""

    def __init__(self, held, n):
        self.held, self.n = held, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.held[i]


if __name__ == "__main__":
    main()
