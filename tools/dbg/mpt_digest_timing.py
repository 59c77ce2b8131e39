"""time the MPT subtree digests (csrc/mpt_digest.hip) over the proofs of one table, device resident, in ONE process (run it under a time
limit: `timeout -k 10 300 python tools/dbg/mpt_digest_timing.py [log_leaves [rounds]]`, log_leaves a multiple of 4):
  S  mp2g_mpt_subtree_digests_dev, no points   the shape, and not it alone: the four passes over the 2^log proofs, the three over the nodes,
                                               the one synchronisation, and the level launches, which then count leaves only; a kernel
                                               trace of this tool (rocprofv3 --kernel-trace --stats, a run of its own) separates the passes
  D  mp2g_mpt_subtree_digests_dev              the same with the sums: D - S is the sum pass (2^log leaf loads, one addition per child
                                               that is not a branch's first)
for scale, the parent commit's kernels in the same process:
  2  mp2g_mpt_verify_paths_dev                 the same paths over the same table: the same dependent-load pattern, with the node bytes
  C  mp2g_curve_sum                            the same 2^log leaf points (host encodings: upload, decode and the block tree of additions):
                                               about the same number of additions, with no shape
The trie is mpt_timing.py's regular one (every key prefix of log / 4 nibbles occurs once). Leaf i holds base point i mod 512. Before
anything is timed the root's digest is held against mp2g_curve_sum over the leaves, its N against the leaf count, the totals
against (0, 0, log / 4 + 1), and a sample of nodes against the oracle's sum over the leaves below them. Device events
(mp2g_timer_*) around every single call after a warm-up of all legs, the legs alternating; median, minimum, maximum and the raw
times per leg, and the ratios."""
import importlib, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools", "dbg"))
mp2 = importlib.import_module("mapreduce-plonky2_amd")
import ec_cases as EC
import keccak_cases as K
import mpt_timing as T
LOG = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
STRIDE = T.STRIDE


def main():
    assert LOG % 4 == 0 and 4 <= LOG <= 24
    T.LOG = LOG
    ctx = mp2.Context(0)
    rows, lens, paths, keys, n_br = T.build(lambda nodes: mp2.keccak256_batch(ctx, nodes))
    n, n_nodes, depth = 1 << LOG, len(lens), paths.shape[1]
    root = K.keccak256(bytes(rows[0, :532]))
    pts = np.ascontiguousarray(EC.base_points(512)[np.arange(n) % 512])
    d_rows, d_lens, d_paths, d_keys = (ctx.to_device(a) for a in (rows, lens, paths, keys))
    d_depths, d_root = ctx.to_device(np.full(n, depth, dtype=np.uint32)), ctx.to_device(np.frombuffer(root, dtype=np.uint8))
    d_hashes, d_info, d_status = ctx.alloc(32 * n_nodes), ctx.alloc(4 * n_nodes), ctx.alloc(4 * n)
    d_leaf, d_acc = ctx.alloc(160 * n), ctx.alloc(160 * n_nodes)
    d_out = [ctx.alloc(4 * n_nodes) for _ in range(4)] + [ctx.alloc(n_nodes)]
    mp2.mpt_open_nodes_dev(ctx, d_rows, STRIDE, d_lens, n_nodes, d_hashes, d_info)
    mp2.curve_decode_dev(ctx, pts, d_leaf)
    totals, total = {}, {}

    def leg_s():
        totals["S"] = mp2.mpt_subtree_digests_dev(ctx, d_info, n_nodes, d_paths, d_depths, depth, d_keys, d_status, n, None, None, *d_out)

    def leg_d():
        totals["D"] = mp2.mpt_subtree_digests_dev(ctx, d_info, n_nodes, d_paths, d_depths, depth, d_keys, d_status, n, d_leaf, d_acc, *d_out)

    def leg_2():
        mp2.mpt_verify_paths_dev(ctx, d_rows, STRIDE, d_lens, d_hashes, d_info, n_nodes, d_paths, d_depths, depth, d_keys, n, d_root, 0,
                                 mp2.MPT_VALUE_WORD, d_status)

    def leg_c():
        total["C"] = mp2.curve_sum(ctx, pts, weierstrass=True)

    legs = (("S mp2g_mpt_subtree_digests_dev, no points", leg_s, n), ("D mp2g_mpt_subtree_digests_dev", leg_d, n), ("2 mp2g_mpt_verify_paths_dev", leg_2, n),
            ("C mp2g_curve_sum", leg_c, n))
    leg_2()  # the statuses the other legs read
    for _, leg, _ in legs:  # the warm-up, and the comparison
        leg()
    ctx.sync()
    assert not d_status.download((n,), np.uint32).any(), "a proof of the built trie fails"
    assert totals["S"] == totals["D"] == (0, 0, depth), totals
    n_leaves, state, via, parent = (d.download((n_nodes,), np.uint32) for d in d_out[:4])
    assert (state == mp2.MPT_SUBTREE_OK).all() and n_leaves[0] == n and (n_leaves[n_br:] == 1).all() and parent[0] == mp2.MPT_NO_NODE
    assert np.array_equal(via[n_br:], np.arange(n, dtype=np.uint32)) and np.array_equal(parent[n_br:], paths[:, depth - 2])
    sample = sorted({0, 1, n_br - 1, n_br, n_nodes - 1})
    w, wei = mp2.curve_emit_dev(ctx, d_acc, len(sample), idx=sample)
    assert np.array_equal(w[0], total["C"][0]) and np.array_equal(wei[0], total["C"][1]), "the root's digest != mp2g_curve_sum over the leaves"
    for j, x in enumerate(sample[1:], 1):
        below = np.flatnonzero((paths == x).any(axis=1))
        assert len(below) == n_leaves[x] and np.array_equal(w[j], EC.orc_sum(pts[below])[0]), f"node {x} != oracle"
    print(f"2^{LOG} proofs of {depth} nodes over {n_nodes} distinct nodes ({n_br} branches): every node OK, the root's digest equals mp2g_curve_sum over "
          f"the leaves, {len(sample) - 1} more nodes equal the oracle's sums", flush=True)
    times = {name: [] for name, *_ in legs}
    for _ in range(ROUNDS):
        for name, leg, _ in legs:
            ctx.timer_start()
            leg()
            times[name].append(ctx.timer_stop())
    med = {}
    for name, _, count in legs:
        t = times[name]
        med[name[0]] = statistics.median(t)
        print(f"  {name}: median {med[name[0]]:.3f} ms, min {min(t):.3f}, max {max(t):.3f}, {count / med[name[0]] / 1e3:.1f} M proofs/s  "
              f"({' '.join(f'{x:.3f}' for x in t)})", flush=True)
    sums = med["D"] - med["S"]
    print(f"  the sum pass (D - S): {sums:.3f} ms; shape / verify_paths = {med['S'] / med['2']:.2f}, sum pass / curve_sum = {sums / med['C']:.2f}, "
          f"whole call / verify_paths = {med['D'] / med['2']:.2f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
