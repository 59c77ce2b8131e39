"""States for Poseidon2's internal layer that aim at its limb sum (p2_limb_sum, csrc/poseidon.cuh): pure Python, no product code.

The device body adds the twelve limbs as wrapping 64-bit integers (W), sums their high words exactly (H), recovers the carry c of the
low words' sum as (hi32(W) - lo32(H)) mod 2^32 and hands gl_reduce96w the pair (W, top) with top = (H + c) >> 32. `model(state)` follows
that sequence on Python integers; the tables below drive c and top through all of 0..11, put the subtract that recovers c on both
sides of its wrap, and H at its maximum. tests/test_gpu_p2_internal_sum.py runs the device body on them, tests/test_p2_internal_sum_cases.py
the portable body and the checks of the tables themselves."""
import numpy as np

import field_cases as F

P, M32, M64 = F.P, F.M32, F.M64
N_UNIFORM = 1 << 16
HI_ONLY = 0xFFFFFFFF00000000


def model(state):
    """the device sequence on the twelve limbs -> dict(W, H, c, top); W + 2^64 top is the exact sum"""
    w = sum(state) & M64
    h = sum(x >> 32 for x in state)
    c = ((w >> 32) - (h & M32)) & M32
    top = (h + c) >> 32
    return {"W": w, "H": h, "c": c, "top": top, "wraps": (w >> 32) < (h & M32)}


def _spread(total, n):
    """n words below 2^32 that sum to `total` (total <= n (2^32 - 1))"""
    out = []
    for i in range(n):
        v = min(M32, total)
        out.append(v)
        total -= v
    assert total == 0
    return out


def structured():
    """list of (label, state) with hand-made states"""
    rows = []
    for k in range(13):
        rows.append(("%d limbs 2^64-1" % k, [M64] * k + [0] * (12 - k)))  # top = max(k - 1, 0), c = max(k - 1, 0)
        rows.append(("%d limbs 2^32-1" % k, [M32] * k + [0] * (12 - k)))  # H = 0, c = max(k - 1, 0)
        rows.append(("%d limbs 2^64-1, at the end" % k, [0] * (12 - k) + [M64] * k))
    rows.append(("all high words full", [HI_ONLY] * 12))  # H = 12 (2^32 - 1), c = 0
    # high words that sum to 2^32 - 1 and to 2^32 exactly (over two limbs and over all twelve), with low words that carry 0, 1 and 11:
    # lo32(H) is 2^32 - 1 or 0, so hi32(W) - lo32(H) wraps in the first case whenever c > 0 does not lift hi32(W) past it
    for total in (M32, M32 + 1):
        for his in (_spread(total, 2) + [0] * 10, [total // 12 + (1 if i < total % 12 else 0) for i in range(12)]):
            assert sum(his) == total
            for los in ([0] * 12, [1] * 12, [M32, 1] + [0] * 10, [M32, M32] + [0] * 10, [M32] * 12, [M32] * 11 + [1]):
                rows.append(("H = %#x" % total, [(h << 32) | l for h, l in zip(his, los)]))
    for v in (P - 1, P, P + 1):
        rows.append(("all limbs %#x" % v, [v] * 12))
        for i in range(12):
            rows.append(("limb %d = %#x" % (i, v), [v if j == i else 0 for j in range(12)]))
    return rows


def lattice_rows(seed=0x51AB):
    """every edge word of field_cases.EANY in one limb at a time, the other eleven seeded uniform"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, M64, size=(12 * len(F.EANY), 12), dtype=np.uint64, endpoint=True)
    r = 0
    for i in range(12):
        for e in F.EANY:
            out[r, i] = e
            r += 1
    return out


def states(n_uniform=N_UNIFORM):
    """uint64 [n][12]: the structured rows, the one-limb lattice, then n_uniform seeded uniform states"""
    s = np.array([st for _, st in structured()], dtype=np.uint64)
    rng = np.random.default_rng(0x5EED12)
    uni = rng.integers(0, M64, size=(n_uniform, 12), dtype=np.uint64, endpoint=True)
    return np.concatenate([s, lattice_rows(), uni])


_want = {}


def reference(n_uniform=N_UNIFORM):
    """(states, field_cases.p2_internal_matrix() applied to each), computed once per size and shared"""
    if n_uniform not in _want:
        st = states(n_uniform)
        _want[n_uniform] = (st, F.mat_apply(F.p2_internal_matrix(), st.tolist()))
    return _want[n_uniform]
