"""Edge-valued inputs for the tests that go through the C ABI (tests/test_gpu_edge_operands.py and its MP2G_NTT_V1 child): rows drawn
from the canonical edge lattice of tests/field_cases.py, and the NTT cases built from them. Seeded, so that the parent and the child
process construct the same arrays. Further down: the case lists of the permutation, lookup-scan and opening-point tests, shared by the
GPU files and by tests/test_argument_edge_inputs.py, which checks them on the reference alone."""
import hashlib

import numpy as np

import field_cases as F
import oracle as O

EC = np.array(F.EC, dtype=np.uint64)
NTT_LOG_N = [3, 6, 9, 11, 12, 13, 15]  # single-pass tiles, the LT >= 11 global-twiddle round, the two-pass kernels
NTT_BATCH = 3
NTT_MODES = [{}, {"inverse": True}, {"coset_shift": O.MULT_GEN}, {"inverse": True, "coset_shift": O.MULT_GEN}, {"bitrev_out": True}]


def edge_rows(shape, seed):
    """an array of the given shape with every entry drawn from the canonical lattice"""
    return EC[np.random.default_rng(seed).integers(0, len(EC), size=shape)]


def constant_rows(width):
    """one row per lattice value, all entries equal"""
    return np.repeat(EC[:, None], width, axis=1)


def oracle_ntt(a, inverse=False, coset_shift=0, bitrev_out=False):
    out = O.fft(a, inverse=inverse, coset_shift=coset_shift)
    return out[:, O.bitrev_perm(a.shape[1])] if bitrev_out else out


def ntt_cases(log_n):
    """(label, input, mode, expected) for one size.
    'in': edge-valued inputs in every mode. 'out': inputs whose transform is edge-valued -- the oracle's inverse transform of an
    edge row e, so that the transform must return e itself and the last butterfly round lands on sums and differences at 0, p - 1
    and just across p; the same with the directions swapped, and through the coset."""
    e = edge_rows((NTT_BATCH, 1 << log_n), 7000 + log_n)
    for i, mode in enumerate(NTT_MODES):
        yield "in%d" % i, e, mode, oracle_ntt(e, **mode)
    g = O.MULT_GEN
    yield "out-fwd", O.fft(e, inverse=True), {}, e
    yield "out-inv", O.fft(e), {"inverse": True}, e
    yield "out-coset", O.fft(e, inverse=True, coset_shift=g), {"coset_shift": g}, e
    yield "out-inv-coset", O.fft(e, coset_shift=g), {"inverse": True, "coset_shift": g}, e
    yield "out-bitrev", O.fft(e, inverse=True), {"bitrev_out": True}, e[:, O.bitrev_perm(1 << log_n)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


# ---- the permutation argument (tests/test_gpu_permutation_edges.py, tests/test_argument_edge_inputs.py) ------------------------
P = O.P
# lattice values whose negation is no lattice value: w + gamma = 0 then has no solution w in the lattice
GAMMAS_A = np.array([g for g in F.EC if (P - g) % P not in set(F.EC)], dtype=np.uint64)
# (log_n, num_routed, degree, nc): one row pair, two chunks, the ZP_MAX_CHUNKS = 16 and ZP_MAX_ROUTED = 256 limits of zperm.hip,
# degree 1, two rows per lane in the scan (n = 2048 > 1024 lanes), the prover's own 80 routed wires
PERM_SHAPES = [(1, 8, 8, 1), (2, 16, 8, 2), (5, 16, 8, 2), (6, 128, 8, 2), (4, 256, 16, 2), (4, 16, 1, 1), (11, 16, 4, 2), (10, 80, 8, 2)]
PERM_EXACT_SHAPES = PERM_SHAPES[:2]  # also compared with Python integers
PERM_PLANTED_SHAPES = [(5, 16, 8, 2), (6, 128, 8, 2)]
# recipe B's challenge pairs (betas, gammas); 0, 1 and p - 1 each appear as a beta and as a gamma. beta = 0 makes every chunk
# quotient 1, so it only ever sits in the second slot: a case with one challenge never gets it
PERM_B_FIXED = [((1, P - 1), (P - 1, 0)), ((P - 1, 0), (1, 1)), ((0xFFFFFFFF, 1), (0, P - 1))]
PERM_RECIPES = ["A0", "A1", "B0", "B1", "B2", "B3"]


def root_of_unity(log_n):
    return pow(7277203076849721926, 1 << (32 - log_n), P)


def _perm_draw(shape, recipe, seed):
    log_n, num_routed, degree, nc = shape
    n = 1 << log_n
    k = int(recipe[1:])
    rng = np.random.default_rng(seed)
    if recipe[0] == "A":
        wires, sigmas = edge_rows((num_routed + 3, n), seed + 1), edge_rows((num_routed, n), seed + 2)
        betas = O.rand_field(nc, seed + 3)
        gammas = GAMMAS_A[rng.integers(0, len(GAMMAS_A), size=nc)]
    else:
        wires, sigmas = O.rand_field((num_routed + 3, n), seed + 1), O.rand_field((num_routed, n), seed + 2)
        if k < len(PERM_B_FIXED):
            betas, gammas = (np.array(v[:nc], dtype=np.uint64) for v in PERM_B_FIXED[k])
        else:
            betas, gammas = EC[rng.integers(1, len(EC), size=nc)], EC[rng.integers(0, len(EC), size=nc)]
    return wires, sigmas, betas, gammas


def perm_informative(want):
    """the condition on a reference output under which equality with it says something: no zero word (Z has not collapsed) and
    a word >= 2^63 (the values are not all small)"""
    return bool((want != 0).all() and (want >= np.uint64(1 << 63)).any())


def perm_case(shape, recipe):
    """(wires [num_routed + 3][n], sigmas [num_routed][n], betas [nc], gammas [nc], want) of one unplanted case, want being the
    oracle's output.
    A: wires and sigmas from the lattice, gammas from GAMMAS_A, betas uniform. B: wires and sigmas uniform, betas and gammas from
    the lattice (B0..B2: the fixed pairs above, B3: seeded draws). Never all four from the lattice: Z then collapses to zero.
    The seed is the first of 16 whose REFERENCE output is informative (the two-word output of the smallest shape has no word
    >= 2^63 half of the time); the code under test has no part in the choice."""
    base = 9000 + 100 * PERM_SHAPES.index(shape) + 16 * PERM_RECIPES.index(recipe)
    for seed in range(base, base + 16):
        wires, sigmas, betas, gammas = _perm_draw(shape, recipe, seed)
        want = O.partial_products_and_zs(wires, sigmas, betas, gammas, shape[2])
        if perm_informative(want):
            return wires, sigmas, betas, gammas, want
    raise AssertionError("no informative reference output for %r %s" % (shape, recipe))


def perm_planted_case(shape):
    """recipe A0 of the shape with two planted zeros in the last quarter of the rows, both in a middle chunk:
    a zero DENOMINATOR factor for challenge 0 at (wire jd, row rd), a zero NUMERATOR factor for challenge 1 at (wire jn, row rn).
    Returns (wires, sigmas, betas, gammas, plant) with plant = {challenge: (row, chunk)}."""
    log_n, num_routed, degree, nc = shape
    assert nc == 2
    n, chunks = 1 << log_n, num_routed // degree
    wires, sigmas, betas, gammas, _ = perm_case(shape, "A0")
    wires = wires.copy()
    kd = kn = chunks // 2
    jd, rd = kd * degree + 3, 3 * n // 4 + 1
    jn, rn = kn * degree + 5, 3 * n // 4 + 4
    wires[jd, rd] = (-(int(betas[0]) * int(sigmas[jd, rd]) + int(gammas[0]))) % P
    x = pow(O.MULT_GEN, jn, P) * pow(root_of_unity(log_n), rn, P) % P
    wires[jn, rn] = (-(int(betas[1]) * x + int(gammas[1]))) % P
    return wires, sigmas, betas, gammas, {0: (rd, kd), 1: (rn, kn)}


def perm_exact(wires, sigmas, betas, gammas, degree):
    """partial_products_and_zs restated on Python integers (inverse-or-zero for a zero denominator)"""
    num_routed, n = sigmas.shape
    chunks, nc = num_routed // degree, len(betas)
    log_n = n.bit_length() - 1
    xs = [pow(root_of_unity(log_n), i, P) for i in range(n)]
    ks = [pow(O.MULT_GEN, j, P) for j in range(num_routed)]
    out = np.zeros((nc * chunks, n), dtype=np.uint64)
    for c in range(nc):
        b, g, z = int(betas[c]), int(gammas[c]), 1
        for i in range(n):
            out[c, i] = z
            for k in range(chunks):
                num = den = 1
                for j in range(k * degree, (k + 1) * degree):
                    num = num * (int(wires[j, i]) + b * ks[j] * xs[i] + g) % P
                    den = den * (int(wires[j, i]) + b * int(sigmas[j, i]) + g) % P
                z = z * num * pow(den, P - 2, P) % P
                if k < chunks - 1:
                    out[nc + c * (chunks - 1) + k, i] = z
    return out


# ---- the lookup scan (tests/test_gpu_lookup_scan.py) ------------------------------------------------------------------------
SCAN_LANES = 64  # lookup_scan_kernel: one wave per (table, challenge round, proof), a run of ceil(total / 64) rows per lane
# (table entries L, lookups k, log_n, total rows, LookupTable rows): per = 1 with every lane busy; per = 2 and per = 3 with a
# lane whose run holds the last table row and the first lookup row, followed by a lane with one row; a one-entry table
SCAN_CASES = [(1586, 100, 8, 64, 61), (1638, 80, 8, 65, 63), (3328, 41, 9, 130, 128), (1, 3, 6, 2, 1)]


def scan_table(L):
    return [(v, (v * 40503 + 7) & 0xFFFF) for v in range(L)]


def scan_runs(total):
    """[(t0, t1)] per lane: walk positions t0 .. t1 - 1 (position t visits row first_lut_row - t), as the kernel splits them"""
    per = -(-total // SCAN_LANES)
    return [(min(l * per, total), min(l * per + per, total)) for l in range(SCAN_LANES)]


def scan_rows(lut):
    """(total rows, LookupTable rows) of one table of a built circuit"""
    return lut["first_lut_row"] - lut["last_lu_row"] + 1, lut["first_lut_row"] - lut["last_lut_row"] + 1


# ---- opening points (tests/test_gpu_fri_points.py) --------------------------------------------------------------------------
OPENING_POINTS = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (P - 1, P - 1), (0, P - 1), (0x1D4B3A5C6E7F8091, 0x0F1E2D3C4B5A6978)]


def ext_eval_exact(coeffs, point):
    """every row of coeffs [w][n] at the point of F_p[X]/(X^2 - 7), on Python integers: sum_i c_i point^i as [w][2]"""
    za, zb = int(point[0]), int(point[1])
    pa, pb = [1], [0]
    for _ in range(coeffs.shape[1] - 1):
        a, b = pa[-1], pb[-1]
        pa.append((a * za + 7 * b * zb) % P)
        pb.append((a * zb + b * za) % P)
    c = coeffs.astype(object)
    return np.stack([c.dot(np.array(pa, dtype=object)) % P, c.dot(np.array(pb, dtype=object)) % P], axis=1).astype(np.uint64)
