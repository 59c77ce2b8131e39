"""Operand tables and exact references for the field-arithmetic tests: pure Python, no product code.

The device bodies of csrc/gl.cuh, gl5.cuh, poseidon.cuh, poseidon_wave.cuh and ntt_arith.cuh take their rare branches (a borrow in
gl_reduce128w, a result in [p, 2^64) before the canonicalisation, the carry of gl_reduce96w ...) with probability ~2^-32 on
uniform operands. The lattice of 32-bit edge words below reaches every one of them; `branch_classes()` counts them with a model of
the device sequences, from the operands alone.

One table per operation (`OPS`): the operand domains its header comment states, the exact reference on Python integers, and how the
output is to be compared. tests/test_gpu_field_device.py runs the device bodies on these tables, tests/test_field_host.py the
portable bodies, tests/test_field_cases.py guards the tables themselves.
"""
import itertools
import os
import re
import zlib

import numpy as np

P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapreduce-plonky2_amd", "csrc")

W = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
E = sorted({(hi << 32) | lo for hi in W for lo in W})
EC = sorted({e for e in E if e < P} | {P - 1, P - 2})  # both are lattice points already: 43 values, 1849 pairs
EANY = sorted(set(E) | {P, P + 1, M64})  # all three are lattice points already: 49 values, 2401 pairs
S3 = [0, 1, M32, 0xFFFFFFFF00000000, P - 1, M64]
N_UNIFORM = 1 << 16

# operand domains: (lattice values, exclusive upper bound of the uniform draw)
DOMAINS = {
    "any": (EANY, 1 << 64),
    "canon": (EC, P),
    "u32": (W, 1 << 32),
    "s3any": (S3, 1 << 64),
    "shift": (list(range(192)), 192),
    "flag": ([0, 1], 2),
}


def uniform(n, hi, seed):
    """n seeded uniform integers in [0, hi) as uint64"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, hi - 1, size=n, dtype=np.uint64, endpoint=True)


def operand_columns(domains, n_uniform=N_UNIFORM, seed=0):
    """the full Cartesian product of the domains' lattice values, then n_uniform seeded uniform cases; one uint64 column per operand"""
    prod = list(itertools.product(*[DOMAINS[d][0] for d in domains]))
    cols = []
    for k, d in enumerate(domains):
        lat = np.array([t[k] for t in prod], dtype=np.uint64)
        cols.append(np.concatenate([lat, uniform(n_uniform, DOMAINS[d][1], (seed, k, 0x5EED))]))
    return cols, len(prod)


# ---- references on Python integers ------------------------------------------------------------------------------------------
def inv(a):
    return pow(a, P - 2, P)


def is_square(a):  # Euler's criterion; zero counts as a square
    return a % P == 0 or pow(a, (P - 1) // 2, P) == 1


def _pow2(s):
    return pow(2, s, P)


# kind: how the device output (o0, o1) is compared with ref(a, b, c)
#   "canon" o0 == ref                    "weak"  o0 = ref (mod p) and o1 = gl_canon(o0) == ref
#   "wide"  o0 + o1 2^64 == ref          "inv"   a o0 = 1, or 0 -> 0          "sqrt"  o1 == is_square(a); o0^2 == a if square, else 0
#   "flag"  o0 == ref as 0 / 1
OPS = {
    # gl.cuh
    "gl_canon": (["any"], "canon", lambda a: a % P),
    "gl_add": (["canon", "canon"], "canon", lambda a, b: (a + b) % P),
    "gl_sub": (["canon", "canon"], "canon", lambda a, b: (a - b) % P),
    "gl_neg": (["canon"], "canon", lambda a: -a % P),
    "gl_addw": (["any", "canon"], "weak", lambda a, b: (a + b) % P),
    "gl_reduce128w": (["any", "any"], "weak", lambda lo, hi: (lo + (hi << 64)) % P),
    "gl_reduce96w": (["any", "u32"], "weak", lambda lo, hi: (lo + (hi << 64)) % P),
    "gl_reduce128": (["any", "any"], "canon", lambda lo, hi: (lo + (hi << 64)) % P),
    "gl_mul_wide": (["any", "any"], "wide", lambda a, b: a * b),
    "gl_mul_add_wide": (["any", "any", "s3any"], "wide", lambda a, b, c: a * b + c),
    "gl_mul": (["any", "any"], "canon", lambda a, b: a * b % P),
    "gl_mulw": (["any", "any"], "weak", lambda a, b: a * b % P),
    "gl_mul_addw": (["any", "any", "s3any"], "weak", lambda a, b, c: (a * b + c) % P),
    "gl_mul_add": (["any", "any", "s3any"], "canon", lambda a, b, c: (a * b + c) % P),
    "gl_mul_small": (["canon", "u32"], "canon", lambda a, c: a * c % P),
    "gl_mul_small_w": (["any", "u32"], "weak", lambda a, c: a * c % P),
    "gl_pow7": (["canon"], "canon", lambda a: pow(a, 7, P)),
    "gl_inv": (["canon"], "inv", None),
    # gl5.cuh, base-field part
    "gl_inv_chain": (["canon"], "inv", None),
    "gl_sqrt": (["canon"], "sqrt", None),
    "gl_is_square": (["canon"], "flag", lambda a: int(is_square(a))),
    # poseidon.cuh S-boxes
    "p2_sbox": (["any", "canon"], "weak", lambda x, rc: pow(x + rc, 7, P)),
    "p2_sbox0": (["any"], "weak", lambda x: pow(x, 7, P)),
    # ntt_arith.cuh
    "gl_mul_2p24": (["canon"], "canon", lambda x: x * _pow2(24) % P),
    "gl_mul_2p48": (["canon"], "canon", lambda x: x * _pow2(48) % P),
    "gl_mul_2p72": (["canon"], "canon", lambda x: x * _pow2(72) % P),
    "gl_sub_mul_2p48": (["canon", "canon"], "canon", lambda u, v: (u - v) * _pow2(48) % P),
    "gl_sub_mul_2p72": (["canon", "canon"], "canon", lambda u, v: (u - v) * _pow2(72) % P),
    "gl_mul_2pow": (["canon", "shift"], "canon", lambda x, s: x * _pow2(s) % P),
}
for _k in (1, 2, 3):
    OPS["gl_mul_w8_%d" % _k] = (["canon"], "canon", lambda x, k=_k: x * _pow2(24 * k) % P)
    OPS["gl_sub_mul_w8_%d" % _k] = (["canon", "canon"], "canon", lambda u, v, k=_k: (u - v) * _pow2(24 * k) % P)
    # forward (u - v) w_8^K, inverse (u - v) w_8^-K, w_8 = 2^24 of order 8
    OPS["bfly_lo_%d" % _k] = (["canon", "canon", "flag"], "canon",
                              lambda u, v, i, k=_k: (u - v) * _pow2(24 * (8 - k if i else k)) % P)


def scalar_cases(name, n_uniform=N_UNIFORM):
    """(columns, number of lattice cases) of one scalar operation"""
    seed = zlib.crc32(name.encode())  # from the name alone: adding an operation leaves every other table as it was
    return operand_columns(OPS[name][0], n_uniform, seed)


def check_scalar(name, cols, o0, o1):
    """indices of the cases whose output (o0, o1) breaks the operation's contract"""
    _, kind, ref = OPS[name]
    ins = [c.tolist() for c in cols]
    o0, o1 = o0.tolist(), o1.tolist()
    bad = []
    for i in range(len(o0)):
        args = [c[i] for c in ins]
        r0, r1 = o0[i], o1[i]
        if kind == "canon":
            ok = r0 == ref(*args)
        elif kind == "weak":
            want = ref(*args)
            ok = r0 % P == want and r1 == want
        elif kind == "wide":
            ok = r0 + (r1 << 64) == ref(*args)
        elif kind == "flag":
            ok = r0 == ref(*args)
        elif kind == "inv":
            a = args[0]
            ok = r0 < P and (r0 == 0 if a == 0 else a * r0 % P == 1)
        elif kind == "sqrt":
            a = args[0]
            sq = is_square(a)
            ok = r1 == int(sq) and r0 < P and (r0 * r0 % P == a if sq else r0 == 0)
        else:
            raise ValueError(kind)
        if not ok:
            bad.append(i)
    return bad


# ---- models of the device sequences: which branch does an operand pair take? ---------------------------------------------------
def model_reduce128w(lo, hi, borrow_correction=True):
    """gl_reduce128w as the device spells it: t = hl EPS + lo with carry c, t - hh with borrow b, r + (c - b) EPS. -> (c, b, r)
    borrow_correction=False: the addend c EPS alone, the mistake that test_field_cases.py shows the tables would catch"""
    hl, hh = hi & M32, hi >> 32
    t = hl * EPS + lo
    c, t = t >> 64, t & M64
    b = int(t < hh)
    r = (t - hh) & M64
    return c, b, (r + (c - (b if borrow_correction else 0)) * EPS) & M64


def model_reduce96w(lo, hi):
    t = hi * EPS + lo
    c, t = t >> 64, t & M64
    return c, (t + c * EPS) & M64


def model_mul_small(a, c):
    p0 = (a & M32) * c
    p1 = (a >> 32) * c + (p0 >> 32)
    return model_reduce96w(((p1 << 32) & M64) | (p0 & M32), p1 >> 32)


def model_add(a, b):
    """gl_add's select (c1 | d1): the carry of a + b, and the carry of s + EPS -> (c1, d1)"""
    s = a + b
    c1, s = s >> 64, s & M64
    return c1, (s + EPS) >> 64


def model_cols_w3(terms, f=1):
    """the top column word of gl_cols after add / add_scaled of the terms: value() subtracts (w3 >> 32) 2^32"""
    c = [0, 0, 0, 0]
    for a, b in terms:
        pr = a * b
        for k in range(4):
            c[k] += ((pr >> (32 * k)) & M32) * f
    assert all(x < (1 << 64) for x in c)
    w1 = c[1] + (c[0] >> 32)
    w2 = c[2] + (w1 >> 32)
    return c[3] + (w2 >> 32)


def branch_classes(n_uniform=0):
    """counts of the branch classes the operand tables reach, computed from the operands alone"""
    out = {}
    lat = lambda name: [c.tolist() for c in scalar_cases(name, n_uniform)[0]]
    lo, hi = lat("gl_reduce128w")
    cb = {}
    high = 0
    for x, y in zip(lo, hi):
        c, b, r = model_reduce128w(x, y)
        assert r % P == (x + (y << 64)) % P
        cb[(c, b)] = cb.get((c, b), 0) + 1
        high += r >= P
    out["reduce128w_cb"] = cb
    out["reduce128_high"] = high
    lo, hi = lat("gl_reduce96w")
    cc = {}
    for x, y in zip(lo, hi):
        c, r = model_reduce96w(x, y)
        assert r % P == (x + (y << 64)) % P
        cc[c] = cc.get(c, 0) + 1
    out["reduce96w_c"] = cc
    a, b = lat("gl_mul")
    out["mul_high"] = sum(model_reduce128w(x * y & M64, x * y >> 64)[2] >= P for x, y in zip(a, b))
    a, b = lat("gl_mul_small")
    out["mul_small_high"] = sum(model_mul_small(x, y)[1] >= P for x, y in zip(a, b))
    a, b = lat("gl_add")
    sel = {}
    for x, y in zip(a, b):
        k = model_add(x, y)
        sel[k] = sel.get(k, 0) + 1
    out["add_select"] = sel
    for name in ("gl_sub", "gl_sub_mul_2p48", "gl_sub_mul_2p72"):
        a, b = lat(name)
        br = {0: 0, 1: 0}
        for x, y in zip(a, b):
            br[int(x < y)] += 1
        out[name + "_borrow"] = br
    # the linear layers hand gl_reduce96w the integer M s (+ rc) split at 2^64: its top word is below 2^9
    states = elements(12, False, 12).tolist()
    out["layer_c"] = {}
    for name, m in (("p2_external", P2_EXTERNAL), ("poseidon_mds", POSEIDON_MDS)):
        cc = {0: 0, 1: 0}
        for st in states:
            for row in m:
                v = sum(w * x for w, x in zip(row, st))
                assert v >> 64 < 1 << 9
                cc[model_reduce96w(v & M64, v >> 64)[0]] += 1
        out["layer_c"][name] = cc
    out["cols_top"] = {(t, f): sum(model_cols_w3(terms, max(f, 1)) >> 32 != 0 for terms in cols_terms(t, f)) for t, f in COLS_SHAPES}
    return out


# ---- gl_cols ---------------------------------------------------------------------------------------------------------------
COLS_SHAPES = [(1, 0), (5, 0), (25, 0), (1, 2), (3, 3), (3, 6)]  # (terms, f): f = 0 add, else add_scaled by f


def mixed(n, width, lattice, hi, seed):
    """n rows of `width` limbs, each from the lattice with probability 3/4 and uniform in [0, hi) otherwise"""
    rng = np.random.default_rng(seed)
    lat = np.array(lattice, dtype=np.uint64)[rng.integers(0, len(lattice), size=(n, width))]
    uni = rng.integers(0, hi - 1, size=(n, width), dtype=np.uint64, endpoint=True)
    return np.where(rng.random((n, width)) < 0.75, lat, uni)


def cols_inputs(terms, f):
    """[n][terms] operand arrays a, b (any u64): every all-equal pair of lattice values, then 4096 mixed rows"""
    pairs = list(itertools.product(EANY, EANY))
    a = np.array([[x] * terms for x, _ in pairs], dtype=np.uint64)
    b = np.array([[y] * terms for _, y in pairs], dtype=np.uint64)
    return (np.concatenate([a, mixed(4096, terms, EANY, 1 << 64, (terms, f, 1))]),
            np.concatenate([b, mixed(4096, terms, EANY, 1 << 64, (terms, f, 2))]))


def cols_terms(terms, f):
    a, b = cols_inputs(terms, f)
    return [list(zip(x, y)) for x, y in zip(a.tolist(), b.tolist())]


def cols_ref(terms, f):
    return [sum(x * y for x, y in t) * max(f, 1) % P for t in cols_terms(terms, f)]


# ---- GF(p^2) = GF(p)[X] / (X^2 - 7), GF(p^5) = GF(p)[z] / (z^5 - 3): schoolbook convolution -------------------------------------
def ext_mul(x, y, deg, nonres):
    c = [0] * (2 * deg - 1)
    for i in range(deg):
        for j in range(deg):
            c[i + j] += x[i] * y[j]
    return [(c[i] + nonres * (c[i + deg] if i + deg < len(c) else 0)) % P for i in range(deg)]


def gl2_mul(x, y):
    return ext_mul(x, y, 2, 7)


def gl5_mul(x, y):
    return ext_mul(x, y, 5, 3)


FROB_GAMMA = pow(3, (P - 1) // 5, P)  # (z^i)^p = z^i 3^(i (p - 1) / 5)


def gl5_frob(x, e):
    return [x[i] * pow(FROB_GAMMA, i * e, P) % P for i in range(5)]


def gl5_norm(x):
    r = x
    for e in range(1, 5):
        r = gl5_mul(r, gl5_frob(x, e))
    assert r[1:] == [0, 0, 0, 0]
    return r[0]


def gl5_sgn0(x):
    for v in x:
        if v:
            return v & 1
    return 0


def elements(width, canonical, seed):
    """every all-limbs-equal element, then 4096 mixed ones -> uint64 [n][width]"""
    lat, hi = (EC, P) if canonical else (EANY, 1 << 64)
    eq = np.array([[e] * width for e in lat], dtype=np.uint64)
    return np.concatenate([eq, mixed(4096, width, lat, hi, (width, seed))])


def element_pairs(width, seed):
    """canonical pairs: every pair of all-equal elements, then 4096 mixed pairs"""
    pairs = list(itertools.product(EC, EC))
    a = np.array([[x] * width for x, _ in pairs], dtype=np.uint64)
    b = np.array([[y] * width for _, y in pairs], dtype=np.uint64)
    return (np.concatenate([a, mixed(4096, width, EC, P, (width, seed, 1))]),
            np.concatenate([b, mixed(4096, width, EC, P, (width, seed, 2))]))


# ---- Poseidon2 / Poseidon linear layers as integer matrices ---------------------------------------------------------------------
def header_table(name):
    """a constant table of csrc/perm_constants.h"""
    src = open(os.path.join(CSRC, "perm_constants.h")).read()
    m = re.search(r"uint64_t %s\[(\d+)\] = \{(.*?)\};" % name, src, re.S)
    vals = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", m.group(2))]
    assert len(vals) == int(m.group(1))
    return vals


M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]
# circ(2 M4, M4, M4)
P2_EXTERNAL = [[M4[i % 4][j % 4] * (2 if i // 4 == j // 4 else 1) for j in range(12)] for i in range(12)]
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
# row r: sum_i circ[i] s[(i + r) % 12], plus 8 s[0] in row 0
POSEIDON_MDS = [[MDS_CIRC[(j - r) % 12] + (8 if r == 0 and j == 0 else 0) for j in range(12)] for r in range(12)]


def p2_internal_matrix():
    d = header_table("POSEIDON2_DIAG_M1")
    return [[1 + (d[i] if i == j else 0) for j in range(12)] for i in range(12)]


def mat_apply(m, states, rc=None):
    """m s (+ rc) mod p for each row of `states` (lists of 12 Python integers)"""
    out = []
    for s in states:
        out.append([(sum(m[i][j] * s[j] for j in range(12)) + (rc[i] if rc else 0)) % P for i in range(12)])
    return out
