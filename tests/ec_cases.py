"""Structured inputs for the Ecgfp5 group kernels (csrc/ec_curve.cuh, csrc/ecgfp5.hip) and an exact reference for them on Python
integers. No GPU is used here: tests/test_ec_cases.py checks the cases on the references alone, tests/test_gpu_ecgfp5_edges.py
feeds the same arrays to the device.

The reference below shares no code with the oracle's C field (oracle/ecgfp5.c) or with the library's gf5.py: GF(p^5) =
GF(p)[z] / (z^5 - 3) by schoolbook products, inverse and Legendre symbol through the norm to GF(p), the square root by
Tonelli-Shanks in GF(p^5) itself, the group by the affine chord/tangent law on y^2 = x (x^2 + 2 x + 263 z) with the group
addition (P + Q) + N, N = (0, 0), and simple_swu restated from mp2-common/src/group_hashing/sswu_value.rs:31-77 with its constants
derived from the curve's own a and b. It is slow (a square root takes milliseconds), so it serves the small structured cases;
everything larger is checked against the oracle.

The case builders are seeded and cached: every caller gets the same arrays and must leave them unchanged."""
import functools

import numpy as np

import edge_inputs as E
import oracle as O

P = O.P
ORDER = P ** 5
ZERO, ONE = (0, 0, 0, 0, 0), (1, 0, 0, 0, 0)
U64_MAX = (1 << 64) - 1


# ---- GF(p^5) on Python integers ----------------------------------------------------------------------------------------------
def el(v):
    return tuple(int(x) % P for x in v)


def add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def neg(a):
    return tuple(-x % P for x in a)


def scale(a, k):
    return tuple(x * k % P for x in a)


def mul(a, b):
    c = [0] * 9
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                c[i + j] += x * y
    return tuple((c[i] + 3 * (c[i + 5] if i < 4 else 0)) % P for i in range(5))  # z^5 = 3


def sqr(a):
    return mul(a, a)


def power(a, e):
    r = ONE
    while e:
        if e & 1:
            r = mul(r, a)
        a = sqr(a)
        e >>= 1
    return r


_FROB = [pow(3, i * (P - 1) // 5, P) for i in range(5)]  # (z^i)^p = z^i 3^(i (p - 1) / 5)


def frob(a):
    return tuple(x * g % P for x, g in zip(a, _FROB))


def _conjugates(a):
    """a^(p + p^2 + p^3 + p^4): times a it is the norm, an element of GF(p)"""
    f, q = frob(a), ONE
    for _ in range(4):
        q = mul(q, f)
        f = frob(f)
    return q


def norm(a):
    n = mul(a, _conjugates(a))
    assert n[1:] == (0, 0, 0, 0)
    return n[0]


def inv(a):
    """the inverse, or 0 for 0"""
    q = _conjugates(a)
    return scale(q, pow(mul(a, q)[0], P - 2, P))


def is_square(a):
    """zero counts as a square. (p^5 - 1) / (p - 1) is odd, so a is a square exactly when its norm is one in GF(p)"""
    n = norm(a)
    return n == 0 or pow(n, (P - 1) // 2, P) == 1


def sgn0(a):
    """the parity of the first non-zero coefficient, 0 for 0"""
    for x in a:
        if x:
            return x & 1
    return 0


_TWO_ADICITY = 32  # p^5 - 1 = 2^32 * odd
_ODD = (ORDER - 1) >> _TWO_ADICITY
_TWO_GEN = (pow(7, (P - 1) >> 32, P), 0, 0, 0, 0)  # 7 generates GF(p)*: an element of order 2^32, of GF(p^5)'s 2-Sylow group too
assert pow(_TWO_GEN[0], 1 << 31, P) == P - 1


def sqrt(a):
    """the square root r of a with sgn0(r) = 0, or None when a is no square"""
    if a == ZERO:
        return ZERO
    if not is_square(a):
        return None
    r = power(a, (_ODD + 1) // 2)
    t = mul(sqr(r), inv(a))  # a^odd
    m, c = _TWO_ADICITY, _TWO_GEN
    while t != ONE:
        i, t2 = 0, t
        while t2 != ONE:
            t2, i = sqr(t2), i + 1
        b = c
        for _ in range(m - i - 1):
            b = sqr(b)
        m, c = i, sqr(b)
        t, r = mul(t, c), mul(r, b)
    assert sqr(r) == a
    return neg(r) if sgn0(r) else r


# ---- the curve y^2 = x (x^2 + A x + B) and the group E[r] + N -----------------------------------------------------------------
A = (2, 0, 0, 0, 0)
B = (0, 263, 0, 0, 0)
N = (ZERO, ZERO)  # the neutral element; None stands for the curve's point at infinity, which is no group element
_HALF = (P + 1) // 2
_THIRD = pow(3, P - 2, P)
TWO_THIRDS = (2 * _THIRD % P, 0, 0, 0, 0)


def on_curve(pt):
    x, y = pt
    return sqr(y) == mul(x, add(add(sqr(x), mul(A, x)), B))


def curve_add(p, q):
    """chord and tangent on the curve itself"""
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if y1 != y2 or y1 == ZERO:
            return None
        lam = mul(add(add(scale(sqr(x1), 3), scale(mul(A, x1), 2)), B), inv(scale(y1, 2)))
    else:
        lam = mul(sub(y2, y1), inv(sub(x2, x1)))
    x3 = sub(sub(sub(sqr(lam), A), x1), x2)
    return x3, sub(mul(lam, sub(x1, x3)), y1)


def group_add(p, q):
    return curve_add(curve_add(p, q), N)


def encode(p):
    return mul(p[1], inv(p[0]))  # N -> 0


@functools.lru_cache(maxsize=None)
def decode(w):
    """the point of encoding w (5 canonical integers), or None for an invalid encoding: x is the non-square root of
    x^2 - (w^2 - A) x + B"""
    e = sub(sqr(w), A)
    r = sqrt(sub(sqr(e), scale(B, 4)))
    if r is None:
        return N if w == ZERO else None
    x1, x2 = scale(add(e, r), _HALF), scale(sub(e, r), _HALF)
    x = x2 if is_square(x1) else x1
    return x, mul(w, x)


def to_weierstrass(p):
    """[x0..x4, y0..y4, is_inf] of (x + A / 3, -y); the neutral element is the point at infinity there"""
    x, y = p
    if x == ZERO:
        return [0] * 10 + [1]
    return list(add(x, TWO_THIRDS)) + list(neg(y)) + [0]


def scalar_mul(p, k):
    """k p by double-and-add, most significant bit first"""
    acc = N
    for i in reversed(range(max(1, int(k).bit_length()))):
        acc = group_add(acc, acc)
        if (k >> i) & 1:
            acc = group_add(acc, p)
    return acc


def exact_sum(encodings):
    """(encoding, Weierstrass limbs) of the sum of the encoded points, or None when one of them is invalid"""
    acc = N
    for w in encodings:
        p = decode(el(w))
        if p is None:
            return None
        acc = group_add(acc, p)
    return list(encode(acc)), to_weierstrass(acc)


def exact_scalar_mul(w, k):
    p = scalar_mul(decode(el(w)), k)
    return list(encode(p)), to_weierstrass(p)


# ---- simple_swu ---------------------------------------------------------------------------------------------------------------
# the short Weierstrass model Y^2 = X^3 + A_SW X + B_SW of the curve, X = x + A / 3
A_SW = sub(B, scale(sqr(A), _THIRD))
B_SW = scale(mul(A, sub(scale(sqr(A), 2), scale(B, 9))), pow(27, P - 2, P))
Z_SW = (P - 4, P - 1, 0, 0, 0)  # the map's non-square constant, -4 - z
NEG_Z_INV = neg(inv(Z_SW))
NEG_B_DIV_A = neg(mul(B_SW, inv(A_SW)))


def g_sw(x):
    return add(add(mul(x, sqr(x)), mul(A_SW, x)), B_SW)


def simple_swu_trace(u):
    """(point, branch facts) of the simplified SWU map of u. With t = Z u^2: x1 = -B/A (1 + 1 / (t^2 + t)), or -B/A (-1/Z) when
    that denominator is zero; x2 = t x1. The first of g(x1), g(x2) that is a square gives X and a root Y whose sgn0 is made u's.
    The result is the group element of encoding Y / (X - 2/3)."""
    t = mul(Z_SW, sqr(u))
    tv1 = inv(add(sqr(t), t))
    x1 = mul(NEG_Z_INV if tv1 == ZERO else add(tv1, ONE), NEG_B_DIV_A)
    y_pos = sqrt(g_sw(x1))
    first = y_pos is not None
    x_sw = x1
    if not first:
        x_sw = mul(t, x1)
        y_pos = sqrt(g_sw(x_sw))
    x_cand = sub(x_sw, TWO_THIRDS)
    flip = sgn0(u) != sgn0(y_pos)
    y_cand = neg(y_pos) if flip else y_pos
    w = mul(y_cand, inv(x_cand))
    facts = {"gx1_square": first, "x_cand_square": is_square(x_cand), "flip": flip, "degenerate": w == ZERO or x_cand == ZERO}
    return decode(w), facts


# ---- the oracle, as arrays ------------------------------------------------------------------------------------------------------
def orc_map(ins, variant=0):
    ins = O.arr(ins)
    w = np.zeros((ins.shape[0], 5), dtype=np.uint64)
    wei = np.zeros((ins.shape[0], 11), dtype=np.uint64)
    O.lib().orc_map_to_curve_batch(variant, O.p(ins), O.sz(ins.shape[1]), O.sz(ins.shape[0]), O.p(w), O.p(wei))
    return w, wei


def orc_sum(pts):
    """(encoding, Weierstrass limbs) of the oracle's sum, or None when it refuses an encoding"""
    pts = O.arr(pts).reshape(-1, 5)
    w, wei = np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    if not O.lib().orc_curve_sum(O.p(pts), O.sz(pts.shape[0]), O.p(w), O.p(wei)):
        return None
    return w, wei


def orc_mul(w_in, k):
    w_in = O.arr(w_in)
    kl = O.arr([(int(k) >> (32 * j)) & 0xFFFFFFFF for j in range(4)], np.uint32)
    w, wei = np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    assert O.lib().orc_scalar_mul(O.p(w_in), O.p(kl), 4, O.p(w), O.p(wei))
    return w, wei


def orc_swu(u):
    u = O.arr(u).reshape(-1, 5)
    w = np.zeros((u.shape[0], 5), dtype=np.uint64)
    wei = np.zeros((u.shape[0], 11), dtype=np.uint64)
    for i in range(u.shape[0]):
        O.lib().orc_swu(O.p(np.ascontiguousarray(u[i])), O.p(w[i]), O.p(wei[i]))
    return w, wei


def orc_valid(w):
    return bool(O.lib().orc_decode_check(O.p(O.arr(w))))


NEUTRAL_W = np.zeros(5, dtype=np.uint64)
NEUTRAL_WEI = np.array([0] * 10 + [1], dtype=np.uint64)


# ---- case builders ----------------------------------------------------------------------------------------------------------
def negate(w):
    """the encoding of -P"""
    w = O.arr(w)
    return (np.uint64(P) - w) % np.uint64(P)


def base_points(k):
    """k valid encodings of points nobody knows a relation between: the oracle's map_to_curve of seeded inputs. base_points(j) is
    a prefix of base_points(k) for j < k"""
    assert k <= 512
    return _base()[:k]


@functools.lru_cache(maxsize=None)
def _base():
    b = orc_map(O.rand_field((512, 9), 0xEC0001))[0]
    b.setflags(write=False)  # shared by every case: a caller that plants something copies first
    return b


# the labels alone, for test ids: collecting the tests builds no case
SUM_LABELS = (["P,P", "P,P,P", "128xP", "129xP"]
              + ["P,-P at lanes %d,%d, %s others" % (s - 1, 2 * s - 1, fill) for s in (1, 2, 4, 8, 16, 32, 64) for fill in ("random", "neutral")]
              + ["P,-P,Q", "P,Q,-P,-Q", "P,-P,Q,-Q", "256: block 0 cancels, block 1 random", "130: inverse pairs only"]
              + ["129: encoding 0 at the %s index" % n for n in ("first", "middle", "last")])


@functools.lru_cache(maxsize=None)
def sum_cases():
    """[(label, encodings [count][5])] for curve_sum. One block of sum_kernel holds point i in lane i (count <= 128) and adds lane
    t + s into lane t < s at the tree level s = 64, 32 .. 1; 129 points and more go through block partials and a second pass."""
    b = base_points(400)
    p, q = b[0], b[1]
    z = np.zeros(5, dtype=np.uint64)
    cases = [("P,P", np.stack([p, p])), ("P,P,P", np.stack([p, p, p])), ("128xP", np.tile(p, (128, 1))), ("129xP", np.tile(p, (129, 1)))]
    for s in (1, 2, 4, 8, 16, 32, 64):
        t = s - 1  # t < s: with neutral points around them the two meet as the operands of one addition, at level s
        for fill in ("random", "neutral"):
            pts = b[2:130].copy() if fill == "random" else np.zeros((128, 5), dtype=np.uint64)
            pts[t], pts[t + s] = p, negate(p)
            cases.append(("P,-P at lanes %d,%d, %s others" % (t, t + s, fill), pts))
    cases.append(("P,-P,Q", np.stack([p, negate(p), q])))
    cases.append(("P,Q,-P,-Q", np.stack([p, q, negate(p), negate(q)])))  # both pairs cancel at level 2: two cancellation-made neutrals meet
    cases.append(("P,-P,Q,-Q", np.stack([p, negate(p), q, negate(q)])))  # P + Q and -P - Q meet at level 1
    # the first block is 64 inverse pairs in lanes (i, i + 64): all cancel at level 64, the block's partial is a neutral made by
    # cancellation, and the second pass adds it to the second block's partial
    first = np.concatenate([b[130:194], negate(b[130:194])])
    cases.append(("256: block 0 cancels, block 1 random", np.concatenate([first, b[194:322]])))
    pairs = np.empty((130, 5), dtype=np.uint64)
    pairs[0::2], pairs[1::2] = b[322:387], negate(b[322:387])
    cases.append(("130: inverse pairs only", pairs))
    for name, i in (("first", 0), ("middle", 64), ("last", 128)):
        pts = b[2:131].copy()
        pts[i] = z
        cases.append(("129: encoding 0 at the %s index" % name, pts))
    assert [label for label, _ in cases] == SUM_LABELS
    return cases


BIG_COUNTS = [16384, 16385, 131072, 131073, 140001]
BIG_LANE_STRIDE = 131072  # sum_kernel's grid is capped at 1024 blocks of 128 lanes: point i + 131072 is lane i's second trip
BIG_PLANT = 777


BIG_LABELS = ["%d" % c for c in BIG_COUNTS] + ["%d, P,-P in one lane's two trips" % BIG_COUNTS[-1]]


def big_sum_case(k):
    """(encodings [count][5], terms) of case BIG_LABELS[k]; terms = [(encoding, multiplicity)] has the same sum as the encodings.
    Each array tiles 64 base points. The last case plants P, -P at indices i and i + 131072: one lane's first and second trip."""
    b = base_points(400)
    count = BIG_COUNTS[min(k, len(BIG_COUNTS) - 1)]
    idx = np.arange(count) % 64
    pts = b[idx]
    if k < len(BIG_COUNTS):
        return pts, [(b[i], int((idx == i).sum())) for i in range(64)]
    p = b[399]
    pts[BIG_PLANT], pts[BIG_PLANT + BIG_LANE_STRIDE] = p, negate(p)
    mult = np.bincount(np.delete(idx, [BIG_PLANT, BIG_PLANT + BIG_LANE_STRIDE]), minlength=64)
    return pts, [(b[i], int(mult[i])) for i in range(64)] + [(p, 1), (negate(p), 1)]


def big_sum_cases():
    """(label, encodings, terms), one at a time"""
    for k, label in enumerate(BIG_LABELS):
        yield (label,) + big_sum_case(k)


def big_sum_expected(terms):
    """the oracle's sum of multiplicity * point over the terms: 64 scalar multiplications instead of 10^5 additions"""
    assert all(0 <= m < 1 << 128 for _, m in terms)
    return orc_sum(np.stack([orc_mul(w, m)[0] for w, m in terms]))


RANGE_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129]
# (start, end): sum_ranges_kernel gives range [lo, hi) one 64-lane block; point lo + t + 64 j is lane t's trip j, the tree adds lane
# t + s into lane t < s while lo + t + s < hi
RANGES = [
    (0, 0), (57, 57), (200, 200),                      # empty: at the start, inside, at the end of the array
    (10, 11), (20, 21), (21, 22), (199, 200),          # one point: P of the equal neighbours, either half of an inverse pair, the last
    (10, 12), (100, 102),                              # only P, P
    (20, 22), (150, 152),                              # only P, -P
    (21, 23), (19, 21),                                # two points that cut an inverse pair
    (20, 83), (22, 85),                                # 63: starts on the pair (20, 21); ends between 84 and 85, on P alone
    (22, 86), (20, 84),                                # 64: ends on the pair (84, 85); starts on a pair
    (21, 86), (30, 95), (19, 84),                      # 65: cuts (20, 21) and ends on a pair; P (30) and -P (94) are lane 0's two trips; straddles (20, 21)
    (20, 147), (24, 151),                              # 127: starts on a pair, P (30) and -P (94) share lane 10; ends between 150 and 151
    (23, 151), (24, 152), (10, 138),                   # 128: cuts (150, 151); ends on it; starts on P, P
    (23, 152), (10, 139), (0, 129), (71, 200),         # 129
    (40, 73),                                          # P (40) and -P (72) are lanes 0 and 32: the tree's first addition
    (0, 200),
]


@functools.lru_cache(maxsize=None)
def range_cases():
    """(encodings [200][5], ranges [n][2]) for curve_sum_ranges: equal neighbours at (10, 11) and (100, 101), adjacent inverse
    pairs at (20, 21), (84, 85) and (150, 151), an inverse pair 64 apart at (30, 94) and one 32 apart at (40, 72)"""
    pts = base_points(400)[200:400].copy()
    for i in (10, 100):
        pts[i + 1] = pts[i]
    for i, j in ((20, 21), (84, 85), (150, 151), (30, 94), (40, 72)):
        pts[j] = negate(pts[i])
    assert set(RANGE_LENGTHS) <= {hi - lo for lo, hi in RANGES}
    return pts, np.array(RANGES, dtype=np.uint32)


SCALAR_CARRIES = [9 << 28, 9 << 60, 9 << 92, 9 << 124]  # 9 = 16 - 7 recodes with a carry into the next window: across each u32 limb of k
SCALAR_COUNTS = [127, 128, 129]
SCALAR_EXACT = [0, 1, 2, 33, 34 + 17, 68 + 1, 72, 73]  # rows also checked on Python integers: 0, 1, 2, 33 on P; 17 on -P; 9 << 60; 2^128 - 1; the neutral base


@functools.lru_cache(maxsize=None)
def scalar_cases():
    """(encodings [129][5], scalars [129]) for scalar_mul_batch; the batches of SCALAR_COUNTS are its prefixes, so that the last
    block is almost full, full, and one lane. Rows 0..33: k = 0..33 on P; 34..67: the same on -P; 68..71: SCALAR_CARRIES; 72:
    2^128 - 1; 73..76: the neutral base with k = 1, 8, 9 << 60, 2^128 - 1; then seeded points and scalars."""
    b = base_points(400)
    p = b[0]
    pts = [p] * 34 + [negate(p)] * 34 + [p] * 5 + [np.zeros(5, dtype=np.uint64)] * 4
    ks = list(range(34)) * 2 + SCALAR_CARRIES + [(1 << 128) - 1] + [1, 8, 9 << 60, (1 << 128) - 1]
    rng = np.random.default_rng(0xEC0002)
    rest = max(SCALAR_COUNTS) - len(pts)
    pts += list(b[2:2 + rest])
    ks += [int.from_bytes(rng.bytes(16), "little") for _ in range(rest)]
    return np.stack(pts), ks


@functools.lru_cache(maxsize=None)
def scalar_expected():
    pts, ks = scalar_cases()
    out = [orc_mul(w, k) for w, k in zip(pts, ks)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


SWU_SEED = 0xEC0003


@functools.lru_cache(maxsize=None)
def swu_inputs():
    """u [278][5], canonical: the sgn0 ladder (each limb alone at 1, 2, p - 1, p - 2 with the others zero: leading zero limbs, an
    odd or even first non-zero limb), all limbs p - 1, u = 0, 192 rows of edge-lattice limbs and 64 uniform rows"""
    rows = []
    for limb in range(5):
        for v in (1, 2, P - 1, P - 2):
            assert v in E.F.EC
            rows.append([v if i == limb else 0 for i in range(5)])
    rows.append([P - 1] * 5)
    rows.append([0] * 5)
    return np.concatenate([np.array(rows, dtype=np.uint64), E.edge_rows((192, 5), SWU_SEED), O.rand_field((64, 5), SWU_SEED + 1)])


@functools.lru_cache(maxsize=None)
def bad_encodings(n):
    """n canonical encodings that the oracle's decode refuses, from seeded uniform draws (about half of all draws are refused)"""
    draws = O.rand_field((4 * n + 16, 5), 0xEC0004)
    bad = [w for w in draws if not orc_valid(w)][:n]
    assert len(bad) == n
    return np.stack(bad)


@functools.lru_cache(maxsize=None)
def noncanonical():
    """a valid encoding with one limb replaced, limb by limb, by p, p + 5 and 2^64 - 1; and (p, 0, 0, 0, 0)"""
    v = base_points(400)[2]
    rows = []
    for limb in range(5):
        for x in (P, P + 5, U64_MAX):
            r = v.copy()
            r[limb] = x
            rows.append(r)
    rows.append(np.array([P, 0, 0, 0, 0], dtype=np.uint64))  # zero mod p: not the neutral point
    return np.stack(rows)


def __getattr__(name):  # NONCANONICAL needs the oracle for its valid encoding: built on first use, not on import
    if name == "NONCANONICAL":
        return noncanonical()
    raise AttributeError(name)


def refusal_batch():
    """300 valid encodings (a fresh copy: the refusal tests overwrite one row)"""
    return base_points(400)[:300].copy()


REFUSAL_INDICES = [0, 127, 128, 299]
