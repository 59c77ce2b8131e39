"""GF(p^5) = GF(p)[z] / (z^5 - 3), the Ecgfp5 base field, in plain Python: the eager values of the builder's quintic hints
(recursion.Builder.quintic_sqrt / quintic_quotient) and the numbers of the witness tape's GF(p^5) opcodes (include/mp2g.h enum
mp2g_witness_op_gf5). An element is a tuple of 5 canonical coefficients, coefficient i of z^i first. The library's replays run the
same operations in csrc/gl5.cuh; nothing here is on a hot path."""

P = 0xFFFFFFFF00000001
ORDER = P ** 5
TWO_ADICITY = 32            # p^5 - 1 = 2^32 * odd: (p^5 - 1) / (p - 1) = 1 + p + ... + p^4 is odd
TWO_GEN = 7277203076849721926  # a generator of GF(p)'s 2-Sylow subgroup, which is also GF(p^5)'s

# the second opcode block of the public tape format (the first block's numbers are recursion.py's OP_*)
OP_QUINTIC_SQRT, OP_QUINTIC_QUOTIENT, OP_GF5_END = 32, 33, 34

ZERO = (0, 0, 0, 0, 0)
ONE = (1, 0, 0, 0, 0)


def elem(v):
    """5 integers (any size, read mod p) -> an element"""
    v = tuple(int(x) % P for x in v)
    assert len(v) == 5
    return v


def add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def neg(a):
    return tuple(-x % P for x in a)


def mul(a, b):
    r = [0] * 5
    for i in range(5):
        for j in range(5):
            if i + j < 5:
                r[i + j] += a[i] * b[j]
            else:
                r[i + j - 5] += 3 * a[i] * b[j]  # z^5 = 3
    return tuple(x % P for x in r)


def power(a, e):
    r = ONE
    while e:
        if e & 1:
            r = mul(r, a)
        a = mul(a, a)
        e >>= 1
    return r


def inv(a):
    """inverse, or 0 for 0"""
    return power(a, ORDER - 2)


def div(a, b):
    """a / b, or 0 when b = 0 (the MP2G_OP_QUINTIC_QUOTIENT rule)"""
    return mul(a, inv(b))


def is_square(a):
    return a == ZERO or power(a, (ORDER - 1) // 2) == ONE


def sgn0(a):
    """the parity of the first non-zero coefficient (0 for 0)"""
    for x in a:
        if x:
            return x & 1
    return 0


def sqrt(a):
    """the square root r of a with sgn0(r) = 0, or None when a is not a square (the MP2G_OP_QUINTIC_SQRT rule). Tonelli-Shanks
    with the base field's 2^32-th root of unity"""
    if a == ZERO:
        return ZERO
    if not is_square(a):
        return None
    q = (ORDER - 1) >> TWO_ADICITY
    c = (TWO_GEN, 0, 0, 0, 0)
    m, t, r = TWO_ADICITY, power(a, q), power(a, (q + 1) // 2)
    while t != ONE:
        i, t2 = 0, t
        while t2 != ONE:
            t2 = mul(t2, t2)
            i += 1
        b = power(c, 1 << (m - i - 1))
        m, c = i, mul(b, b)
        t, r = mul(t, c), mul(r, b)
    assert mul(r, r) == a
    return neg(r) if sgn0(r) else r
