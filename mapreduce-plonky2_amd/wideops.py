"""The wide opcode block of the witness tape in plain Python (include/mp2g.h enum mp2g_witness_op_wide): its numbers, and the
eager values of the builder methods that record them -- recursion.Builder.u32_interleave / uninterleave_to_b32 / uninterleave_to_u32
(the bit-interleaving gates of [dep] plonky2_crypto), u256_div_hint (UInt256DivGenerator, mp2-common/src/u256.rs:920-952),
biguint_div_rem_hint ([dep] plonky2_ecdsa BigUintDivRemGenerator) and poseidon_mds_row. The library's replays run the same
operations in csrc/witness_wide.h; nothing here is on a hot path. A multi-limb integer is a list of u32 limbs, least significant
first."""

# the fourth opcode block of the public tape format (the first block's numbers are recursion.py's OP_*, then gf5.py's and lut.py's)
(OP_U32_INTERLEAVE, OP_UNINTERLEAVE_TO_B32, OP_UNINTERLEAVE_TO_U32, OP_U256_DIV, OP_BIGUINT_DIV_REM, OP_POSEIDON_MDS,
 OP_WIDE_END) = range(48, 55)
U256_LIMBS = 8
BIGUINT_MAX_LIMBS = 32  # MP2G_OP_BIGUINT_DIV_REM: limbs of either operand
MASK32 = 0xFFFFFFFF


def interleave(x):
    """U32InterleaveGenerator: bit k of the low 32 bits of x -> bit 2k"""
    x = int(x) & MASK32
    return sum(((x >> k) & 1) << (2 * k) for k in range(32))


def uninterleave_b32(x):
    """UninterleaveToB32Generator: (evens, odds) of a 64-bit value, each still spread -- bit 2b (2b + 1) of x at bit 2b"""
    x = int(x)
    return x & 0x5555555555555555, (x >> 1) & 0x5555555555555555


def uninterleave_u32(x):
    """UninterleaveToU32Generator: (evens, odds) of a 64-bit value as u32 words -- bit 2b (2b + 1) of x at bit b"""
    x = int(x)
    return sum(((x >> (2 * b)) & 1) << b for b in range(32)), sum(((x >> (2 * b + 1)) & 1) << b for b in range(32))


def to_limbs(v, n):
    """the n u32 limbs of v, least significant first (v < 2^(32 n))"""
    v = int(v)
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * k)) & MASK32 for k in range(n)]


def from_limbs(limbs):
    """limbs read as the executors read them: the low 32 bits of each"""
    return sum((int(x) & MASK32) << (32 * k) for k, x in enumerate(limbs))


def u256_div(dividend, divisor, is_div):
    """UInt256DivGenerator::run_once on integers below 2^256: (quotient, remainder)"""
    if is_div:
        return (0, dividend) if divisor == 0 else divmod(dividend, divisor)
    return 1, (dividend - dividend * divisor) % (1 << 256)


def biguint_div_rem(a, b, nb):
    """BigUintDivRemGenerator: divmod(a, b); b = 0 gives (0, a cut to nb limbs) -- this library's choice, [dep] plonky2_ecdsa's
    generator panics on a zero divisor"""
    return (0, a % (1 << (32 * nb))) if b == 0 else divmod(a, b)
