"""The reference's UInt256Target gadgets over a recursion.Builder: mp2-common/src/u256.rs:273-560 (CircuitBuilderU256) and :726-794
(mul_div_u256), restated gadget by gadget. A u256 target is a list of NUM_LIMBS = 8 base-field targets, u32 limbs, least
significant first (UInt256Target's order). The limb arithmetic is [dep] plonky2-u32's (add_u32s_with_carry, add_many_u32,
mul_add_u32, sub_u32: gadgets/arithmetic_u32.rs, recalled) on the builder's U32ArithmeticGate / U32AddManyGate / U32SubtractionGate
rows, whose generators are tape instructions; the division hint is the tape's MP2G_OP_U256_DIV (Builder.u256_div_hint). So a circuit
built from these gadgets has its whole witness replayed by the recorded program, on host or device.

Booleans are base-field targets that hold 0 or 1. Nothing here is used by table.py's circuits."""
from . import recursion as R
from . import wideops

NUM_LIMBS = wideops.U256_LIMBS
P = R.P


# ---- values --------------------------------------------------------------------------------------------------------------------
def value(u):
    """the integer a u256 target holds (limbs read as u32)"""
    return wideops.from_limbs(t.v for t in u)


def add_virtual_u256_unsafe(b, v):
    """u256.rs:229-231: 8 witness limbs, no range check"""
    return [b.add_virtual(x) for x in wideops.to_limbs(v, NUM_LIMBS)]


def add_virtual_u256(b, v):
    """u256.rs:233-263: 8 witness limbs, each range-checked by a U32RangeCheckGate (7 limbs a row, rows shared between calls; the
    reference packs the limbs of ONE call into rows of their own)"""
    u = add_virtual_u256_unsafe(b, v)
    for t in u:
        b.u32_range_check(t)
    return u


def constant_u256(b, v):
    return [b.constant(x) for x in wideops.to_limbs(v, NUM_LIMBS)]


def zero_u256(b):
    """u256.rs:300-303"""
    return [b.zero()] * NUM_LIMBS


def one_u256(b):
    """u256.rs:305-310"""
    return [b.one()] + [b.zero()] * (NUM_LIMBS - 1)


def register_public_input_u256(b, u):
    """u256.rs:265-271: the limbs in big-endian order"""
    b.register_public_inputs(list(reversed(u)))


# ---- [dep] plonky2-u32 gadgets/arithmetic_u32.rs ---------------------------------------------------------------------------------
def _add_many_ops(na):
    """U32AddManyGate::new_from_config: operations a row with na addends (na + 3 routed wires and 18 limbs each)"""
    return min(R.NUM_ROUTED // (na + 3), R.NUM_WIRES // (na + 3 + 18))


def mul_add_u32(b, x, y, z):
    """x y + z = low + 2^32 high"""
    return b.u32_arithmetic(x, y, z)


def add_u32(b, x, y):
    return mul_add_u32(b, x, b.one(), y)


def add_u32s_with_carry(b, to_add, carry):
    if len(to_add) == 1:
        return add_u32(b, to_add[0], carry)
    return b.u32_add_many(to_add, carry, ops=_add_many_ops(len(to_add)))


def add_many_u32(b, to_add):
    if len(to_add) == 0:
        return b.zero(), b.zero()
    if len(to_add) == 1:
        return to_add[0], b.zero()
    if len(to_add) == 2:
        return add_u32(b, to_add[0], to_add[1])
    return b.u32_add_many(to_add, b.zero(), ops=_add_many_ops(len(to_add)))


def sub_u32(b, x, y, borrow):
    return b.u32_sub(x, y, borrow)


# ---- CircuitBuilderU256 -----------------------------------------------------------------------------------------------------------
def add_u256(b, left, right):
    """u256.rs:273-298: (sum mod 2^256, carry)"""
    carry, out = b.zero(), []
    for l, r in zip(left, right):
        res, carry = add_u32s_with_carry(b, [l, r], carry)
        out.append(res)
    return out, carry


def sub_u256(b, left, right):
    """u256.rs:394-414: (difference mod 2^256, borrow)"""
    borrow, out = b.zero(), []
    for l, r in zip(left, right):
        res, borrow = sub_u32(b, l, r, borrow)
        out.append(res)
    return out, borrow


def mul_u256(b, left, right):
    """u256.rs:312-392: schoolbook product over the limbs, (product mod 2^256, overflow). The carries and non-zero limb products that
    would land above limb 7 are summed in the field (u32 values: the sum cannot wrap) and the flag is sum != 0."""
    tmp = [[] for _ in range(NUM_LIMBS)]
    zero = b.zero()
    sum_carries = zero
    for i in range(NUM_LIMBS):
        if len(tmp[i]) == 0:
            carry = zero
        elif len(tmp[i]) == 1:
            carry = tmp[i][0]
        else:
            carry, c = add_many_u32(b, tmp[i])
            if i + 1 < NUM_LIMBS:
                tmp[i + 1].append(c)
            else:
                sum_carries = b.add(sum_carries, c)
        tmp[i] = []
        for j in range(NUM_LIMBS):
            if i + j >= NUM_LIMBS:
                prod = b.mul(left[j], right[i])  # u32 operands: the product in the field is the integer product
                sum_carries = b.add(sum_carries, b.not_(b.is_equal(prod, zero)))
            else:
                res, carry = mul_add_u32(b, left[j], right[i], carry)
                tmp[i + j].append(res)
        sum_carries = b.add(sum_carries, carry)
    assert all(len(t) == 1 for t in tmp)
    return [t[0] for t in tmp], b.not_(b.is_equal(sum_carries, zero))


def enforce_equal_u256(b, left, right):
    """u256.rs:429-436"""
    for l, r in zip(left, right):
        b.connect(l, r)


def is_zero(b, u):
    """u256.rs:508-518: the limbs are u32, so their sum in the field is zero only when every limb is"""
    acc = b.zero()
    for t in u:
        acc = b.add(acc, t)
    return b.is_equal(acc, b.zero())


def is_equal_u256(b, left, right):
    """u256.rs:438-486 without its shortcuts for constant operands (which change rows, not the result): the and of the limbs'
    equalities"""
    eq = b.one()
    for l, r in zip(left, right):
        eq = b.mul(eq, b.is_equal(l, r))
    return eq


def is_less_than_u256(b, left, right):
    """u256.rs:520-524: left < right iff left - right borrows"""
    return sub_u256(b, left, right)[1]


def is_less_or_equal_than_u256(b, left, right):
    """u256.rs:498-506: not (right < left)"""
    return b.not_(is_less_than_u256(b, right, left))


def select_u256(b, cond, left, right):
    """u256.rs:525-559 without its shortcuts for constant operands: cond ? left : right, limb by limb"""
    return [b.select(cond, l, r) for l, r in zip(left, right)]


def mul_div_u256(b, this, other, is_div):
    """u256.rs:726-794. is_div true: quotient and remainder of this / other, (0, this) and is_zero = 1 for other = 0; is_div false:
    prod = this other with its overflow flag (quotient and remainder are then the hint's dummies). Returns (prod, quotient,
    remainder, mul_overflow, is_zero). is_div is a boolean TARGET here (the reference also folds a constant flag)."""
    zero = b.zero()
    other_is_zero = is_zero(b, other)
    qh, rh = b.u256_div_hint(this, other, is_div)
    # add_virtual_u256: the hinted limbs are range-checked
    for t in qh + rh:
        b.u32_range_check(t)
    # remainder < other unless other = 0 or is_div is false: antecedent = is_div (1 - is_zero), and antecedent (1 - less) = 0
    antecedent = b.arithmetic(P - 1, is_div, other_is_zero, 1, is_div)
    less = is_less_than_u256(b, rh, other)
    b.connect(b.arithmetic(P - 1, antecedent, less, 1, antecedent), zero)
    # quotient other + remainder = this (is_div false: this other + remainder = this, which the hint's remainder satisfies mod 2^256)
    prod, mul_overflow = mul_u256(b, select_u256(b, is_div, qh, this), other)
    computed, carry = add_u256(b, prod, rh)
    enforce_equal_u256(b, this, computed)
    # no overflow when dividing
    b.connect(b.mul(is_div, mul_overflow), zero)
    b.connect(b.mul(is_div, carry), zero)
    return prod, qh, rh, mul_overflow, other_is_zero


def div_u256(b, left, right):
    """u256.rs:416-427: (quotient, remainder, is_zero)"""
    _, q, r, _, z = mul_div_u256(b, left, right, b.one())
    return q, r, z
