"""The witness tape's wide opcode block (include/mp2g.h enum mp2g_witness_op_wide: the bit-interleaving gates, the u256 and
multi-limb division hints, PoseidonMds) on the CPU: numbers and shapes held against the header and csrc/witness_ops.h, validation by
mp2g_witness_program_create, the library's host replay against the builder's eager values and the ORACLE's gate evaluators and
prover, the u256 gadgets (u256.py) against Python integers, the in-circuit evaluators of the interleave gates through a wrap, a
self-made golden tape and a fuzz. The device replay of the same circuits is tests/test_gpu_witness_tape_wide.py."""
import ctypes
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import circuits as C
import hosttest
import oracle as O
from test_recursion import verifier_data

R = importlib.import_module("mapreduce-plonky2_amd.recursion")
U = importlib.import_module("mapreduce-plonky2_amd.u256")
W = importlib.import_module("mapreduce-plonky2_amd.wideops")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "witness_tape_wide_vectors.json")
P = O.P
# the header's numbers, written out: a renumbering must fail here
INTERLEAVE, TO_B32, TO_U32, U256_DIV, BIGUINT_DIV_REM, POSEIDON_MDS, WIDE_END = 48, 49, 50, 51, 52, 53, 54
WIDE = {INTERLEAVE, TO_B32, TO_U32, U256_DIV, BIGUINT_DIV_REM, POSEIDON_MDS}
M32, M256 = (1 << 32) - 1, (1 << 256) - 1
EDGE_WORDS = [0, M32, 0x55555555, 0xAAAAAAAA]
EDGE_U256 = [0, 1, M256, 1 << 128, M32 << 96]  # the last: 2^32 - 1 in a single limb


# ---- circuits ---------------------------------------------------------------------------------------------------------------------------
def biguint_mul_add_check(b, d, bb, r, a):
    """d bb + r = a over u32 limb lists (least significant first) and r < bb, by U32Arithmetic and U32Subtraction rows: what a gadget
    that takes the BigUintDivRem hint constrains. Per limb pair two operations, so that no intermediate reaches 2^64."""
    zero, one = b.zero(), b.one()
    acc = list(r) + [zero] * (len(d) + len(bb) - len(r))
    for i, di in enumerate(d):
        carry = zero
        for j, bj in enumerate(bb):
            lo, hi = b.u32_arithmetic(di, bj, acc[i + j])
            acc[i + j], c2 = b.u32_arithmetic(lo, one, carry)
            carry = b.add(hi, c2)  # hi 2^32 + lo + carry < 2^64: the sum of the two high parts is a u32
        acc[i + len(bb)] = carry
    for k, t in enumerate(acc):
        b.connect(t, a[k] if k < len(a) else zero)
    borrow = zero
    for x, y in zip(r, bb):
        _, borrow = b.u32_sub(x, y, borrow)
    b.connect(borrow, one)


def wide_inputs(seed, words=None, dividend=None, divisor=None, big_a=None, big_b=None):
    """the inputs of wide_circuit: 9 u32 words, two u256, a 20-limb and a 10-limb integer, a 32-limb pair, 12 extension elements"""
    rng = np.random.default_rng(seed)
    big = lambda bits: int.from_bytes(rng.bytes(bits // 8), "little")
    return {"words": list(words) if words is not None else [int(x) for x in rng.integers(0, 1 << 32, size=9)],
            "dividend": big(256) if dividend is None else dividend, "divisor": big(136) if divisor is None else divisor,
            "big_a": big(640) if big_a is None else big_a, "big_b": (big(320) | 1 << 300) if big_b is None else big_b,
            "wide_a": big(1024), "wide_b": big(1000), "mds": [int(x) for x in O.rand_field(24, seed)]}


def wide_input_vector(v):
    """the input words of wide_circuit in its add_virtual order"""
    return (list(v["words"]) + W.to_limbs(v["dividend"], 8) + W.to_limbs(v["divisor"], 8) + W.to_limbs(v["big_a"], 20) + W.to_limbs(v["big_b"], 10)
            + W.to_limbs(v["wide_a"], 32) + W.to_limbs(v["wide_b"], 32) + list(v["mds"]))


def wide_circuit(v, independent=6, strict=True, builder=None):
    """every builder method of the wide block. A chain of 8 dependent xors over the 9 words; `independent` interleaves of the words
    on one dependency level and 3 independent xor / and pairs; div_u256; a 20-by-10-limb BigUintDivRem hint checked by u32 rows; a
    32-by-32-limb one (the largest), its results public; an uninterleave_to_b32; a PoseidonMds row."""
    b = builder or R.Builder(strict)
    x = [b.add_virtual(w) for w in v["words"]]
    dividend, divisor = U.add_virtual_u256(b, v["dividend"]), U.add_virtual_u256(b, v["divisor"])
    big_a = [b.add_virtual(w) for w in W.to_limbs(v["big_a"], 20)]
    big_b = [b.add_virtual(w) for w in W.to_limbs(v["big_b"], 10)]
    wide_a = [b.add_virtual(w) for w in W.to_limbs(v["wide_a"], 32)]
    wide_b = [b.add_virtual(w) for w in W.to_limbs(v["wide_b"], 32)]
    mds = [R.E(b.add_virtual(v["mds"][2 * i]), b.add_virtual(v["mds"][2 * i + 1])) for i in range(12)]
    chain = x[0]
    for t in x[1:]:
        chain = b.xor_u32(chain, t)
    level = [b.u32_interleave(x[k % 9]) for k in range(independent)]
    pairs = [b.xor_and_u32(x[k], x[k + 1]) for k in range(3)]
    and01 = b.and_u32(x[0], x[1])
    spread = b.uninterleave_to_b32(b.add(level[0], level[1]))
    q, r, is_zero = U.div_u256(b, dividend, divisor)
    d, rem = b.biguint_div_rem_hint(big_a, big_b)
    for t in d + rem:
        b.u32_range_check(t)
    biguint_mul_add_check(b, d, big_b, rem, big_a)
    wd, wr = b.biguint_div_rem_hint(wide_a, wide_b)
    out = b.poseidon_mds_row(mds)
    less = U.is_less_than_u256(b, dividend, divisor)
    b.register_public_inputs([chain, and01, less, is_zero] + [t for p in pairs for t in p] + list(spread) + q + r + d + rem + wd + wr
                             + [t for e in out for t in (e.a, e.b)] + [level[-1]])
    return b.build()


def expected_public_inputs(v, independent=6):
    """wide_circuit's public inputs by Python integers"""
    w = v["words"]
    chain = 0
    for t in w:
        chain ^= t
    s = W.interleave(w[0]) + W.interleave(w[1 % 9])
    q, r = (0, v["dividend"]) if v["divisor"] == 0 else divmod(v["dividend"], v["divisor"])
    d, rem = divmod(v["big_a"], v["big_b"])
    wd, wr = divmod(v["wide_a"], v["wide_b"])
    mds = [C.poseidon_mds([v["mds"][2 * i + c] for i in range(12)]) for c in range(2)]
    return ([chain, w[0] & w[1], int(v["dividend"] < v["divisor"]), int(v["divisor"] == 0)] + [f(w[k], w[k + 1]) for k in range(3) for f in (int.__xor__, int.__and__)]
            + [s & 0x5555555555555555, (s >> 1) & 0x5555555555555555] + W.to_limbs(q, 8) + W.to_limbs(r, 8) + W.to_limbs(d, 20) + W.to_limbs(rem, 10)
            + W.to_limbs(wd, 32) + W.to_limbs(wr, 32) + [mds[c][i] for i in range(12) for c in range(2)] + [W.interleave(w[(independent - 1) % 9])])


def interleave_base_circuit(words, strict=True, flip=None):
    """a base circuit with interleave rows for the wrap: xor and and of two word pairs and an uninterleave_to_b32. flip = (row kind,
    wire): that bit wire of the first row of the kind is inverted after the build (a witness the circuit does not accept)."""
    b = R.Builder(strict)
    x = [b.add_virtual(w) for w in words]
    x01, a01 = b.xor_and_u32(x[0], x[1])
    x23 = b.xor_u32(x[2], x[3])
    ev, od = b.uninterleave_to_b32(b.add(b.u32_interleave(x01), b.u32_interleave(x23)))
    b.register_public_inputs([x01, a01, x23, ev, od])
    ck = b.build()
    if flip is not None:
        row = next(r for r, i in enumerate(ck.instances) if ck.gates[i].kind == flip[0])
        ck.wires[flip[1], row] ^= np.uint64(1)
    return ck


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def create(tape, n_slots=160, log_n=3, n_inputs=4):
    """mp2g_witness_program_create; None when accepted (the program is freed), else the error"""
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    h = ctypes.c_void_p()
    t = np.ascontiguousarray(tape, dtype=np.uint64)
    ins = np.arange(n_inputs, dtype=np.uint32)
    rc = mp2.load().mp2g_witness_program_create(t.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(t.size), n_slots, log_n,
                                                ins.ctypes.data_as(ctypes.c_void_p), n_inputs, None, 0, ctypes.byref(h))
    if rc == 0:
        mp2.load().mp2g_witness_program_free(h)
        return None
    return mp2.load().mp2g_last_error()


class golden_program:
    """the fields of a golden tape in the shape mp2.WitnessProgram takes"""

    def __init__(self, g):
        self.tape = np.array(g["tape"], dtype=np.uint64)
        self.input_sids = np.array(g["input_sids"], dtype=np.uint32)
        self.const_slots = np.array(g["const_slots"], dtype=np.uint64).reshape(-1, 2)
        self.n_slots, self.log_n = g["n_slots"], g["log_n"]
        self.pi_hash_sids = np.array(g["probe"][:4], dtype=np.uint32)
        self.public_input_sids = np.array(g["probe"][4:], dtype=np.uint32)


def golden_wires(case, log_n):
    w = np.zeros((135, 1 << log_n), dtype=np.uint64)
    for col, row, val in case["wires"]:
        w[col, row] = val
    return w


@pytest.fixture(scope="module")
def shape_test(tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("witness_shape_wide"), "witness_shape_test")


@pytest.fixture(scope="module")
def wide_case():
    v = wide_inputs(0x51DE)
    return v, wide_circuit(v)


# ---- 1. header and Python agree --------------------------------------------------------------------------------------------------------
def test_public_header_and_python_agree_on_the_wide_opcodes():
    text = open(os.path.join(ROOT, "include", "mp2g.h")).read()
    body = text[text.index("enum mp2g_witness_op_wide {"):]
    body = body[:body.index("};")]
    public = {m.group(1): int(m.group(2)) for m in re.finditer(r"MP2G_(OP_[A-Z0-9_]+) = (\d+)", body)}
    assert public == {"OP_U32_INTERLEAVE": INTERLEAVE, "OP_UNINTERLEAVE_TO_B32": TO_B32, "OP_UNINTERLEAVE_TO_U32": TO_U32, "OP_U256_DIV": U256_DIV,
                      "OP_BIGUINT_DIV_REM": BIGUINT_DIV_REM, "OP_POSEIDON_MDS": POSEIDON_MDS, "OP_WIDE_END": WIDE_END}
    assert {k: v for k, v in vars(W).items() if k.startswith("OP_")} == public
    internal = open(os.path.join(ROOT, "mapreduce-plonky2_amd", "csrc", "witness.h")).read()
    for name in public:
        assert f"{name} = MP2G_{name}" in internal
    assert WIDE <= set(R._OPS) and WIDE_END not in R._OPS
    # the other blocks are where they were
    assert not any(k.startswith("OP_") and v >= 24 for k, v in vars(R).items() if isinstance(v, int))
    assert "MP2G_OP_END = 24" in text and "MP2G_OP_GF5_END = 34" in text and "MP2G_OP_LUT_END = 41" in text


# ---- 2. shape table -----------------------------------------------------------------------------------------------------------------------
def test_python_table_and_op_shape_agree_on_the_wide_opcodes(shape_test, wide_case):
    tapes = [("golden", json.load(open(GOLDEN))["wide_ops"]["tape"]), ("wide circuit", wide_case[1].tape),
             ("interleave base", interleave_base_circuit([1, 2, 3, 4]).tape)]
    seen = set()
    for name, tape in tapes:
        tape = [int(w) for w in tape]
        r = subprocess.run([shape_test], input=" ".join(str(w) for w in tape), capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stdout[-200:] + r.stderr
        native = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        mine = list(R.tape_instructions(tape)) + [(len(tape), None)]
        assert [(pos, op) for pos, op, *_ in native] == mine[:-1], name
        for (pos, op, ln, first_slot, r0, nr, w0, nw), (nxt, _) in zip(native, mine[1:]):
            assert nxt == pos + 1 + ln, (name, pos, op)
            if op not in WIDE:
                continue
            seen.add(op)
            assert first_slot == r0, (name, pos, op)  # everything from the first slot read on is a slot
            rd, wr, cells, after = R.instruction_slots(tape, pos)
            t = tape[pos + 1:]
            assert after == nxt and list(rd) == t[r0:r0 + nr] and list(wr) == t[w0:w0 + nw] and r0 + nr == w0 and w0 + nw == ln, (name, pos, op)
            assert len(set(cells)) == len(cells) == {INTERLEAVE: 34, TO_B32: 67, TO_U32: 67, U256_DIV: 0, BIGUINT_DIV_REM: 0, POSEIDON_MDS: 48}[op]
    assert seen == WIDE, sorted(WIDE - seen)


def test_op_shape_refuses_what_is_no_wide_instruction(shape_test):
    run = lambda tape: subprocess.run([shape_test], input=" ".join(map(str, tape)), capture_output=True, text=True)
    ok = {INTERLEAVE: [INTERLEAVE, 0, 2, 3, 0, 10], TO_B32: [TO_B32, 0, 1, 2, 0, 10, 11], TO_U32: [TO_U32, 0, 0, 1, 0, 10, 11],
          U256_DIV: [U256_DIV] + list(range(33)), BIGUINT_DIV_REM: [BIGUINT_DIV_REM, 3, 2] + list(range(10)),
          POSEIDON_MDS: [POSEIDON_MDS, 0] + list(range(48))}
    for op, tape in ok.items():
        assert run(tape).returncode == 0, op
        r = run(tape[:-1])                                                             # truncated by one word
        assert r.returncode == 1 and "malformed" in r.stdout, op
    for na, nb in [(0, 1), (1, 0), (33, 1), (1, 33), (1 << 40, 1), (1, 1 << 40), ((1 << 64) - 1, 1), (1, (1 << 64) - 1), (1 << 63, 1 << 63),
                   ((1 << 64) - 1, (1 << 64) - 1), ((1 << 32) + 1, 1)]:
        r = run([BIGUINT_DIV_REM, na, nb] + [0] * 200)
        assert r.returncode == 1 and "malformed" in r.stdout, (na, nb)
    assert run([BIGUINT_DIV_REM, 32, 32] + [0] * 128).returncode == 0 and run([BIGUINT_DIV_REM, 32, 32] + [0] * 127).returncode == 1
    assert run([BIGUINT_DIV_REM]).returncode == 1 and run([BIGUINT_DIV_REM, 1]).returncode == 1
    for op in (47, WIDE_END, 55):
        assert run([op] + [0] * 60).returncode == 1


def test_tape_validation_of_the_wide_opcodes():
    """mp2g_witness_program_create: rows, i < ops, the ops ranges, the limb counts, every slot operand < n_slots"""
    assert create([INTERLEAVE, 7, 2, 3, 0, 10]) is None
    assert create([INTERLEAVE, 8, 2, 3, 0, 10]) is not None                            # row 8 of 8
    assert create([INTERLEAVE, 0, 3, 3, 0, 10]) is not None                            # operation 3 of 3
    assert create([INTERLEAVE, 0, 0, 0, 0, 10]) is not None and create([INTERLEAVE, 0, 0, 4, 0, 10]) is not None  # ops = 0, ops = 4
    assert create([INTERLEAVE, 0, 0, 3, 160, 10]) is not None and create([INTERLEAVE, 0, 0, 3, 0, 160]) is not None  # slot 160 of 160
    for op in (TO_B32, TO_U32):
        assert create([op, 7, 1, 2, 0, 10, 11]) is None
        assert create([op, 8, 1, 2, 0, 10, 11]) is not None and create([op, 0, 2, 2, 0, 10, 11]) is not None
        assert create([op, 0, 0, 0, 0, 10, 11]) is not None and create([op, 0, 0, 3, 0, 10, 11]) is not None     # ops = 0, ops = 3
        assert create([op, 0, 0, 2, 0, 10, 160]) is not None
    for big in (1 << 40, 1 << 63, (1 << 64) - 1):                                      # no bound wraps
        assert create([INTERLEAVE, big, 0, 3, 0, 10]) is not None and create([INTERLEAVE, 0, big, 3, 0, 10]) is not None
        assert create([INTERLEAVE, 0, 0, big, 0, 10]) is not None and create([INTERLEAVE, 0, big, big, 0, 10]) is not None
        assert create([TO_U32, big, 0, 2, 0, 10, 11]) is not None and create([TO_U32, 0, big, big, 0, 10, 11]) is not None
        assert create([INTERLEAVE, 0, 0, 3, big, 10]) is not None and create([POSEIDON_MDS, big] + list(range(48))) is not None
        assert create([BIGUINT_DIV_REM, big, 1] + list(range(70))) is not None and create([BIGUINT_DIV_REM, 1, big] + list(range(70))) is not None
        assert create([BIGUINT_DIV_REM, big, big] + list(range(140))) is not None
    div = [U256_DIV] + list(range(17)) + list(range(20, 36))
    assert create(div) is None and create(div[:-1]) is not None
    for k in range(1, 34):                                                             # any operand one past the end
        t = list(div)
        t[k] = 160
        assert create(t) is not None, k
    big = [BIGUINT_DIV_REM, 32, 32] + list(range(64)) + list(range(70, 134))
    assert create(big) is None and create(big[:-1]) is not None
    assert create([BIGUINT_DIV_REM, 33, 32] + list(range(65)) + list(range(70, 135))) is not None
    assert create([BIGUINT_DIV_REM, 1, 0, 0, 10]) is not None and create([BIGUINT_DIV_REM, 0, 1, 0, 10]) is not None
    assert create([BIGUINT_DIV_REM, 1, 1, 0, 1, 10, 11]) is None and create([BIGUINT_DIV_REM, 1, 1, 0, 1, 10, 160]) is not None
    mds = [POSEIDON_MDS, 7] + list(range(24)) + list(range(30, 54))
    assert create(mds) is None and create([POSEIDON_MDS, 8] + mds[2:]) is not None and create(mds[:-1]) is not None
    for op in (47, WIDE_END, 55, 63):
        assert create([op] + div[1:]) is not None, op


# ---- 3. host replay equals builder, wire for wire ----------------------------------------------------------------------------------------
def test_xor_and_and_equal_python():
    rng = np.random.default_rng(0x51D0)
    words = EDGE_WORDS + [int(x) for x in rng.integers(0, 1 << 32, size=4)]
    b = R.Builder()
    t = [b.add_virtual(w) for w in words]
    for i, x in enumerate(words):
        for j, y in enumerate(words):
            xo, an = b.xor_and_u32(t[i], t[j])
            assert (xo.v, an.v) == (x ^ y, x & y), (x, y)
    assert b.xor_u32(t[1], t[2]).v == M32 ^ 0x55555555 and b.and_u32(t[2], t[3]).v == 0
    for x in words + [1 << 32 | 5]:
        assert W.interleave(x) == int("".join("0" + c for c in f"{x & M32:032b}"), 2)
    for x in [0, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555] + [int(v) for v in rng.integers(0, 1 << 63, size=4)]:
        bits = f"{x:064b}"
        assert W.uninterleave_u32(x) == (int(bits[1::2], 2), int(bits[0::2], 2))
        assert W.uninterleave_b32(x) == tuple(W.interleave(h) for h in W.uninterleave_u32(x))
    ck = b.build()
    assert not C.eval_on_points(ck, ck.pre[:ck.num_constants], ck.wires).any()


def test_host_replay_equals_the_builder_and_the_oracle_proves(wide_case):
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    v0, ck = wide_case
    others = [wide_inputs(2, words=EDGE_WORDS + EDGE_WORDS + [1], divisor=0, big_b=1),
              wide_inputs(3, dividend=5, divisor=M256, big_a=7, big_b=1 << 319)]
    ckts = [ck] + [wide_circuit(v) for v in others]
    assert all(np.array_equal(c.tape, ck.tape) and np.array_equal(c.pre, ck.pre) for c in ckts)  # the structure does not depend on values
    ops = [op for _, op in R.tape_instructions(ck.tape)]
    assert WIDE <= set(ops) and ops.count(INTERLEAVE) >= 8 * 2 + 6 and ops.count(BIGUINT_DIV_REM) == 2
    assert {C.U32_INTERLEAVE, C.UNINTERLEAVE_TO_B32, C.UNINTERLEAVE_TO_U32, C.POSEIDON_MDS} <= {g.kind for g in ck.gates}
    prog = mp2.WitnessProgram(ck)
    assert prog.n_levels >= 8 * 3  # the chain: interleave, add, uninterleave per xor
    assert all([int(x) for x in c.input_values] == wide_input_vector(v) for c, v in zip(ckts, [v0] + others))
    wires, pi_hash, pis = prog.run(np.array([c.input_values for c in ckts], dtype=np.uint64))
    for k, (c, v) in enumerate(zip(ckts, [v0] + others)):
        assert np.array_equal(wires[k], c.wires), f"host replay != builder (inputs {k})"
        assert np.array_equal(pis[k], c.public_inputs) and np.array_equal(pi_hash[k], c.pi_hash)
        assert [int(x) for x in pis[k]] == expected_public_inputs(v), k
        assert not C.eval_on_points(c, c.pre[:c.num_constants], wires[k]).any(), "a gate constraint does not vanish on the replayed wires"
    assert int(pis[1][3]) == 1 and int(pis[2][2]) == 1  # divisor 0: is_zero; dividend < divisor
    fp = C.oracle_params(ck, pow_bits=4, num_queries=2)
    _, cd = verifier_data(ck)
    caps, openings, proof, _ = C.prove_witness(ck, fp, cd, wires[0], pi_hash[0])
    assert C.verify(ck, fp, cd, pi_hash[0], caps, openings, proof) == 0
    # a word that is no u32: the interleave gate's bit decomposition no longer recomposes
    bad = ck.input_values.copy()
    bad[0] = (1 << 32) + 5
    w_bad, _, _ = prog.run(bad[None])
    assert C.eval_on_points(ck, ck.pre[:ck.num_constants], w_bad[0]).any()
    prog.free()


# ---- 4. u256.py against Python integers ---------------------------------------------------------------------------------------------------
def u256_cases():
    rng = np.random.default_rng(0x0256)
    big = lambda bits: int.from_bytes(rng.bytes(32), "little") >> (256 - bits)
    pairs = [(big(256), big(256)), (big(256), big(130)), (big(100), big(200)), (big(256), big(32)), (big(128), big(128))]
    pairs += [(a, b) for a in EDGE_U256 for b in EDGE_U256]
    pairs += [(big(256), e) for e in EDGE_U256] + [(e, big(200)) for e in EDGE_U256]
    pairs += [(1 << 128, 1 << 128), ((1 << 128) - 1, (1 << 128) + 1), (1 << 255, 2), ((1 << 255) - 1, 2), (M32 << 224, M32 << 32), (M32 << 224, 1 << 32)]
    return pairs


def test_u256_gadgets_against_python_integers():
    overflowed = set()
    for a, bb in u256_cases():
        b = R.Builder()
        ta, tb = U.add_virtual_u256(b, a), U.add_virtual_u256(b, bb)
        s, carry = U.add_u256(b, ta, tb)
        assert (U.value(s), carry.v) == ((a + bb) & M256, (a + bb) >> 256), (a, bb)
        d, borrow = U.sub_u256(b, ta, tb)
        assert (U.value(d), borrow.v) == ((a - bb) & M256, int(a < bb)), (a, bb)
        m, over = U.mul_u256(b, ta, tb)
        assert (U.value(m), over.v) == ((a * bb) & M256, int(a * bb > M256)), (a, bb)
        overflowed.add(over.v)
        assert U.is_zero(b, ta).v == int(a == 0) and U.is_equal_u256(b, ta, tb).v == int(a == bb) and U.is_equal_u256(b, ta, ta).v == 1
        assert U.is_less_than_u256(b, ta, tb).v == int(a < bb) and U.is_less_or_equal_than_u256(b, ta, tb).v == int(a <= bb)
        assert U.is_less_or_equal_than_u256(b, ta, ta).v == 1 and U.is_less_than_u256(b, ta, ta).v == 0
        assert U.value(U.select_u256(b, b.one(), ta, tb)) == a and U.value(U.select_u256(b, b.zero(), ta, tb)) == bb
        U.enforce_equal_u256(b, U.select_u256(b, carry, ta, ta), ta)
        q, r, z = U.div_u256(b, ta, tb)
        want = (0, a) if bb == 0 else divmod(a, bb)
        assert (U.value(q), U.value(r), z.v) == (*want, int(bb == 0)), (a, bb)   # check_div_result, u256.rs:1445-1446
        # is_div false: the product with its overflow flag; the hint's dummies satisfy the shared constraints
        prod, q1, r1, over2, z2 = U.mul_div_u256(b, ta, tb, b.zero())
        assert (U.value(prod), over2.v, z2.v) == ((a * bb) & M256, int(a * bb > M256), int(bb == 0)) and U.value(q1) == 1
        assert U.value(r1) == (a - a * bb) & M256 == W.u256_div(a, bb, False)[1]
        # ... and with is_div a witness rather than a constant
        flag = b.add_virtual(1)
        _, q2, r2, _, _ = U.mul_div_u256(b, ta, tb, flag)
        assert (U.value(q2), U.value(r2)) == want
        ck = b.build()
        assert not C.eval_on_points(ck, ck.pre[:ck.num_constants], ck.wires).any(), (a, bb)
    assert overflowed == {0, 1}
    # a multiplication that overflows and one that just does not
    for a, bb, want in (((1 << 128), (1 << 128), 1), ((1 << 128) - 1, (1 << 128) + 1, 0), (M256, 1, 0), (M256, 2, 1), ((1 << 255), 2, 1), ((1 << 255) - 1, 2, 0)):
        b = R.Builder()
        assert U.mul_u256(b, U.constant_u256(b, a), U.constant_u256(b, bb))[1].v == want
    assert W.u256_div(7, 0, True) == (0, 7) and W.u256_div(7, 9, True) == (0, 7) and W.u256_div(M256, 3, False) == (1, (M256 - 3 * M256) & M256)
    assert W.biguint_div_rem(1 << 100, 0, 2) == (0, 0) and W.biguint_div_rem((1 << 100) + 9, 0, 2) == (0, 9) and W.biguint_div_rem(100, 7, 1) == (14, 2)


class _OffByOne(R.Builder):
    """a dishonest generator: quotient + 1"""

    def u256_div_hint(self, a, b, is_div):
        q, r = super().u256_div_hint(a, b, is_div)
        q[0].v = (q[0].v + 1) % P
        return q, r


def test_a_wrong_division_hint_fails_the_witness_check():
    a, bb = 0x1234567890ABCDEF << 100, 0xFEDCBA987
    def circuit(builder):
        ta, tb = U.add_virtual_u256(builder, a), U.add_virtual_u256(builder, bb)
        q, r, _ = U.div_u256(builder, ta, tb)
        builder.register_public_inputs(q + r)
        return builder.build()
    good = circuit(R.Builder())
    assert W.from_limbs(good.public_inputs[:8]) == a // bb
    with pytest.raises(AssertionError):
        circuit(_OffByOne())                     # the eager builder stops at quotient divisor + remainder = dividend
    bad = circuit(_OffByOne(strict=False))       # built anyway: same circuit, a witness that violates it
    assert np.array_equal(bad.pre, good.pre) and W.from_limbs(bad.public_inputs[:8]) == a // bb + 1
    fp = C.oracle_params(good, pow_bits=4, num_queries=2)
    _, cd = verifier_data(good)
    for ck, accepted in ((good, True), (bad, False)):
        caps, openings, proof, _ = C.prove_witness(ck, fp, cd, ck.wires, ck.pi_hash)
        assert (C.verify(ck, fp, cd, ck.pi_hash, caps, openings, proof) == 0) == accepted


# ---- 5. wrap --------------------------------------------------------------------------------------------------------------------------------
def test_a_circuit_with_interleave_rows_is_wrapped():
    words = [0xDEADBEEF, 0x12345678, 0xFFFFFFFF, 0x0F0F0F0F]
    base = interleave_base_circuit(words)
    assert [int(x) for x in base.public_inputs[:3]] == [words[0] ^ words[1], words[0] & words[1], words[2] ^ words[3]]
    assert {C.U32_INTERLEAVE, C.UNINTERLEAVE_TO_B32, C.UNINTERLEAVE_TO_U32} <= {g.kind for g in base.gates}
    fp = C.oracle_params(base, pow_bits=4, num_queries=2)
    cap, cd = verifier_data(base)
    caps, openings, proof, _ = C.prove(base, fp, cd)
    assert C.verify(base, fp, cd, base.pi_hash, caps, openings, proof) == 0
    inner = R.InnerCircuit(base, fp, cap, cd, len(base.public_inputs))
    wrap = R.wrap_circuit(inner, caps, openings, proof, base.public_inputs)
    assert not C.eval_on_points(wrap, wrap.pre[:wrap.num_constants], wrap.wires).any()
    assert np.array_equal(wrap.public_inputs, base.public_inputs)
    wfp = C.oracle_params(wrap, pow_bits=4, num_queries=2)
    _, wcd = verifier_data(wrap)
    wc, wo, wp, _ = C.prove(wrap, wfp, wcd)
    assert C.verify(wrap, wfp, wcd, wrap.pi_hash, wc, wo, wp) == 0
    # one bit wire of an interleave row (of an uninterleave row) flipped before proving: the base proof does not verify, and the
    # wrap over it is not provable -- the in-circuit evaluator of the gate carries the failed constraint
    for kind, wire in ((C.U32_INTERLEAVE, 2 * 3 + 31), (C.UNINTERLEAVE_TO_U32, 3 * 2 + 5)):
        flipped = interleave_base_circuit(words, flip=(kind, wire))
        assert np.array_equal(flipped.pre, base.pre) and C.eval_on_points(flipped, flipped.pre[:flipped.num_constants], flipped.wires).any()
        bc, bo, bp, _ = C.prove(flipped, fp, cd)
        assert C.verify(flipped, fp, cd, flipped.pi_hash, bc, bo, bp) != 0
        with pytest.raises(AssertionError):
            R.wrap_circuit(inner, bc, bo, bp, flipped.public_inputs)
        bad_wrap = R.wrap_circuit(inner, bc, bo, bp, flipped.public_inputs, strict=False)
        assert np.array_equal(bad_wrap.pre, wrap.pre)
        c2, o2, p2, _ = C.prove(bad_wrap, wfp, wcd)
        assert C.verify(bad_wrap, wfp, wcd, bad_wrap.pi_hash, c2, o2, p2) != 0


# ---- 6. golden tape -----------------------------------------------------------------------------------------------------------------------
def test_host_replay_reproduces_the_golden_wide_tape():
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    doc = json.load(open(GOLDEN))
    assert "self-made" in doc["_generator"]
    g = doc["wide_ops"]
    assert g["log_n"] == 3 and set(g["opcodes_used"]) >= WIDE
    prog = mp2.WitnessProgram(golden_program(g))
    a = np.array([c["inputs"] for c in g["cases"]], dtype=np.uint64)
    wires, head, rest = prog.run(a)
    for k, c in enumerate(g["cases"]):
        assert np.array_equal(wires[k], golden_wires(c, g["log_n"])), k
        assert [int(v) for v in head[k]] + [int(v) for v in rest[k]] == c["slots"], k
    prog.free()


# ---- 7. fuzz ------------------------------------------------------------------------------------------------------------------------------
def test_random_wide_tapes_are_refused_or_replayed_without_harm():
    """400 random tapes of the six wide opcodes, operands drawn around their limits (rows, operation indices, counts, limb counts,
    slots one past the end; now and then 2^40, 2^63 or 2^64 - 1), some truncated: each is refused, or replayed on the host for two
    input vectors into a guarded wire buffer and a guarded probe with the guards intact"""
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    lib = mp2.load()
    rng = np.random.default_rng(0x51D7)
    log_n, n_slots, n = 3, 150, 8

    def slot():
        return int(rng.integers(0, n_slots + (1 if rng.random() < 0.02 else 0)))

    def row():
        return int(rng.integers(0, n + (1 if rng.random() < 0.05 else 0)))

    def cnt(lo, hi):
        if rng.random() < 0.03:
            return [1 << 40, 1 << 63, (1 << 64) - 1][int(rng.integers(0, 3))]
        return int(rng.integers(lo, hi))

    def instr():
        op = int(rng.integers(INTERLEAVE, WIDE_END + 1))
        sl = lambda k: [slot() for _ in range(k)]
        if op == INTERLEAVE: return [op, row(), cnt(0, 4), cnt(0, 5)] + sl(2)
        if op in (TO_B32, TO_U32): return [op, row(), cnt(0, 3), cnt(0, 4)] + sl(3)
        if op == U256_DIV: return [op] + sl(33)
        if op == BIGUINT_DIV_REM:
            na, nb = cnt(0, 35), cnt(0, 35)
            return [op, na, nb] + sl(2 * (min(na, 34) + min(nb, 34)))
        if op == POSEIDON_MDS: return [op, row()] + sl(48)
        return [op, 0, 0]  # MP2G_OP_WIDE_END: no such opcode

    accepted = 0
    ins = np.arange(8, dtype=np.uint32)
    probe = np.arange(n_slots, dtype=np.uint32)
    for _ in range(400):
        tape = []
        for _ in range(int(rng.integers(1, 4))):
            tape += instr()
        if rng.random() < 0.1:
            tape = tape[:-1]
        t = np.ascontiguousarray(tape, dtype=np.uint64)
        h = ctypes.c_void_p()
        rc = lib.mp2g_witness_program_create(t.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(t.size), n_slots, log_n,
                                             ins.ctypes.data_as(ctypes.c_void_p), 8, None, 0, ctypes.byref(h))
        if rc:
            continue
        accepted += 1
        guard = 64
        wires = np.full(2 * 135 * n + 2 * guard, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        out = np.full(2 * n_slots + 2 * guard, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        inputs = np.ascontiguousarray(O.rand_field(16, int(rng.integers(1, 1 << 30))).reshape(2, 8))
        rc = lib.mp2g_witness_program_run(h, inputs.ctypes.data_as(ctypes.c_void_p), 2, 2, ctypes.c_void_p(wires.ctypes.data + 8 * guard),
                                          probe.ctypes.data_as(ctypes.c_void_p), n_slots, ctypes.c_void_p(out.ctypes.data + 8 * guard))
        assert rc == 0
        for buf in (wires, out):
            assert (buf[:guard] == 0xDEADBEEFDEADBEEF).all() and (buf[-guard:] == 0xDEADBEEFDEADBEEF).all(), "a replay wrote outside its buffers"
        lib.mp2g_witness_program_free(h)
    assert 20 <= accepted <= 380, accepted  # both outcomes occur


def test_division_opcodes_against_python_integers():
    """MP2G_OP_U256_DIV and MP2G_OP_BIGUINT_DIV_REM replayed from hand-written tapes: every branch of the u256 generator, limb
    counts 1..32 on either side, operands with leading zero limbs, a zero divisor, limb slots holding more than 32 bits"""
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    rng = np.random.default_rng(0xD1F)
    big = lambda limbs: int.from_bytes(rng.bytes(4 * limbs), "little") >> int(rng.integers(0, 32 * limbs))

    class prog_of:
        def __init__(self, tape, n_in, n_out):
            self.tape, self.input_sids = np.array(tape, dtype=np.uint64), np.arange(n_in, dtype=np.uint32)
            self.const_slots, self.n_slots, self.log_n = np.zeros((0, 2), dtype=np.uint64), n_in + n_out, 3
            # every result slot is probed (run() hands the probe back in two parts: the first four words, the rest)
            self.pi_hash_sids, self.public_input_sids = np.arange(n_in, n_in + n_out, dtype=np.uint32), np.zeros(0, dtype=np.uint32)

    prog = mp2.WitnessProgram(prog_of([U256_DIV] + list(range(33)), 17, 16))
    cases = [(a, b, f) for a, b in u256_cases() for f in (1, 0)] + [(big(8), big(8), 7) for _ in range(8)]
    rows = [W.to_limbs(a, 8) + W.to_limbs(b, 8) + [f] for a, b, f in cases]
    rows.append([x + (k + 1 << 32) for k, x in enumerate(W.to_limbs(M256 - 5, 8))] + [x + (5 << 32) for x in W.to_limbs(12345, 8)] + [1])  # more than 32 bits a slot
    cases.append((M256 - 5, 12345, 1))
    _, head, rest = prog.run(np.array(rows, dtype=np.uint64))
    for k, (a, b, f) in enumerate(cases):
        got = [int(x) for x in head[k]] + [int(x) for x in rest[k]]
        assert (W.from_limbs(got[:8]), W.from_limbs(got[8:])) == W.u256_div(a, b, f) and max(got) <= M32, (a, b, f)
    prog.free()
    edge = [0, 1, 0x7FFFFFFF, 0x80000000, M32]
    for na, nb in [(1, 1), (1, 32), (32, 1), (32, 32), (20, 10), (10, 20), (7, 3), (2, 2), (31, 17), (4, 3), (5, 2)]:
        prog = mp2.WitnessProgram(prog_of([BIGUINT_DIV_REM, na, nb] + list(range(2 * (na + nb))), na + nb, na + nb))
        cases = [(big(na), big(nb)) for _ in range(6)] + [(big(na), 0), (0, big(nb)), ((1 << 32 * na) - 1, (1 << 32 * nb) - 1), ((1 << 32 * na) - 1, 1),
                                                         (big(na), 1 << (32 * nb - 1)), ((1 << 32 * na) - 1, (1 << 32 * (nb - 1)) + 1)]
        if na <= 5:  # digits at their limits: quotient-digit estimates that are one or two too large, and the add-back step, which
            # random operands reach once in 2^31 digits (0x7fffffff 80000000 00000000 00000000 / 0x80000000 00000000 00000001 needs it)
            cases += [(0x7FFFFFFF << 96 | 0x80000000 << 64, 0x80000000 << 64 | 1)] if (na, nb) == (4, 3) else []
            cases += [(W.from_limbs(rng.choice(edge, size=na)), W.from_limbs(rng.choice(edge, size=nb))) for _ in range(300)]
        _, head, rest = prog.run(np.array([W.to_limbs(a, na) + W.to_limbs(b, nb) for a, b in cases], dtype=np.uint64))
        for k, (a, b) in enumerate(cases):
            got = [int(x) for x in head[k]] + [int(x) for x in rest[k]]
            assert (W.from_limbs(got[:na]), W.from_limbs(got[na:])) == W.biguint_div_rem(a, b, nb) and max(got) <= M32, (na, nb, a, b)
        prog.free()
