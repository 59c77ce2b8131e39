"""The witness tape's GF(p^5) opcodes (include/mp2g.h enum mp2g_witness_op_gf5: MP2G_OP_QUINTIC_SQRT, MP2G_OP_QUINTIC_QUOTIENT) on the
CPU: validation by mp2g_witness_program_create, the library's host replay against the builder's eager values (gf5.py), every result
checked with the ORACLE's GF(p^5) arithmetic (orc_gl5_mul / _sqrt / _sgn0), the golden tape, and a fuzz of tapes that mix the new
opcodes with the base set. The device replay of the same tapes is tests/test_gpu_witness_tape_gf5.py."""
import ctypes
import importlib
import json
import os
import re

import numpy as np

import oracle as O

R = importlib.import_module("mapreduce-plonky2_amd.recursion")
GF5 = importlib.import_module("mapreduce-plonky2_amd.gf5")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "witness_tape_gf5_vectors.json")
P = O.P
SQRT, QUOT = 32, 33  # the header's numbers, written out: a renumbering must fail here


# ---- the oracle's GF(p^5) arithmetic ------------------------------------------------------------------------------------------------
def orc_mul(a, b):
    x, y, o = O.arr(a), O.arr(b), np.zeros(5, dtype=np.uint64)
    O.lib().orc_gl5_mul(O.p(x), O.p(y), O.p(o))
    return tuple(int(v) for v in o)


def orc_sqrt(a):
    """(is a square, some root) by the oracle"""
    x, o = O.arr(a), np.zeros(5, dtype=np.uint64)
    ok = O.lib().orc_gl5_sqrt(O.p(x), O.p(o))
    return bool(ok), tuple(int(v) for v in o)


def orc_sgn0(a):
    return int(O.lib().orc_gl5_sgn0(O.p(O.arr(a))))


# ---- a circuit that uses both hints --------------------------------------------------------------------------------------------------
def gf5_hint_circuit(x, a, b):
    """root, is_sqrt = quintic_sqrt(x) and q = quintic_quotient(a, b) as two sections of a parallel region; chained on their outputs,
    q2 = quintic_quotient(root, x) and (r2, s2) = quintic_sqrt(q); public inputs root, is_sqrt, q, q2, r2, s2. Inputs: x, a, b (15
    words)."""
    bl = R.Builder()
    tx, ta, tb = ([bl.add_virtual(int(v)) for v in e] for e in (x, a, b))
    with bl.parallel_sections() as region:  # the region's check walks the new instructions (recursion.instruction_slots)
        with region.section():
            root, is_sqrt = bl.quintic_sqrt(tx)
        with region.section():
            q = bl.quintic_quotient(ta, tb)
    q2 = bl.quintic_quotient(root, tx)
    r2, s2 = bl.quintic_sqrt(q)
    bl.register_public_inputs(root + [is_sqrt] + q + q2 + r2 + [s2])
    return bl.build()


def rand_elem(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=5, dtype=np.uint64))


def hint_inputs(seed, n):
    """n input vectors (x, a, b): x a square in about half of them (one is x = 0), one b = 0 and one a = 0"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        x = rand_elem(rng)
        if k % 2 == 0:
            x = GF5.mul(x, x)
        a, b = rand_elem(rng), rand_elem(rng)
        if k == 1:
            x = GF5.ZERO
        if k == 2:
            b = GF5.ZERO
        if k == 3:
            a = GF5.ZERO
        out.append((x, a, b))
    return out


def check_hint_values(x, a, b, root, is_sqrt, q):
    """the opcodes' rules, by the oracle's arithmetic alone"""
    square, _ = orc_sqrt(x)
    if is_sqrt == 1:
        assert square and orc_mul(root, root) == tuple(x) and orc_sgn0(root) == 0, "not the root with sgn0 = 0"
    else:
        assert is_sqrt == 0 and tuple(root) == GF5.ZERO and not square, "a square reported as none"
    if tuple(b) != GF5.ZERO:
        assert orc_mul(q, b) == tuple(a), "q b != a"
    else:
        assert tuple(q) == GF5.ZERO


def create(tape, n_slots=64, log_n=3, n_inputs=4):
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


def test_tapes_with_the_gf5_opcodes_are_accepted():
    assert create([SQRT] + list(range(0, 5)) + list(range(10, 15)) + [15]) is None
    assert create([QUOT] + list(range(0, 10)) + list(range(20, 25))) is None
    # mixed with the base set, chained through their slots
    assert create([SQRT] + list(range(0, 5)) + list(range(10, 16)) + [QUOT] + list(range(10, 15)) + list(range(0, 5)) + list(range(20, 25))
                  + [R.OP_WIRE, 0, 0, 15]) is None


def test_tape_validation_of_the_gf5_opcodes():
    ok_sqrt = [SQRT] + list(range(0, 5)) + list(range(10, 15)) + [15]
    ok_quot = [QUOT] + list(range(0, 10)) + list(range(20, 25))
    assert create(ok_sqrt[:-1]) is not None and create(ok_quot[:-1]) is not None     # truncated
    assert create(ok_sqrt, n_slots=16) is None and create(ok_sqrt, n_slots=15) is not None  # slot 15 of 15
    assert create(ok_quot, n_slots=25) is None
    for k in range(1, 16):                                                           # any operand one past the end
        t = list(ok_quot)
        t[k] = 25
        assert create(t, n_slots=25) is not None, k
    for op in (0, 24, 31, 34, 35, 64, 1 << 40):                                      # outside [1, 24) and [32, 34)
        assert create([op] + ok_sqrt[1:]) is not None, op
        assert create([op] + ok_quot[1:]) is not None, op


def test_host_replay_equals_the_builder_and_the_oracle():
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    ins = hint_inputs(0x5E1, 24)
    ckts = [gf5_hint_circuit(*v) for v in ins]
    ck = ckts[0]
    assert all(np.array_equal(c.tape, ck.tape) and np.array_equal(c.pre, ck.pre) for c in ckts)  # the structure does not depend on values
    assert {op for _, op in R.tape_instructions(ck.tape)} >= {SQRT, QUOT, R.OP_PAR}
    roles = {}
    for pos, op in R.tape_instructions(ck.tape):
        if op in (SQRT, QUOT):
            rd, wr, cells, nxt = R.instruction_slots(ck.tape, pos)
            roles.setdefault(op, (len(rd), len(wr), len(cells), nxt - pos))
    assert roles == {SQRT: (5, 6, 0, 12), QUOT: (10, 5, 0, 16)}
    prog = mp2.WitnessProgram(ck)
    a = np.array([[w for e in v for w in e] for v in ins], dtype=np.uint64)
    wires, pi_hash, pis = prog.run(a)
    w1, _, _ = prog.run(a[:1], threads=4)  # fewer proofs than threads: the parallel region's sections on separate threads
    assert np.array_equal(w1[0], wires[0])
    squares = 0
    for k, (c, (x, av, bv)) in enumerate(zip(ckts, ins)):
        assert np.array_equal(wires[k], c.wires) and np.array_equal(pis[k], c.public_inputs) and np.array_equal(pi_hash[k], c.pi_hash), k
        pi = [int(v) for v in pis[k]]
        root, is_sqrt, q, q2, r2, s2 = pi[0:5], pi[5], pi[6:11], pi[11:16], pi[16:21], pi[21]
        check_hint_values(x, av, bv, root, is_sqrt, q)
        check_hint_values(q, root, x, r2, s2, q2)
        squares += is_sqrt
    assert 8 <= squares <= 20, squares
    assert int(pis[0][5]) == 1 and int(pis[2][5]) == 1                               # the squares made as squares
    assert [int(v) for v in pis[1][:5]] == [0] * 5 and int(pis[1][5]) == 1          # x = 0: a square, root 0
    assert [int(v) for v in pis[2][6:11]] == [0] * 5                                # b = 0: q = 0
    assert [int(v) for v in pis[3][6:11]] == [0] * 5                                # a = 0: q = 0
    prog.free()


def test_public_header_and_python_agree_on_the_gf5_opcodes():
    text = open(os.path.join(ROOT, "include", "mp2g.h")).read()
    body = text[text.index("enum mp2g_witness_op_gf5 {"):]
    body = body[:body.index("};")]
    public = {m.group(1): int(m.group(2)) for m in re.finditer(r"MP2G_(OP_[A-Z0-9_]+) = (\d+)", body)}
    assert public == {"OP_QUINTIC_SQRT": 32, "OP_QUINTIC_QUOTIENT": 33, "OP_GF5_END": 34}
    assert {k: v for k, v in vars(GF5).items() if k.startswith("OP_")} == public
    assert not any(k.startswith("OP_") and v >= 24 for k, v in vars(R).items() if isinstance(v, int))
    internal = open(os.path.join(ROOT, "mapreduce-plonky2_amd", "csrc", "witness.h")).read()
    for name in public:
        assert f"{name} = MP2G_{name}" in internal


def test_gf5_module_against_the_oracle():
    """gf5.py (the builder's eager values) agrees with the oracle: products, inverses, square-root existence and the sgn0 rule"""
    rng = np.random.default_rng(0x5E2)
    for _ in range(12):
        a, b = rand_elem(rng), rand_elem(rng)
        assert GF5.mul(a, b) == orc_mul(a, b)
        assert orc_mul(GF5.inv(a), a) == GF5.ONE
        square, some_root = orc_sqrt(a)
        r = GF5.sqrt(a)
        assert (r is not None) == square == GF5.is_square(a)
        if square:
            assert r in (some_root, GF5.neg(some_root)) and orc_sgn0(r) == GF5.sgn0(r) == 0
    assert GF5.inv(GF5.ZERO) == GF5.ZERO and GF5.sqrt(GF5.ZERO) == GF5.ZERO


def test_host_replay_reproduces_the_golden_gf5_tape():
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    g = json.load(open(GOLDEN))["gf5_hints"]
    assert set(g["opcodes_used"]) >= {SQRT, QUOT}
    ck = _golden_program(g)
    prog = mp2.WitnessProgram(ck)
    a = np.array([c["inputs"] for c in g["cases"]], dtype=np.uint64)
    wires, pi_hash, pis = prog.run(a)
    for k, c in enumerate(g["cases"]):
        assert fnv(wires[k]) == c["wires_fnv1a"]
        assert [int(v) for v in pi_hash[k]] + [int(v) for v in pis[k]] == c["probe"]
    prog.free()


class _golden_program:
    """the fields of a golden tape in the shape mp2.WitnessProgram takes"""

    def __init__(self, g):
        self.tape = np.array(g["tape"], dtype=np.uint64)
        self.input_sids = np.array(g["input_sids"], dtype=np.uint32)
        self.const_slots = np.array(g["const_slots"], dtype=np.uint64).reshape(-1, 2)
        self.n_slots, self.log_n = g["n_slots"], g["log_n"]
        self.pi_hash_sids = np.array(g["probe"][:4], dtype=np.uint32)
        self.public_input_sids = np.array(g["probe"][4:], dtype=np.uint32)


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_random_tapes_with_gf5_opcodes_are_refused_or_replayed_without_harm():
    """random tapes mixing the GF(p^5) opcodes with base-set ones, operands around their limits (slots one past the end, opcodes just
    outside both blocks, truncations): each is refused, or replayed on the host inside a guarded wire buffer and a guarded probe"""
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    lib = mp2.load()
    rng = np.random.default_rng(0x5E3)
    log_n, n_slots, n = 3, 40, 8

    def slot():
        return int(rng.integers(0, n_slots + (1 if rng.random() < 0.05 else 0)))

    def row():
        return int(rng.integers(0, n + (1 if rng.random() < 0.05 else 0)))

    def instr():
        sl = lambda k: [slot() for _ in range(k)]
        c = int(rng.integers(0, 8))
        if c <= 1: return [SQRT] + sl(11)
        if c <= 3: return [QUOT] + sl(15)
        if c == 4: return [R.OP_WIRE, row(), int(rng.integers(0, 137))] + sl(1)
        if c == 5: return [R.OP_HINT_DIV_EXT] + sl(6)
        if c == 6: return [R.OP_ARITH, row(), int(rng.integers(0, 21)), 1, 1] + sl(4)
        return [int(rng.choice([0, 24, 31, 34, 35]))] + sl(int(rng.integers(0, 16)))  # no such opcode

    accepted = 0
    ins = np.arange(4, dtype=np.uint32)
    probe_sids = np.arange(0, n_slots, 3, dtype=np.uint32)
    for _ in range(300):
        tape = []
        for _ in range(int(rng.integers(1, 6))):
            tape += instr()
        if rng.random() < 0.1:
            tape = tape[:-int(rng.integers(1, 4))]
        t = np.ascontiguousarray(tape, dtype=np.uint64)
        h = ctypes.c_void_p()
        rc = lib.mp2g_witness_program_create(t.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(t.size), n_slots, log_n,
                                             ins.ctypes.data_as(ctypes.c_void_p), 4, None, 0, ctypes.byref(h))
        if rc:
            continue
        accepted += 1
        guard = 64
        wires = np.full(2 * 135 * n + 2 * guard, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        probe = np.full(2 * probe_sids.size + 2 * guard, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        inputs = np.ascontiguousarray(O.rand_field(8, int(rng.integers(1, 1 << 30))).reshape(2, 4))
        rc = lib.mp2g_witness_program_run(h, inputs.ctypes.data_as(ctypes.c_void_p), 2, 2, ctypes.c_void_p(wires.ctypes.data + 8 * guard),
                                          probe_sids.ctypes.data_as(ctypes.c_void_p), int(probe_sids.size), ctypes.c_void_p(probe.ctypes.data + 8 * guard))
        assert rc == 0
        assert (wires[:guard] == 0xDEADBEEFDEADBEEF).all() and (wires[-guard:] == 0xDEADBEEFDEADBEEF).all(), "a replay wrote outside the wire matrix"
        assert (probe[:guard] == 0xDEADBEEFDEADBEEF).all() and (probe[-guard:] == 0xDEADBEEFDEADBEEF).all(), "a replay wrote outside the probe"
        assert (probe[guard:-guard] < P).all(), "a slot holds a non-canonical value"
        lib.mp2g_witness_program_free(h)
    assert 20 <= accepted <= 280, accepted  # both outcomes occur
