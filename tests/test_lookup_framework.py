"""Lookup tables in the framework, on the CPU (the oracle proves; no GPU): recursion.Builder.add_lookup_table / add_lookup_from_index,
the witness tape's MP2G_OP_LOOKUP with mp2g_witness_program_set_lookups (host replay: the opcode, then prove()'s set_lookup_wires),
the in-circuit verifier's lookup argument (a wrap circuit around a proof with lookup polynomials), and the byte-realignment leaf of
the values-extraction column gadget (recursion.column_realign_logic) in a circuit set with a two-verifier parent. The GPU side is
tests/test_gpu_lookup_wires.py."""
import ctypes
import importlib
import json
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import circuits as C
import hosttest
import oracle as O
from test_recursion import OracleProver, verifier_data

R = importlib.import_module("mapreduce-plonky2_amd.recursion")
LUT = importlib.import_module("mapreduce-plonky2_amd.lut")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
ROOT = O.ROOT


def leaf_inputs(seed, offset=None):
    """32 value bytes and a bit offset in 0..7"""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, 256, 32)] + [int(rng.integers(0, 8)) if offset is None else offset]


def extract_leaf(inputs, strict=True):
    b = R.Builder(strict)
    b.register_public_inputs(R.column_realign_logic(b, [], inputs))
    return b.build()


def merge_logic(b, child_pis, inputs):
    """a reduce-style parent for the leaf's 8 public inputs: the limb-wise sum of its two children's"""
    return [b.add(x, y) for x, y in zip(child_pis[0], child_pis[1])]


def framework_circuits():
    return [R.FrameworkCircuit("extract", 0, R.column_realign_logic, 8), R.FrameworkCircuit("merge", 2, merge_logic, 8)]


# ---- 1. the builder ------------------------------------------------------------------------------------------------------------------
def test_builder_column_realign_leaf():
    vals = leaf_inputs(1)[:32]
    ckts = [extract_leaf(vals + [j]) for j in range(8)]
    for j, ckt in enumerate(ckts):
        assert [int(x) for x in ckt.public_inputs] == R.column_realign_value(vals, j)
        assert np.array_equal(ckt.pre, ckts[0].pre) and np.array_equal(ckt.tape, ckts[0].tape)  # neither depends on the input values
    assert R.column_realign_value([0x80] + [0] * 30 + [0xFF], 1) == [0] * 7 + [0x1FE]  # the top bit leaves, the last byte moves up
    ckt = ckts[3]
    other = extract_leaf(leaf_inputs(2))
    assert np.array_equal(other.pre, ckt.pre) and np.array_equal(other.tape, ckt.tape) and not np.array_equal(other.wires, ckt.wires)
    assert ckt.log_n == 8 and len(ckt.luts) == 14 and ckt.num_lookup_selectors == 4 + 14 and ckt.num_lookup_polys == 7
    assert ckt.num_constants == ckt.num_selectors + 18 + 2
    assert sum(t["n_lookups"] for t in ckt.luts) == 441 and sorted({t["n_lookups"] for t in ckt.luts}) == [31, 32]
    assert {len(t["table"]) for t in ckt.luts} == {256, 257, 264}
    assert {C.LOOKUP, C.LOOKUP_TABLE} <= {g.kind for g in ckt.gates}
    # every gate constraint vanishes on H (the gates see the selectors and the gate constants, not the lookup selectors between them)
    gate_consts = np.delete(ckt.pre[:ckt.num_constants], range(ckt.num_selectors, ckt.num_selectors + ckt.num_lookup_selectors), axis=0)
    assert not C.eval_on_points(ckt, gate_consts, ckt.wires).any()
    fp = C.oracle_params(ckt, pow_bits=6, num_queries=4)
    cap, cd = verifier_data(ckt)
    caps, openings, proof, _ = C.prove(ckt, fp, cd)
    assert C.verify(ckt, fp, cd, ckt.pi_hash, caps, openings, proof) == 0
    for t in ckt.luts:
        n_lu, n_lut = t["last_lut_row"] - t["last_lu_row"], t["first_lut_row"] - t["last_lut_row"] + 1
        assert (n_lu, n_lut) == LUT.rows_needed(len(t["table"]), t["n_lookups"]) and n_lut * 26 > len(t["table"])  # a padded last row
        assert ckt.instances[t["first_lut_row"] + 1] == next(i for i, g in enumerate(ckt.gates) if g.kind == C.NOOP)
        pairs = [(int(a), int(b)) for a, b in t["table"]]
        # the LookupTableGate rows = a Counter over the lookups the tape records for this table, plus the padding
        seen = Counter()
        for j in range(n_lu * 40):
            r, c = t["last_lu_row"] + j // 40, 2 * (j % 40)
            pair = (int(ckt.wires[c, r]), int(ckt.wires[c + 1, r]))
            assert j < t["n_lookups"] or pair == pairs[0]
            seen[pair] += 1
        assert set(seen) <= set(pairs)
        mult = 0
        for e in range(n_lut * 26):
            r, c = t["first_lut_row"] - e // 26, 3 * (e % 26)
            got = tuple(int(ckt.wires[c + k, r]) for k in range(3))
            assert got == ((pairs[e][0], pairs[e][1], seen[pairs[e]]) if e < len(pairs) else (0, 0, 0))
            mult += got[2]
        assert mult == 40 * n_lu
    # the tape holds one MP2G_OP_LOOKUP per lookup, each in its table's rows
    lookups = [ckt.tape[pos + 1:pos + 6] for pos, op in R.tape_instructions(ckt.tape) if op == LUT.OP_LOOKUP]
    assert len(lookups) == 441
    assert all(ckt.luts[int(t[2])]["last_lu_row"] <= int(t[0]) < ckt.luts[int(t[2])]["last_lut_row"] and int(t[1]) < 40 for t in lookups)
    # a circuit without tables builds as before: no lookup selectors, no lookup polynomials, no lookup opcode
    plain = R.map_circuit(O.rand_field(4, 77))
    assert plain.luts == [] and plain.num_lookup_selectors == 0 and plain.num_lookup_polys == 0 and plain.num_constants == plain.num_selectors + 2
    assert LUT.OP_LOOKUP not in {op for _, op in R.tape_instructions(plain.tape)}


def test_builder_refuses_bad_tables():
    b = R.Builder()
    with pytest.raises(AssertionError):
        b.add_lookup_table([(1, 2), (1, 3)])  # an input twice
    with pytest.raises(AssertionError):
        b.add_lookup_table([(1, 70000)])
    idx = b.add_lookup_table_from_fn(lambda v: v + 1, range(4))
    assert idx == 0 and b.add_lookup_from_index(b.add_virtual(3), idx).v == 4
    with pytest.raises(AssertionError):
        b.add_lookup_from_index(b.add_virtual(9), idx)  # the strict builder stops at an input the table does not hold


# ---- 2. header, Python table and op_shape ------------------------------------------------------------------------------------------
def test_header_and_python_agree_on_the_lookup_block():
    text = open(os.path.join(ROOT, "include", "mp2g.h")).read()
    assert text.index("enum mp2g_witness_op_gf5 {") < text.index("enum mp2g_witness_op_lut {")
    body = text[text.index("enum mp2g_witness_op_lut {"):]
    body = body[:body.index("};")]
    public = {m.group(1): int(m.group(2)) for m in re.finditer(r"MP2G_(OP_[A-Z0-9_]+) = (\d+)", body)}
    assert public == {"OP_LOOKUP": 40, "OP_LUT_END": 41}
    assert {k: v for k, v in vars(LUT).items() if k.startswith("OP_")} == public
    internal = open(os.path.join(ROOT, "mapreduce-plonky2_amd", "csrc", "witness.h")).read()
    for name in public:
        assert f"{name} = MP2G_{name}" in internal
    assert LUT.OP_LOOKUP in R._OPS and LUT.OP_LUT_END not in R._OPS


@pytest.fixture(scope="module")
def shape_test(tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("witness_shape_lut"), "witness_shape_test")


def test_python_table_and_op_shape_agree_on_a_lookup_tape(shape_test):
    tape = [int(w) for w in extract_leaf(leaf_inputs(3)).tape]
    r = subprocess.run([shape_test], input=" ".join(str(w) for w in tape), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-200:] + r.stderr
    native = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    mine = list(R.tape_instructions(tape))
    assert [(pos, op) for pos, op, *_ in native] == mine
    n_lookup = 0
    for pos, op, ln, first_slot, r0, nr, w0, nw in native:
        if op != LUT.OP_LOOKUP:
            continue
        n_lookup += 1
        assert (ln, first_slot, r0, nr, w0, nw) == (5, 3, 3, 1, 4, 1)
        rd, wr, cells, after = R.instruction_slots(tape, pos)
        t = tape[pos + 1:]
        assert after == pos + 6 and list(rd) == t[3:4] and list(wr) == t[4:5] and cells == [(t[0], 2 * t[1]), (t[0], 2 * t[1] + 1)]
    assert n_lookup == 441
    for bad in ([39, 0, 0, 0, 0, 0], [41, 0, 0, 0, 0, 0], [40, 0, 0, 0, 0]):  # 39 and 41 are no opcodes; a lookup cut short
        r = subprocess.run([shape_test], input=" ".join(map(str, bad)), capture_output=True, text=True)
        assert r.returncode == 1 and "malformed" in r.stdout, bad


# ---- 3. host replay --------------------------------------------------------------------------------------------------------------------
class Program:
    """mp2g_witness_program_* by hand (create / set_lookups return codes instead of exceptions)"""

    def __init__(self, mp2, tape, n_slots=16, log_n=4, n_inputs=4):
        self.mp2, self.lib, self.log_n, self.n_inputs = mp2, mp2.load(), log_n, n_inputs
        t = np.ascontiguousarray(tape, dtype=np.uint64)
        ins = np.arange(n_inputs, dtype=np.uint32)
        self.h = ctypes.c_void_p()
        self.rc = self.lib.mp2g_witness_program_create(t.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(t.size), n_slots, log_n,
                                                       ins.ctypes.data_as(ctypes.c_void_p), n_inputs, None, 0, ctypes.byref(self.h))

    def set_lookups(self, luts):
        arr, keep = self.mp2.lookup_array(luts)
        return self.lib.mp2g_witness_program_set_lookups(self.h, arr, len(luts))

    def run(self, inputs, probe=(), guard=64):
        """(rc, wires [B][135][n], probe values); asserts that nothing outside the wire matrices was written"""
        a = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, self.n_inputs)
        B, n = a.shape[0], 1 << self.log_n
        buf = np.full(B * 135 * n + 2 * guard, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        sids = np.ascontiguousarray(probe, dtype=np.uint32)
        out = np.zeros((B, max(1, sids.size)), dtype=np.uint64)
        rc = self.lib.mp2g_witness_program_run(self.h, a.ctypes.data_as(ctypes.c_void_p), B, 2, ctypes.c_void_p(buf.ctypes.data + 8 * guard),
                                               sids.ctypes.data_as(ctypes.c_void_p) if sids.size else None, int(sids.size),
                                               out.ctypes.data_as(ctypes.c_void_p) if sids.size else None)
        assert (buf[:guard] == 0xDEADBEEFDEADBEEF).all() and (buf[-guard:] == 0xDEADBEEFDEADBEEF).all(), "a replay wrote outside the wire matrix"
        return rc, buf[guard:-guard].reshape(B, 135, n), out

    def free(self):
        if self.h:
            self.lib.mp2g_witness_program_free(self.h)
        self.h = None


def test_host_replay_reproduces_the_builder(mp2):
    ckt = extract_leaf(leaf_inputs(10))
    prog = mp2.WitnessProgram(ckt)
    ins = [leaf_inputs(11), leaf_inputs(12, 0), leaf_inputs(13, 7), [0] * 33, [255] * 32 + [5]]
    wires, pi_hash, pis = prog.run(np.array(ins, dtype=np.uint64))
    rows, _, _ = prog.run(np.array(ins, dtype=np.uint64), rows=True)
    for b, x in enumerate(ins):
        want = extract_leaf(x)
        assert np.array_equal(wires[b], want.wires) and np.array_equal(rows[b].T, want.wires)
        assert np.array_equal(pis[b], want.public_inputs) and np.array_equal(pi_hash[b], want.pi_hash)
        assert [int(v) for v in pis[b]] == R.column_realign_value(x[:32], x[32])
    prog.free()


def test_golden_lookup_tape(mp2):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "witness_tape_lookup_vectors.json")))["lookup_tape"]
    luts = [dict(t, table=np.array(t["table"], dtype=np.uint16)) for t in g["luts"]]
    p = Program(mp2, g["tape"], g["n_slots"], g["log_n"], len(g["input_sids"]))
    assert p.rc == 0 and p.set_lookups(luts) == 0
    rc, wires, probe = p.run([c["inputs"] for c in g["cases"]], g["probe_sids"])
    assert rc == 0
    for b, c in enumerate(g["cases"]):
        want = np.zeros((135, 1 << g["log_n"]), dtype=np.uint64)
        for col, row, v in c["cells"]:
            want[col, row] = v
        assert np.array_equal(wires[b], want) and probe[b].tolist() == c["probe"]
    p.free()


def small_luts(n_entries=30, first_lut_row=3):
    return [{"table": np.array([(v, (3 * v + 1) & 0xFF) for v in range(n_entries)], dtype=np.uint16), "last_lu_row": 1, "last_lut_row": 2,
             "first_lut_row": first_lut_row}]


def test_create_and_set_lookups_refuse_bad_programs(mp2):
    look = lambda row, i, lut, s=0, d=8: [LUT.OP_LOOKUP, row, i, lut, s, d]
    good = look(1, 0, 0) + look(1, 1, 0, 1, 9)

    def outcome(tape, luts):
        p = Program(mp2, tape)
        out = ("create",) if p.rc else ("set_lookups",) if p.set_lookups(luts) else ("ok",)
        p.free()
        return out[0]

    assert outcome(good, small_luts()) == "ok"
    assert outcome(look(1, 0, 1), small_luts()) == "set_lookups"             # table 1 of 1
    assert outcome(look(1, 0, 16), small_luts()) == "create"                  # table 16: beyond MP2G_MAX_LUTS
    assert outcome(look(1, 0, 1 << 40), small_luts()) == "create"
    assert outcome(look(1, 40, 0), small_luts()) == "create"                  # slot 40 of 40
    assert outcome(look(16, 0, 0), small_luts()) == "create"                  # row 16 of 16
    assert outcome(look(2, 0, 0), small_luts()) == "set_lookups"              # a LookupTableGate row
    assert outcome(look(0, 0, 0), small_luts()) == "set_lookups"              # the row before the table's rows
    assert outcome(look(1, 0, 0) + look(1, 0, 0, 1, 9), small_luts()) == "set_lookups"  # one slot twice
    assert outcome(look(1, 0, 0) + look(1, 2, 0, 1, 9), small_luts()) == "set_lookups"  # slot 1 left free
    assert outcome(look(1, 1, 0), small_luts()) == "set_lookups"              # slot 0 left free
    assert outcome(look(1, 0, 0, 0, 16), small_luts()) == "create"            # slot 16 of 16
    assert outcome(good[:-1], small_luts()) == "create"                       # truncated
    assert outcome([39, 0, 0, 0, 0, 0], small_luts()) == "create" and outcome([41, 0, 0, 0, 0, 0], small_luts()) == "create"
    twice = small_luts()
    twice[0]["table"][7, 0] = 3
    assert outcome(good, twice) == "set_lookups"                              # input 3 twice
    assert outcome(good, small_luts(30, 4)) == "set_lookups"                  # 3 LookupTableGate rows for 30 entries
    assert outcome(good, small_luts(27, 2)) == "set_lookups"                  # 1 row for 27 entries
    assert outcome(good, small_luts(26, 2)) == "ok"
    assert outcome(good, small_luts(30, 15)) == "set_lookups"                 # no row left after the table
    assert outcome(good, small_luts() + small_luts()) == "set_lookups"        # two tables in the same rows
    # a program with the opcode and no tables is refused at run; with them it runs
    p = Program(mp2, good)
    assert p.rc == 0
    rc, _, _ = p.run([[1, 2, 0, 0]])
    assert rc != 0 and "set_lookups" in mp2.load().mp2g_last_error().decode()
    assert p.set_lookups(small_luts()) == 0
    rc, wires, probe = p.run([[1, 2, 0, 0], [29, 30, 0, 0]], probe=[8, 9])
    assert rc == 0 and probe.tolist() == [[4, 7], [88, 0]]                    # 30 is not in the table: 0
    assert wires[0, :4, 1].tolist() == [1, 4, 2, 7] and wires[0, 4:6, 1].tolist() == [0, 1]  # the padding: the first pair
    assert wires[0, 2, 3] == 38 and wires[0, 5, 3] == 1 and wires[0, 8, 3] == 1  # multiplicities of entries 0 (the 38 padding slots), 1, 2
    assert wires[1, 2, 3] == 38 and wires[1, 3 * 3 + 2, 2] == 1 and int(wires[1, 2:78:3, 2:4].sum()) == 39  # (30, 0) counts for nothing
    p.free()


def test_random_lookup_tapes_are_refused_or_replayed_without_harm(mp2):
    """as tests/test_witness_tape.py's fuzzing, for the lookup block: whatever tape and table rows a caller hands over, the library
    refuses them or replays inside its buffers -- operands drawn around their limits and, now and then, huge"""
    rng = np.random.default_rng(0xC0FFEE08)
    n, n_slots = 16, 16

    def cnt(lo, hi):
        if rng.random() < 0.04:
            return [1 << 40, 1 << 63, (1 << 64) - 1][int(rng.integers(0, 3))]
        return int(rng.integers(lo, hi))

    ran = refused = 0
    for _ in range(400):
        n_luts = int(rng.integers(1, 3))
        luts, row = [], int(rng.integers(0, 3))
        for _ in range(n_luts):
            n_lu, ln = int(rng.integers(1, 3)), int(rng.integers(1, 60))
            n_lut = -(-ln // 26) + (1 if rng.random() < 0.1 else 0)
            tab = np.stack([rng.permutation(200)[:ln], rng.integers(0, 65536, ln)], axis=1).astype(np.uint16)
            if rng.random() < 0.05 and ln > 1:
                tab[0, 0] = tab[1, 0]
            luts.append({"table": tab, "last_lu_row": row, "last_lut_row": row + n_lu, "first_lut_row": row + n_lu + n_lut - 1})
            row += n_lu + n_lut + int(rng.integers(0, 2))
        tape = []
        for t, info in enumerate(luts):
            k = int(rng.integers(0, 6))
            for j in range(k):
                if rng.random() < 0.9:
                    r, i = info["last_lu_row"] + j // 40, j % 40
                else:
                    r, i = cnt(0, n + 1), cnt(0, 42)
                tape += [LUT.OP_LOOKUP, r, i, t if rng.random() < 0.95 else cnt(0, 18), int(rng.integers(0, n_slots + (1 if rng.random() < 0.03 else 0))),
                         int(rng.integers(4, n_slots))]
        if not tape:
            tape = [R.OP_WIRE, 0, 0, 0]
        p = Program(mp2, tape, n_slots)
        if p.rc or p.set_lookups(luts):
            refused += 1
            p.free()
            continue
        ins = rng.integers(0, 260, (2, 4)).astype(np.uint64)
        ins[0, 0] = [O.P - 1, 65536, 1 << 40][int(rng.integers(0, 3))]
        rc, wires, _ = p.run(ins)
        assert rc == 0
        ran += 1
        for b in range(2):  # the table rows are the tables, the multiplicities sum to at most the LookupGate slots
            for info in luts:
                top, tab = info["first_lut_row"], info["table"]
                got = np.stack([wires[b, 3 * (e % 26):3 * (e % 26) + 2, top - e // 26] for e in range(len(tab))])
                assert np.array_equal(got, tab.astype(np.uint64))
                assert int(wires[b, 2:78:3, info["last_lut_row"]:top + 1].sum()) <= 40 * (info["last_lut_row"] - info["last_lu_row"])
        p.free()
    assert ran >= 40 and refused >= 40, (ran, refused)


def test_an_input_outside_the_tables_replays_and_fails_the_lookup_argument(mp2):
    x = leaf_inputs(20)
    x[5] = 300
    ckt = extract_leaf(leaf_inputs(21))
    prog = mp2.WitnessProgram(ckt)
    wires, pi_hash, _ = prog.run(np.array([x], dtype=np.uint64))
    assert np.array_equal(wires[0], extract_leaf(x, strict=False).wires)
    fp = C.oracle_params(ckt, pow_bits=4, num_queries=3)
    cap, cd = verifier_data(ckt)
    caps, openings, proof, _ = C.prove_witness(ckt, fp, cd, wires[0], pi_hash[0])
    assert C.verify(ckt, fp, cd, pi_hash[0], caps, openings, proof) in (10, 11)
    prog.free()


# ---- 4. the in-circuit verifier ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_and_proof():
    base = extract_leaf(leaf_inputs(30))
    fp = C.oracle_params(base)
    cap, cd = verifier_data(base)
    caps, openings, proof, _ = C.prove(base, fp, cd)
    assert fp.num_lookup_polys == 7 and len(openings) == sum(fp.oracle_w[o] for o in range(4)) + 2 + 14
    assert C.verify(base, fp, cd, base.pi_hash, caps, openings, proof) == 0
    return base, fp, cap, cd, caps, openings, proof


def test_wrap_of_a_proof_with_lookup_tables(base_and_proof):
    base, fp, cap, cd, caps, openings, proof = base_and_proof
    inner = R.InnerCircuit(base, fp, cap, cd, len(base.public_inputs))
    assert len(inner.luts) == 14 and inner.num_lookup_selectors == 18
    # the strict builder accepts the honest proof: every lookup term is in vanishing(zeta) = Z_H(zeta) t(zeta), or this raises
    wrap = R.wrap_circuit(inner, caps, openings, proof, base.public_inputs)
    assert wrap.log_n == R.RECURSION_THRESHOLD and wrap.luts == []
    assert C.CONSTANT not in {g.kind for g in wrap.gates}  # the shape every wrapped circuit of a framework shares
    assert not C.eval_on_points(wrap, wrap.pre[:wrap.num_constants], wrap.wires).any()
    assert np.array_equal(wrap.public_inputs, base.public_inputs)
    wfp = C.oracle_params(wrap)
    wcap, wcd = verifier_data(wrap)
    wc, wo, wp, _ = C.prove(wrap, wfp, wcd)
    assert C.verify(wrap, wfp, wcd, wrap.pi_hash, wc, wo, wp) == 0
    # the same wrap circuit around another base proof
    base2 = extract_leaf(leaf_inputs(31))
    c2, o2, p2, _ = C.prove(base2, fp, cd)
    wrap2 = R.wrap_circuit(inner, c2, o2, p2, base2.public_inputs)
    assert np.array_equal(wrap2.pre, wrap.pre) and np.array_equal(wrap2.tape, wrap.tape)
    assert not C.eval_on_points(wrap2, wrap2.pre[:wrap2.num_constants], wrap2.wires).any()
    # and around the dummy proof the structure is built from
    inner_fw = R.InnerCircuit(base, FW.circuit_fri_params(base), cap, cd, len(base.public_inputs))  # the product's parameters: they know the proof's length
    dummy = R.wrap_circuit(inner_fw, *R.dummy_proof(inner_fw), strict=False)
    assert np.array_equal(dummy.pre, wrap.pre)


def test_wrap_rejects_a_bad_lookup_argument(base_and_proof):
    base, fp, cap, cd, caps, openings, proof = base_and_proof
    inner = R.InnerCircuit(base, fp, cap, cd, len(base.public_inputs))
    lookup_at_zeta = sum(fp.oracle_w[o] for o in range(4)) - 14
    for idx in (lookup_at_zeta + 2, len(openings) - 3):  # a lookup opening at zeta, one at g zeta
        bad = openings.copy()
        bad[idx, 0] = (int(bad[idx, 0]) + 1) % O.P
        with pytest.raises(AssertionError):
            R.wrap_circuit(inner, caps, bad, proof, base.public_inputs)
    # a base proof made from a witness with one wrong multiplicity
    w = base.wires.copy()
    r = base.luts[4]["first_lut_row"]
    w[2, r] = (int(w[2, r]) + 1) % O.P
    bc, bo, bp, _ = C.prove_witness(base, fp, cd, w, base.pi_hash)
    assert C.verify(base, fp, cd, base.pi_hash, bc, bo, bp) in (10, 11)
    with pytest.raises(AssertionError):
        R.wrap_circuit(inner, bc, bo, bp, base.public_inputs)
    wrap = R.wrap_circuit(inner, bc, bo, bp, base.public_inputs, strict=False)
    wfp = C.oracle_params(wrap, pow_bits=4, num_queries=2)
    wcap, wcd = verifier_data(wrap)
    wc, wo, wp, _ = C.prove(wrap, wfp, wcd)
    assert C.verify(wrap, wfp, wcd, wrap.pi_hash, wc, wo, wp) != 0


# ---- 5. the framework ----------------------------------------------------------------------------------------------------------------
def test_lookup_leaf_in_a_circuit_set():
    circs = framework_circuits()
    fw = R.RecursiveCircuits(circs, OracleProver(), FW.circuit_fri_params)
    assert {k: [c[0].log_n for c in v] for k, v in fw.chains.items()} == {"extract": [8, 12], "merge": [13, 12]}
    ins = [leaf_inputs(40), leaf_inputs(41)]
    p0 = fw.generate_proof("extract", [], [], ins[0])
    p1 = fw.generate_proof("extract", [], [], ins[1])
    b0, b1 = fw.generate_proofs_batch("extract", [([], [], ins[0]), ([], [], ins[1])])
    assert all(np.array_equal(x, y) for x, y in zip(b0, p0)) and all(np.array_equal(x, y) for x, y in zip(b1, p1))
    vals = [R.column_realign_value(x[:32], x[32]) for x in ins]
    assert [int(v) for v in p0[3][:8]] == vals[0] and [int(v) for v in p1[3][:8]] == vals[1]
    root = fw.generate_proof("merge", [p0, p1], ["extract", "extract"], None)
    assert [int(v) for v in root[3][:8]] == [a + b for a, b in zip(*vals)]
    assert np.array_equal(root[3][8:], np.asarray(fw.set_digest, dtype=np.uint64))
    wckt, wcap, wdig = fw.chains["merge"][-1]
    assert C.verify(wckt, C.oracle_params(wckt), wdig, O.hash_n_to_m_no_pad(root[3], 4), *root[:3]) == 0
    # the parameter file keeps the base circuit's tables: same proofs from the loaded set
    fw2 = R.RecursiveCircuits.from_bytes(fw.to_bytes(), circs, OracleProver(), FW.circuit_fri_params)
    l0, l2 = fw.chains["extract"][0][0].luts, fw2.chains["extract"][0][0].luts
    assert len(l2) == 14 and all(np.array_equal(a["table"], b["table"]) and {k: a[k] for k in a if k != "table"} == {k: b[k] for k in b if k != "table"}
                                 for a, b in zip(l0, l2))
    assert fw2.chains["extract"][0][0].num_lookup_polys == 7 and fw2.chains["merge"][0][0].luts == []
    (q0,) = fw2.generate_proofs_batch("extract", [([], [], ins[0])])
    assert all(np.array_equal(x, y) for x, y in zip(q0, p0))
    (r2,) = fw2.generate_proofs_batch("merge", [([p0, p1], ["extract", "extract"], None)])
    assert all(np.array_equal(x, y) for x, y in zip(r2, root))
