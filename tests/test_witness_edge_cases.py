"""The circuits and vectors of tests/witness_edge_cases.py on the CPU: the opcode circuit holds every base opcode, the vectors are
canonical and hold every corner of the opcodes (asserted from the inputs alone), a family records one tape, the level shapes are
the ones the device's level loop branches on, and the host replay (mp2g_witness_program_run) equals the builder's Python integers on
every vector of every family. The device replay of the same families is tests/test_gpu_witness_replay_edges.py."""
import importlib

import numpy as np
import pytest

import circuits as C
import witness_edge_cases as E

R = importlib.import_module("mapreduce-plonky2_amd.recursion")
MP2 = importlib.import_module("mapreduce-plonky2_amd")
P = E.P


def test_the_opcode_circuit_holds_every_base_opcode():
    ck = E.family("opcodes")[1][0]
    ops = {op for _, op in R.tape_instructions(ck.tape)}
    assert R.OP_EXP + 1 == 24  # MP2G_OP_END
    assert set(range(1, 24)) <= ops, sorted(set(range(1, 24)) - ops)
    kinds = {(g.kind, g.p0, g.p1) for g in ck.gates}
    assert {(C.COMPARISON, 63, 16), (C.COMPARISON, 32, 16), (C.COMPARISON, 63, 1), (C.U32_ADD_MANY, 16, 1), (C.EXPONENTIATION, 66, 0),
            (C.BASE_SUM, 31, 4), (C.BASE_SUM, 63, 2), (C.COSET_INTERPOLATION, 4, C.coset_interpolation_degree(4))} <= kinds
    assert sum(op == R.OP_REDUCING for _, op in R.tape_instructions(ck.tape)) == 2  # 44 terms: the second row starts from the first's sum
    assert sum(op == R.OP_REDUCING_EXT for _, op in R.tape_instructions(ck.tape)) == 2
    assert ck.log_n <= 9


def test_the_vectors_are_canonical_and_hold_every_corner():
    vs = E.opcode_vectors()
    assert len(vs) >= 24 and all(len(v) == E.OPCODE_WORDS and all(0 <= x < P for x in v) for v in vs)
    for fill in (0, 1, P - 1, 0xFFFFFFFF):
        assert [fill] * E.OPCODE_WORDS in vs
    lattice = [v for v in vs if set(v) <= set(E.EC) and len(set(v)) > 1]
    assert len(lattice) >= 16
    fs = [E.fields(v) for v in vs]
    for name, holds in E.CORNERS.items():
        assert any(holds(f) for f in fs), f"no vector has: {name}"
    # the domain vector: every gate's precondition
    d = fs[E.DOMAIN_VECTOR]
    assert all(x < 1 << 32 for k in ("u32_arith", "u32_sub", "add_many", "range_check", "cmp32", "cmp_same") for x in d[k])
    assert all(x < 1 << 63 for k in ("bits63", "cmp63", "cmp1") for x in d[k]) and d["base4"][0] < 1 << 62 and d["ra_index"][0] < 16
    assert set(d["exp_bits"]) == {0, 1} and d["swap"] == d["pswap"] == [1] and d["u32_sub"][2] in (0, 1)
    assert d["div_den"] != [0, 0] and d["coset_shift"] != [0]
    for vs, words in ((E.p2_vectors(), E.P2_WORDS), (E.chain_vectors(), E.CHAIN_WORDS)):
        assert len(vs) <= 48 and all(len(v) == words and all(0 <= x < P for x in v) for v in vs)
    # every state of twelve equal lattice words stands in some Poseidon2 vector, with a swap of 0
    equal = {v[0] for v in E.p2_vectors() if len(set(v[:12])) == 1 and v[24] == 0} | {v[12] for v in E.p2_vectors() if len(set(v[12:24])) == 1 and v[25] == 0}
    assert set(E.EC) <= equal


@pytest.mark.parametrize("name", E.FAMILIES)
def test_a_family_records_one_tape(name):
    a, ckts = E.family(name)
    assert a.shape[0] == len(ckts) <= 48 and all(c.log_n <= 9 for c in ckts)
    for k, c in enumerate(ckts):
        assert np.array_equal(c.tape, ckts[0].tape) and np.array_equal(c.pre, ckts[0].pre), f"vector {k} changes the structure"
        assert np.array_equal(c.input_values, a[k])
    assert len({c.wires.tobytes() for c in ckts}) == len(ckts)


@pytest.mark.parametrize("name,rows,op", [("p2_coop", 8, R.OP_P2), ("p2_lanes", 65, R.OP_P2), ("poseidon", 8, R.OP_POSEIDON)])
def test_the_gate_path_circuits_put_their_rows_on_level_one(name, rows, op):
    """8 rows: 8 x 16 lanes fit the block twice over, the cooperative body runs; 65 rows: 65 x 16 > 2 x 512, one lane per row"""
    ck = E.family(name)[1][0]
    levels = E.levels_by_opcode(ck.tape)
    assert levels[1].get(op, 0) == rows and set(levels[1]) <= {op, R.OP_WIRE}
    first = [pos for pos, o, l in E.level_schedule(ck.tape) if o == op and l == 1]
    ins = set(int(s) for s in ck.input_sids)
    assert all(set(int(s) for s in R.instruction_slots(ck.tape, pos)[0]) <= ins for pos in first)  # raw input words only
    assert E.p2_gate_rows(ck, op)[:rows] == list(range(rows))


@pytest.mark.parametrize("instance", E.INSTANCES)
def test_the_chain_circuit_reaches_every_branch_of_the_level_loop(instance):
    """witness_dev.hip's level loop: 1..64 Poseidon2 rows on a level take the cooperative body, 33..64 a second round of groups, 65
    one lane per row; the other instructions are renumbered around the Poseidon2 run, so every level has some on both sides of it in
    opcode order; more than 512 of them make lanes take a second one"""
    ck = E.family("chain_" + instance)[1][0]
    prog = MP2.WitnessProgram(ck)
    assert prog.n_levels == E.check_chain_shape(ck, instance) == len(E.CHAIN_P2) + 2
    prog.free()


@pytest.mark.parametrize("name", E.FAMILIES)
def test_host_replay_equals_the_builder(name):
    a, ckts = E.family(name)
    prog = MP2.WitnessProgram(ckts[0])
    wires, pi_hash, pis = prog.run(a)
    prog.free()
    for k, c in enumerate(ckts):
        assert np.array_equal(wires[k], c.wires), f"host replay != builder (vector {k}): {E.mismatch(wires[k], c.wires)}"
        assert np.array_equal(pi_hash[k], c.pi_hash) and np.array_equal(pis[k], c.public_inputs), k
    if name == "opcodes":
        d = E.DOMAIN_VECTOR
        assert E.gate_constraints_hold(ckts[d], wires[d], C.eval_on_points), "a gate constraint does not vanish on the domain vector's wires"
        bad = wires[d].copy()
        row = next(r for r, i in enumerate(ckts[d].instances) if ckts[d].gates[i].kind == C.COMPARISON and ckts[d].gates[i].p1 == 1)
        bad[3, row] ^= np.uint64(1)  # the most significant difference of the one-chunk comparison
        assert not E.gate_constraints_hold(ckts[d], bad, C.eval_on_points)
        assert not E.gate_constraints_hold(ckts[d], wires[0], C.eval_on_points)  # another vector's wires under this one's public-inputs hash
    if name in E.P2_ROWS:
        E.check_permutations(name, a, ckts[0], wires)


def test_comparison_row_holds_agrees_with_the_oracle_evaluator():
    """the restated ComparisonGate constraints on a gate the evaluator can run: they accept the builder's row and refuse what the
    evaluator refuses, wire by wire"""
    b = R.Builder(strict=False)
    b.register_public_inputs([b.comparison_le(b.add_virtual(0x12345678), b.add_virtual(0x12345679), 32, 16)])
    ck = b.build()
    row = next(r for r, i in enumerate(ck.instances) if ck.gates[i].kind == C.COMPARISON)
    consts = ck.pre[:ck.num_constants]
    assert E.comparison_row_holds(ck.wires[:, row], 32, 16) and not C.eval_on_points(ck, consts, ck.wires).any()
    free = [4 + 2 * 16 + i for i in range(1, 16)]  # the equality dummies of equal chunks (the operands differ in chunk 0 only)
    for col in range(4 + 5 * 16 + 3):
        w = ck.wires.copy()
        w[col, row] = (int(w[col, row]) + 1) % P
        refused = bool(C.eval_on_points(ck, consts, w).any())
        assert refused == (col not in free) and E.comparison_row_holds(w[:, row], 32, 16) == (not refused), col
