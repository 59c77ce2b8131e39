"""csrc/witness_ops.h op_shape compiled for the host (tools/hosttest/witness_shape_test.cpp) against recursion.py's table of the same
facts (_OPS, through tape_instructions and instruction_slots): for every instruction of the golden tapes, of a wrap circuit's tape,
of a circuit over the Poseidon config, of the GF(p^5) hint circuit and of a hash-limb split the two give the same length, the same run
of slots read and the same run of slots written (and the slot operands start where op_shape's first_slot says) -- and the tapes together hold every one of the 25 opcodes, so none agrees by being absent."""
import importlib
import json
import os
import subprocess

import pytest

import hosttest
import oracle as O
from test_recursion import verifier_data
from test_witness_tape import leaf_logic_circuit, leaf_logic_inputs
from test_witness_tape_gf5 import gf5_hint_circuit, hint_inputs

R = importlib.import_module("mapreduce-plonky2_amd.recursion")
GF5 = importlib.import_module("mapreduce-plonky2_amd.gf5")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
ALL_OPCODES = set(range(1, 24)) | {32, 33}  # include/mp2g.h: enum mp2g_witness_op without its END, enum mp2g_witness_op_gf5 likewise


@pytest.fixture(scope="module")
def shape_test(tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("witness_shape"), "witness_shape_test")


def tapes():
    golden = json.load(open(os.path.join(O.ROOT, "tests", "golden", "witness_tape_vectors.json")))
    for name in ("c_witness_tape_demo", "leaf_gate_opcodes"):
        yield name, golden[name]["tape"]
    yield "gf5 golden", json.load(open(os.path.join(O.ROOT, "tests", "golden", "witness_tape_gf5_vectors.json")))["gf5_hints"]["tape"]
    base = R.map_circuit(O.rand_field(4, 77))
    cap, cd = verifier_data(base)
    inner = R.InnerCircuit(base, FW.circuit_fri_params(base), cap, cd, len(base.public_inputs))
    yield "wrap circuit", R.wrap_circuit(inner, *R.dummy_proof(inner), strict=False).tape  # the tape does not depend on the proof's values
    yield "map circuit, Poseidon config", R.map_circuit(O.rand_field(4, 78), R.Builder(hasher=1)).tape
    yield "leaf gates", leaf_logic_circuit(leaf_logic_inputs(1)).tape
    yield "gf5 hints", gf5_hint_circuit(*hint_inputs(0x5E1, 1)[0]).tape
    b = R.Builder()  # the one opcode none of the above records: the split hint of the hash-limb flattening
    b.register_public_inputs(list(R.split_hash_element_to_low_high(b, b.add_virtual(0x123456789ABCDEF))))
    yield "split hint", b.build().tape


def test_python_table_and_op_shape_agree(shape_test):
    seen = set()
    for name, tape in tapes():
        tape = [int(w) for w in tape]
        r = subprocess.run([shape_test], input=" ".join(str(w) for w in tape), capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stdout[-200:] + r.stderr
        native = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        mine = list(R.tape_instructions(tape)) + [(len(tape), None)]
        assert [(pos, op) for pos, op, *_ in native] == mine[:-1], name
        for (pos, op, ln, first_slot, r0, nr, w0, nw), (nxt, _) in zip(native, mine[1:]):
            seen.add(op)
            assert nxt == pos + 1 + ln, (name, pos, op)
            if op == R.OP_PAR:  # a header only: the sections are instructions of their own
                assert (first_slot, r0, nr, w0, nw) == (0, 0, 0, 0, 0) and ln == 1 + tape[pos + 1]
                continue
            # the slot operands (bounds-checked at create) start where the reads do; the split hint's source slot sits before its bit
            # position, which is no slot: it is checked apart and the slots start at the two it writes
            assert first_slot == (w0 if op == R.OP_HINT_SPLIT else r0), (name, pos, op)
            rd, wr, _, after = R.instruction_slots(tape, pos)
            t = tape[pos + 1:]
            assert after == nxt and list(rd) == t[r0:r0 + nr] and list(wr) == t[w0:w0 + nw], (name, pos, op)
    assert seen == ALL_OPCODES, sorted(ALL_OPCODES - seen)


def test_op_shape_refuses_what_is_no_instruction(shape_test):
    """unknown opcodes, counts outside their ranges (huge ones included), instructions cut short"""
    ok = [R.OP_U32_ADD_MANY, 2, 4, 5, 3, 0, 1, 2, 3, 10, 11]
    assert subprocess.run([shape_test], input=" ".join(map(str, ok)), capture_output=True, text=True).returncode == 0
    for bad in ([0], [24, 0, 0], [31], [34], [1 << 40], ok[:-1], ok[:4], [R.OP_U32_ADD_MANY, 2, 4, 5, 17] + [0] * 20,
                [R.OP_U32_ADD_MANY, 2, 4, 5, 1 << 63] + [0] * 20, [R.OP_COSET, 0, 1] + [0] * 80, [R.OP_COSET, 0, 6] + [0] * 200,
                [R.OP_COSET, 0, (1 << 64) - 1] + [0] * 80, [R.OP_BASE_SPLIT, 0, 2, 64] + [0] * 70, [R.OP_BASE_SPLIT, 0, 2, 1 << 40] + [0] * 70,
                [R.OP_EXP, 0, 0, 1, 2], [R.OP_EXP, 0, 67] + [0] * 70, [R.OP_PAR, 4097] + [0] * 5000, [R.OP_PAR], [GF5.OP_QUINTIC_SQRT] + [0] * 10):
        r = subprocess.run([shape_test], input=" ".join(map(str, bad)), capture_output=True, text=True)
        assert r.returncode == 1 and "malformed" in r.stdout, bad
