"""The witness tape's GF(p^5) opcodes on the GPU: the device replay (mp2g_witness_program_run_dev, the kernel instance with the GF(p^5)
code) against the host replay, the builder and the golden tape; and proofs of a circuit whose hints are constrained in-circuit by
arithmetic gates (root^2 = x, q b = a), with the witness check on, verified by the oracle -- a proof whose x has no square root
fails the check alone."""
import importlib
import json

import numpy as np
import pytest

import circuits as C
from test_witness_tape_gf5 import GOLDEN, _golden_program, check_hint_values, fnv, gf5_hint_circuit, hint_inputs, rand_elem

pytestmark = pytest.mark.gpu
R = importlib.import_module("mapreduce-plonky2_amd.recursion")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
GF5 = importlib.import_module("mapreduce-plonky2_amd.gf5")


def run_dev(ctx, prog, log_n, a):
    B, n = a.shape[0], 1 << log_n
    d_in, d_w, d_pr = ctx.to_device(a), ctx.alloc(B * 135 * n * 8), ctx.alloc(B * prog.probe.size * 8)
    prog.run_dev(ctx, d_in, B, d_w, d_pr)
    return d_w, d_pr, d_w.download((B, 135, n)), d_pr.download((B, prog.probe.size))


def test_device_replay_of_the_gf5_opcodes(ctx, mp2):
    """a batch of 16 (squares and non-squares, x = 0, b = 0, a = 0): the device replay equals the host replay and the builder word for
    word, wires and probe"""
    ins = hint_inputs(0x6E1, 16)
    ckts = [gf5_hint_circuit(*v) for v in ins]
    ck = ckts[0]
    prog = mp2.WitnessProgram(ck)
    a = np.array([[w for e in v for w in e] for v in ins], dtype=np.uint64)
    want_w, want_h, want_pi = prog.run(a)
    _, _, got_w, got_pr = run_dev(ctx, prog, ck.log_n, a)
    for k, c in enumerate(ckts):
        assert np.array_equal(got_w[k], c.wires), f"device replay != builder (proof {k})"
        pi = [int(v) for v in got_pr[k, 4:]]
        check_hint_values(ins[k][0], ins[k][1], ins[k][2], pi[0:5], pi[5], pi[6:11])
    assert np.array_equal(got_w, want_w) and np.array_equal(got_pr[:, :4], want_h) and np.array_equal(got_pr[:, 4:], want_pi)
    assert 0 < int(got_pr[:, 4 + 5].sum()) < len(ins)
    prog.free()


def test_device_replay_reproduces_the_golden_gf5_tape(ctx, mp2):
    g = json.load(open(GOLDEN))["gf5_hints"]
    prog = mp2.WitnessProgram(_golden_program(g))
    a = np.array([c["inputs"] for c in g["cases"]], dtype=np.uint64)
    _, _, got_w, got_pr = run_dev(ctx, prog, g["log_n"], a)
    for k, c in enumerate(g["cases"]):
        assert fnv(got_w[k]) == c["wires_fnv1a"] and [int(v) for v in got_pr[k]] == c["probe"]
    prog.free()


def gf5_mul_gates(b, x, y):
    """x y in GF(p^5) = GF(p)[z] / (z^5 - 3) by ArithmeticGate operations: out_k = sum_{i + j = k} x_i y_j + 3 sum_{i + j = k + 5} x_i y_j"""
    out = []
    for k in range(5):
        acc = None
        for i in range(5):
            j = (k - i) % 5
            c = 1 if i + j < 5 else 3
            acc = b.arithmetic(c, x[i], y[j], 0, x[i]) if acc is None else b.arithmetic(c, x[i], y[j], 1, acc)
        out.append(acc)
    return out


def constrained_hint_circuit(x, a, b):
    """(root, is_sqrt) = quintic_sqrt(x), q = quintic_quotient(a, b), constrained by root^2 = x (unconditionally) and q b = a;
    public inputs root, is_sqrt, q, x, a (which also gives x and a the wires that the products are copy-constrained to)"""
    bl = R.Builder()
    tx, ta, tb = ([bl.add_virtual(int(v)) for v in e] for e in (x, a, b))
    root, is_sqrt = bl.quintic_sqrt(tx)
    q = bl.quintic_quotient(ta, tb)
    for got, want in zip(gf5_mul_gates(bl, root, root), tx):
        bl.connect(got, want)
    for got, want in zip(gf5_mul_gates(bl, q, tb), ta):
        bl.connect(got, want)
    bl.register_public_inputs(root + [is_sqrt] + q + tx + ta)
    return bl.build()


def constrained_inputs(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        y = rand_elem(rng)
        out.append((GF5.mul(y, y), rand_elem(rng), rand_elem(rng)))
    return out


def test_constrained_gf5_hints_prove_and_verify(ctx, mp2):
    """the hints feed arithmetic gates that constrain them: the device-replayed witnesses pass prove()'s witness check, the oracle
    verifies every proof, and a proof equals the oracle's proof of the same witness"""
    ins = constrained_inputs(0x6E2, 4)
    ckts = [constrained_hint_circuit(*v) for v in ins]
    ck = ckts[0]
    prog = mp2.WitnessProgram(ck)
    a = np.array([[w for e in v for w in e] for v in ins], dtype=np.uint64)
    d_w, d_pr, got_w, got_pr = run_dev(ctx, prog, ck.log_n, a)
    B = len(ins)
    for k, c in enumerate(ckts):
        assert np.array_equal(got_w[k], c.wires) and np.array_equal(got_pr[k, 4:], c.public_inputs)
        assert not C.eval_on_points(c, c.pre[:c.num_constants], got_w[k]).any()
    cp = FW.CircuitProver(ctx, ck, B, witness_check=True, pow_bits=8, num_queries=6)
    cp.prove(d_w, ctx.to_device(np.ascontiguousarray(got_pr[:, :4])))
    assert cp.pr.witness_status().tolist() == [0] * B
    caps, openings, proofs = cp.results()
    fp = C.oracle_params(ck, pow_bits=8, num_queries=6)
    for k in range(B):
        assert C.verify(ck, fp, cp.circuit_digest, got_pr[k, :4], caps[k], openings[k], proofs[k]) == 0, f"the oracle rejects proof {k}"
    oc, oo, op, _ = C.prove_witness(ck, fp, cp.circuit_digest, got_w[0], got_pr[0, :4])
    assert np.array_equal(caps[0], oc) and np.array_equal(openings[0], oo) and np.array_equal(proofs[0], op), "GPU proof != the oracle's proof of the same witness"
    cp.free()
    prog.free()


def test_a_non_square_fails_only_its_own_proof(ctx, mp2):
    """one x of the batch has no square root: its replay writes root = 0, is_sqrt = 0 (the replay itself succeeds), root^2 = x fails
    in that proof's witness check, and only there"""
    ins = constrained_inputs(0x6E3, 4)
    ck = constrained_hint_circuit(*ins[0])
    rng = np.random.default_rng(0x6E4)
    while True:
        ns = rand_elem(rng)
        if GF5.sqrt(ns) is None:
            break
    ins[2] = (ns, ins[2][1], ins[2][2])
    prog = mp2.WitnessProgram(ck)
    a = np.array([[w for e in v for w in e] for v in ins], dtype=np.uint64)
    d_w, d_pr, got_w, got_pr = run_dev(ctx, prog, ck.log_n, a)
    assert [int(v) for v in got_pr[2, 4:10]] == [0] * 6 and [int(got_pr[k, 4 + 5]) for k in (0, 1, 3)] == [1, 1, 1]
    cp = FW.CircuitProver(ctx, ck, len(ins), witness_check=True, pow_bits=8, num_queries=6)
    cp.prove(d_w, ctx.to_device(np.ascontiguousarray(got_pr[:, :4])))
    with pytest.raises(mp2.Mp2gError) as ei:
        cp.pr.witness_status()
    assert ei.value.flags[2] != 0 and [int(ei.value.flags[k]) for k in (0, 1, 3)] == [0, 0, 0]
    cp.free()
    prog.free()
