"""Edge-valued witnesses through the whole prover. The LDE of a random witness looks uniform at every point, whatever the
witness is; a constant column takes its edge value at EVERY LDE point, so these witnesses put 0, 1, p - 1 and the other lattice
values of tests/field_cases.py into quotient_perm_kernel, quotient_lookup_kernel, the gate LDE kernels and lookup_rows_kernel,
and single-coefficient polynomials into openings_kernel and compose_kernel. None of them satisfies the circuit; the oracle proves
any witness, and every proof must be the oracle's, word for word."""
import importlib

import numpy as np
import pytest

import circuits as C
import edge_inputs as E
import oracle as O

pytestmark = pytest.mark.gpu
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
FRI = dict(pow_bits=4, num_queries=3)


def edge_witnesses(ckt, seed):
    """[(name, wires [135][n])]: three draws of constant columns, all cells lattice-random, all zero, all p - 1, the circuit's own"""
    n = 1 << ckt.log_n
    ws = [("constant%d" % k, np.repeat(E.edge_rows((C.NUM_WIRES, 1), seed + k), n, axis=1)) for k in range(3)]
    ws += [("lattice", E.edge_rows((C.NUM_WIRES, n), seed + 3)), ("zero", np.zeros((C.NUM_WIRES, n), dtype=np.uint64)),
           ("p-1", np.full((C.NUM_WIRES, n), O.P - 1, dtype=np.uint64)), ("satisfying", ckt.wires)]
    return ws


def circuit(which):
    if which == "lookup7":
        return C.build(7, C.ALL_KINDS + C.LOOKUP_KINDS, 3, luts=[(t, 100) for t in C.bits_lookup_tables()])
    return C.build(which, C.ALL_KINDS, 3)


@pytest.mark.parametrize("which,variant", [(5, 0), (5, 1), (6, 0), ("lookup7", 0)])
def test_edge_witnesses_prove_as_the_oracle_does(ctx, mp2, which, variant):
    ckt = circuit(which)
    ws = edge_witnesses(ckt, 40 + ckt.log_n)
    B = len(ws)
    cp = FW.CircuitProver(ctx, ckt, B, variant, **FRI)
    ofp = C.oracle_params(ckt, variant, **FRI)
    assert bytes(ofp) == bytes(cp.fp)
    cp.prove(ctx.to_device(np.stack([w for _, w in ws])), ctx.to_device(np.stack([ckt.pi_hash] * B)))
    caps, openings, proofs = cp.results()
    for b, (name, w) in enumerate(ws):
        oc, oo, op, _ = C.prove_witness(ckt, ofp, cp.circuit_digest, w, ckt.pi_hash)
        assert np.array_equal(caps[b], oc), name
        assert np.array_equal(openings[b], oo), name
        assert np.array_equal(proofs[b], op), name
        code = C.verify(ckt, ofp, cp.circuit_digest, ckt.pi_hash, caps[b], openings[b], proofs[b])
        assert (code == 0) == (name == "satisfying"), (name, code)
    cp.free()
