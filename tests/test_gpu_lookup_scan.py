"""The running sums of the lookup argument (csrc/lookup.hip: lookup_rows_kernel, lookup_scan_kernel) where a lane of the scan
folds more than one row: complete proofs of circuits whose table geometry puts the run boundaries of tests/edge_inputs.py
SCAN_CASES on the table's end, word for word against the oracle."""
import importlib

import numpy as np
import pytest

import circuits as C
import edge_inputs as E
import oracle as O

pytestmark = pytest.mark.gpu
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
FRI = dict(pow_bits=4, num_queries=3)


def prove_and_compare(ctx, mp2, ckt, wires, flags):
    """prove the batch `wires` [B][135][n] with the witness check on; every proof must be the oracle's proof of that witness;
    returns the oracle verifier's codes"""
    B = len(wires)
    cp = FW.CircuitProver(ctx, ckt, B, witness_check=True, **FRI)
    ofp = C.oracle_params(ckt, **FRI)
    assert bytes(ofp) == bytes(cp.fp)
    cp.prove(ctx.to_device(wires), ctx.to_device(np.stack([ckt.pi_hash] * B)))
    if any(flags):
        with pytest.raises(mp2.Mp2gError) as e:
            cp.pr.witness_status()
        assert e.value.flags.tolist() == flags
    else:
        assert cp.pr.witness_status().tolist() == flags
    caps, openings, proofs = cp.results()
    codes = []
    for b in range(B):
        oc, oo, op, _ = C.prove_witness(ckt, ofp, cp.circuit_digest, wires[b], ckt.pi_hash)
        assert np.array_equal(caps[b], oc), b
        assert np.array_equal(openings[b], oo), b
        assert np.array_equal(proofs[b], op), b
        codes.append(C.verify(ckt, ofp, cp.circuit_digest, ckt.pi_hash, caps[b], openings[b], proofs[b]))
    cp.free()
    return codes


@pytest.mark.parametrize("L,k,log_n,total,lut_rows", E.SCAN_CASES)
def test_running_sums_match_oracle(ctx, mp2, L, k, log_n, total, lut_rows):
    ckt = C.build(log_n, C.ALL_KINDS + C.LOOKUP_KINDS, 5, luts=[(E.scan_table(L), k)])
    assert E.scan_rows(ckt.luts[0]) == (total, lut_rows)
    assert prove_and_compare(ctx, mp2, ckt, np.stack([ckt.wires] * 2), [0, 0]) == [0, 0]


def test_two_tables_of_unequal_size(ctx, mp2):
    """lookup_rows_kernel's grid is sized by the larger table: the one-entry table's surplus blocks and lanes write nothing"""
    ckt = C.build(8, C.ALL_KINDS + C.LOOKUP_KINDS, 5, luts=[(E.scan_table(1638), 80), (E.scan_table(1), 3)])
    assert [E.scan_rows(t) for t in ckt.luts] == [(65, 63), (2, 1)]
    assert prove_and_compare(ctx, mp2, ckt, np.stack([ckt.wires] * 2), [0, 0]) == [0, 0]


def test_wrong_multiplicity_in_the_middle_of_a_run(ctx, mp2):
    """65 rows, two per lane: proof 1 has one multiplicity changed in a LookupTable row that is the second row of lane 10's run.
    The sums no longer close (flag 4), and the proof is still the oracle's proof of that witness."""
    L, k, log_n, total, lut_rows = E.SCAN_CASES[1]
    ckt = C.build(log_n, C.ALL_KINDS + C.LOOKUP_KINDS, 5, luts=[(E.scan_table(L), k)])
    assert E.scan_rows(ckt.luts[0]) == (total, lut_rows)
    t0, t1 = E.scan_runs(total)[10]
    assert t1 - t0 == 2 and t1 - 1 < lut_rows
    row = ckt.luts[0]["first_lut_row"] - (t1 - 1)
    wires = np.stack([ckt.wires] * 2)
    wires[1, 3 * 7 + 2, row] = (int(wires[1, 3 * 7 + 2, row]) + 1) % O.P  # slot 7's multiplicity
    codes = prove_and_compare(ctx, mp2, ckt, wires, [0, 4])
    assert codes[0] == 0 and codes[1] != 0
