"""The circuits the front end builds did not move: tests/golden/circuit_fingerprints.json holds a SHA-256 per field of a fixed list
of circuits (tools/circuit_fingerprints.py: the random circuits of circuits.build with and without lookup tables, the framework's
bench circuits, Builder circuits with tapes, lookup tables, generated gate rows, a Poseidon public-input hash and a domain
separator, a wrap circuit, a parameter-file round trip), taken at the commit before the front-end refactor. Every field of every
circuit is recomputed here and compared. No GPU: the library is loaded for its host-side parameter helpers only."""
import importlib.util
import json
import os

import pytest

import circuits as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("circuit_fingerprints", os.path.join(ROOT, "tools", "circuit_fingerprints.py"))
FP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FP)

with open(FP.GOLDEN) as _f:
    GOLDEN = json.load(_f)

def test_the_golden_file_lists_the_tools_circuits():
    assert sorted(GOLDEN) == sorted(FP.CIRCUITS)


@pytest.mark.parametrize("name", sorted(FP.CIRCUITS))
def test_circuit_fingerprint(name):
    got, want = FP.fingerprint(FP.CIRCUITS[name]()), GOLDEN[name]
    moved = sorted(k for k in want if got.get(k) != want[k])
    assert not moved, f"{name}: {moved} differ from the golden file"
    # a field the circuit did not have when the golden file was made is a declared field at its neutral value
    neutral = FP.fingerprint(C.Circuit())
    extra = sorted(k for k in got if k not in want and got[k] != neutral[k])
    assert not extra, f"{name}: {extra} are set, and the golden file has no such field"


def test_a_parameter_file_circuit_differs_in_its_witness_only():
    """circuit_from_arrays gives the circuit back without its wire matrix (a parameter file holds circuits, not witnesses)"""
    a, b = FP.fingerprint(FP.leaf_circuit()), FP.fingerprint(FP.leaf_round_trip())
    assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == ["wires"] and b["wires"] == "None"
