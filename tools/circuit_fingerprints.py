#!/usr/bin/env python3
"""Generate tests/golden/circuit_fingerprints.json: a SHA-256 per field of a fixed list of built circuits, so that a change to
the Python front end (circuits.py, recursion.py's Builder and verifier gadgets, the parameter-file round trip) that moves a
circuit -- a selector, a sigma, a gate constant, a tape word -- is caught field by field (tests/test_circuit_fingerprints.py).

The committed file was made at the commit BEFORE the front-end refactor that introduced it and is compared unchanged after it.
Run this tool again only when a pull request MEANS to change a circuit, and say so there: every params file and every circuit
digest made before then stops matching.

Per circuit, every instance field is written as sha256(shape string + the field's bytes as a contiguous uint64 array); gates as
rows [kind, p0, p1, p2, selector_index, group_start, group_end]; each lookup table by the keys table, n_lookups, last_lu_row,
last_lut_row, first_lut_row only (the multiplicity scratch list circuits.fill_lookup_row leaves in the dict is not part of a
circuit); None as the string "None". gate_array (a ctypes copy of gates) and _prover_key (a cache) are skipped."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import circuits as C  # noqa: E402
import oracle as O  # noqa: E402

R = importlib.import_module("mapreduce-plonky2_amd.recursion")

GOLDEN = os.path.join(ROOT, "tests", "golden", "circuit_fingerprints.json")
SKIPPED = ("gate_array", "_prover_key")
LUT_KEYS = ("table", "n_lookups", "last_lu_row", "last_lut_row", "first_lut_row")
FRAMEWORK_SEED = 0xC0FFEE03  # framework.FrameworkProver: base circuit seed + base_bits, wrap circuit seed + wrap_bits + 100


def _sha(parts):
    h = hashlib.sha256()
    for a in parts:
        a = np.ascontiguousarray(np.asarray(a).astype(np.uint64))
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def field_fingerprint(name, v):
    if v is None:
        return "None"
    if name == "gates":
        return _sha([np.array([[g.kind, g.p0, g.p1, g.p2, g.selector_index, g.group_start, g.group_end] for g in v]).reshape(-1, 7)])
    if name == "luts":
        return _sha([len(v)] + [t[k] for t in v for k in LUT_KEYS])
    return _sha([v])


def fingerprint(ckt):
    """{field: digest} over the circuit's instance fields"""
    return {k: field_fingerprint(k, v) for k, v in sorted(vars(ckt).items()) if k not in SKIPPED}


def leaf_circuit():
    fc = R.FrameworkCircuit("leaf", 0, R.column_realign_logic, 8, min_log_n=8, extra_gates=C.LEAF_KINDS)
    return fc.build_base(None, [], [], [], list(range(32)) + [3], [1, 2, 3, 4])


def leaf_round_trip():
    out = {}
    R.circuit_to_arrays(leaf_circuit(), "leaf/", out)
    return R.circuit_from_arrays(out, "leaf/")


def map_wrap_circuit():
    """the wrap circuit of the map proof, made as tests/test_recursion.py base_and_proof makes it (the oracle's prove() is deterministic)"""
    base = R.map_circuit(O.rand_field(4, 77))
    fp = C.oracle_params(base)
    cap = O.merkle_cap(O.merkle_build(O.lde_leaves(O.fft(base.pre, inverse=True), 3), 4), 4)
    dom = O.hash_n_to_m_no_pad([1, 0, 0, 0, 0, 0, 0, 1], 4)
    cd = O.hash_n_to_m_no_pad(list(cap.reshape(-1)) + list(dom) + [base.log_n], 4)
    caps, openings, proof, _ = C.prove(base, fp, cd)
    return R.wrap_circuit(R.InnerCircuit(base, fp, cap, cd, len(base.public_inputs)), caps, openings, proof, base.public_inputs)


def poseidon_builder_circuit():
    """PoseidonGate public-input rows and a non-empty domain separator"""
    b = R.Builder(hasher=1)
    b.set_domain_separator([5, 6])
    x, y = b.add_virtual(11), b.add_virtual(13)
    b.register_public_inputs([b.mul(x, y), b.add(x, y)])
    return b.build()


def _luts():
    return [(t, 5) for t in C.bits_lookup_tables()]


# name -> constructor. EXTRACTION_KINDS holds no NoopGate of its own (a lookup table ends with one): it is built on the leaf set,
# as everywhere else in the tests.
CIRCUITS = {
    "build(5, ALL_KINDS, 1)": lambda: C.build(5, C.ALL_KINDS, 1),
    "build(7, ALL_KINDS, 3)": lambda: C.build(7, C.ALL_KINDS, 3),
    "build(7, VERIFIER_KINDS + LOOKUP_KINDS, 3, luts)": lambda: C.build(7, C.VERIFIER_KINDS + C.LOOKUP_KINDS, 3, luts=_luts()),
    "build(7, LEAF_KINDS + EXTRACTION_KINDS, 3, luts)": lambda: C.build(7, C.LEAF_KINDS + C.EXTRACTION_KINDS, 3, luts=_luts()),
    "build(12, VERIFIER_KINDS, framework wrap seed)": lambda: C.build(12, C.VERIFIER_KINDS, FRAMEWORK_SEED + 12 + 100),
    "build(13, LEAF_KINDS, framework base seed)": lambda: C.build(13, C.LEAF_KINDS, FRAMEWORK_SEED + 13),
    "dummy_circuit(6, 9)": lambda: R.dummy_circuit(6, 9),
    "map_circuit(rand_field(4, 77))": lambda: R.map_circuit(O.rand_field(4, 77)),
    "leaf": leaf_circuit,
    "leaf through circuit_to_arrays / circuit_from_arrays": leaf_round_trip,
    "wrap of the map proof": map_wrap_circuit,
    "Builder(hasher=1), domain separator, two public inputs": poseidon_builder_circuit,
}


def fingerprints():
    return {name: fingerprint(make()) for name, make in CIRCUITS.items()}


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(fingerprints(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
