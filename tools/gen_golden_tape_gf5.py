#!/usr/bin/env python3
"""Generate tests/golden/witness_tape_gf5_vectors.json: the witness tape's GF(p^5) opcodes (include/mp2g.h enum mp2g_witness_op_gf5)
frozen as data, next to tools/gen_golden_tape.py's file for the base set.

One tape -- the one recursion.Builder records for tests/test_witness_tape_gf5.py gf5_hint_circuit: two MP2G_OP_QUINTIC_SQRT and two
MP2G_OP_QUINTIC_QUOTIENT, the first pair as the two sections of an MP2G_OP_PAR region, the second pair reading the first pair's
results -- with inputs and what its replay must produce. Expected
values come from the Python builder's eager evaluation (gf5.py; wire matrix FNV-1a, public-inputs hash, public inputs) -- NOT from
the library's replay -- and every hint result was checked with the ORACLE's GF(p^5) arithmetic when the file was made (root^2 = x
with sgn0(root) = 0, or root = 0 for a non-square; q b = a, or q = 0 for b = 0). The cases: a square x, a non-square x, b = 0."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_witness_tape_gf5 import check_hint_values, fnv, gf5_hint_circuit, orc_sqrt, rand_elem  # noqa: E402

R = importlib.import_module("mapreduce-plonky2_amd.recursion")
GF5 = importlib.import_module("mapreduce-plonky2_amd.gf5")


def main():
    rng = np.random.default_rng(7)
    y = rand_elem(rng)
    square = GF5.mul(y, y)
    while True:
        non_square = rand_elem(rng)
        if not orc_sqrt(non_square)[0]:
            break
    ins = [(square, rand_elem(rng), rand_elem(rng)), (non_square, rand_elem(rng), rand_elem(rng)), (rand_elem(rng), rand_elem(rng), GF5.ZERO)]
    ckts = [gf5_hint_circuit(*v) for v in ins]
    ck = ckts[0]
    cases = []
    for (x, a, b), c in zip(ins, ckts):
        assert np.array_equal(c.tape, ck.tape)
        pi = [int(v) for v in c.public_inputs]
        check_hint_values(x, a, b, pi[0:5], pi[5], pi[6:11])
        check_hint_values(pi[6:11], pi[0:5], x, pi[16:21], pi[21], pi[11:16])
        cases.append({"inputs": [int(w) for e in (x, a, b) for w in e], "wires_fnv1a": fnv(c.wires),
                      "probe": [int(v) for v in c.pi_hash] + pi})
    assert [c["probe"][4 + 5] for c in cases] == [1, 0, cases[2]["probe"][9]]
    out = {"_generator": "tools/gen_golden_tape_gf5.py (expected values: the Python builder's eager evaluation; hint results checked with the oracle's GF(p^5) arithmetic)",
           "gf5_hints": {"tape": [int(x) for x in ck.tape], "n_slots": int(ck.n_slots), "log_n": int(ck.log_n), "input_sids": [int(x) for x in ck.input_sids],
                         "const_slots": [[int(a), int(b)] for a, b in ck.const_slots], "probe": [int(x) for x in ck.pi_hash_sids] + [int(x) for x in ck.public_input_sids],
                         "opcodes_used": sorted({int(op) for _, op in R.tape_instructions(ck.tape)}), "cases": cases}}
    path = os.path.join(ROOT, "tests", "golden", "witness_tape_gf5_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes; opcodes", out["gf5_hints"]["opcodes_used"])


if __name__ == "__main__":
    main()
