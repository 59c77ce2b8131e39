"""The quotient and FRI kernels that read precomputed power tables (the per-circuit coset tables of zperm.h, the per-batch
alpha / zeta power tables): complete proofs bit-exact against the oracle at edge shapes -- small and larger log_n, one and
two challenge rounds, a table of a single gate (num_selectors == 1) and the full gate set."""
import ctypes

import numpy as np
import pytest

import circuits as C
import oracle as O

pytestmark = pytest.mark.gpu


SHAPES = [(log_n, "one_gate") for log_n in (3, 5, 9, 12)] + [(log_n, "all_kinds") for log_n in (5, 9, 12)]


@pytest.mark.parametrize("log_n,table", SHAPES)
@pytest.mark.parametrize("nc", [1, 2])
def test_proof_matches_oracle(ctx, mp2, log_n, table, nc):
    kinds = [(C.ARITHMETIC, 20, 0, 0)] if table == "one_gate" else C.ALL_KINDS
    ckt = C.build(log_n, kinds, 40 + log_n)
    ofp = O.standard_params(log_n, (int(ckt.pre.shape[0]), C.NUM_WIRES, 10 * nc, 8 * nc), zs_count=nc, pow_bits=2, num_queries=2)
    fp = mp2.FriParams()
    ctypes.memmove(ctypes.byref(fp), ctypes.byref(ofp), ctypes.sizeof(fp))
    B = 2
    pr = mp2.BatchedProver(ctx, fp, B)
    pr.set_preprocessed(ctx.to_device(ckt.pre))
    pr.enable_permutation(C.NUM_ROUTED, 8)
    pr.enable_quotient()
    pr.set_gates([mp2.Gate(g.kind, g.p0, g.p1, g.p2, g.selector_index, g.group_start, g.group_end) for g in ckt.gates], ckt.num_selectors)
    cd = O.rand_field(4, 7 + nc)
    pr.prove([ctx.to_device(np.stack([ckt.wires] * B)), None, None], ctx.to_device(cd), ctx.to_device(np.stack([ckt.pi_hash] * B)))
    caps, openings, proofs = pr.results()
    oc, oo, op, chal = C.prove(ckt, ofp, cd)
    for b in range(B):
        assert np.array_equal(caps[b], oc), "caps (the quotient commitment reads the coset tables)"
        assert np.array_equal(openings[b], oo), "openings (zeta power tables)"
        assert np.array_equal(proofs[b], op), "FRI proof (alpha power tables, composition)"
    assert C.identity_check(ckt, ofp, openings[0], chal) == 0
    pr.free()
