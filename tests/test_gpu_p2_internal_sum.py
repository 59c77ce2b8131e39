"""The DEVICE body of Poseidon2's internal layer (p2_internal, csrc/poseidon.cuh) on states that aim at its limb sum: the sum's top
word and the carry of the low words at every value in 0..11, the subtract that recovers that carry on both sides of its wrap, the high
words at their maximum, the field's edges, every edge word in one limb at a time and 2^16 seeded uniform states
(tests/p2_internal_sum_cases.py). The layer runs through tests/devfield; the comparison with field_cases.p2_internal_matrix() happens
on the host, bit-exact after canonicalisation. tests/test_p2_internal_sum_cases.py guards the tables and runs the portable body."""
import pytest

import devfield as D
import field_checks as C
import p2_internal_sum_cases as S

pytestmark = pytest.mark.gpu


def test_p2_internal_on_sum_cases():
    states, want = S.reference()
    assert len(states) >= 3 * 13 + 1 + 24 + 3 * 13 + 12 * 49 + S.N_UNIFORM
    C.assert_weak_rows(D, "p2_internal", D.vec("p2_internal", states)[0], want, states)
