"""The DEVICE body of gl_mulc_addw (csrc/gl.cuh), the multiply-add by a constant that Poseidon2's internal layer uses for d_i s_i + sum:
every diagonal entry, as p2_internal calls it (the narrow form or the one that folds the carry), on the full edge-word lattice of
tests/field_cases.py for a and c, the operands that drive each column to its end (tests/p2_diag_cases.py) and 2^16 seeded uniform
pairs, against exact Python integers. The routine runs through tests/devfield_mulc; the comparison canon(out) == (a d + c) mod p happens
on the host, bit-exact."""
import pytest

import devfield_mulc as D
import field_cases as F
import p2_diag_cases as C

pytestmark = pytest.mark.gpu


def test_harness_takes_the_forms_the_header_names():
    d = F.header_table("POSEIDON2_DIAG_M1")
    want = sum(1 << k for k in range(12) if (d[k] >> 32) + (((d[k] << 32) % F.P) >> 32) <= (1 << 32) - 3)
    assert D.narrow_mask() == want
    assert 0 < want < (1 << 12) - 1, "both forms are in use"


@pytest.mark.parametrize("k", range(12))
def test_mulc_addw(k):
    a, c = C.cases(k)
    assert len(a) >= 49 * 49 + 3 + C.N_UNIFORM
    out = D.mulc_addw(a, c, k)
    bad = C.bad_cases(k, a, c, out)
    assert not bad, "k=%d: %d wrong, first a=%#x c=%#x out=%#x" % (k, len(bad), int(a[bad[0]]), int(c[bad[0]]), int(out[bad[0]]))
