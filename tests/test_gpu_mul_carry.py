"""The DEVICE bodies of the general product on the operands of tests/mul_carry_cases.py -- the pairs that put the middle accumulator of
gl_mulw_k on both sides of 2^64 and at its ends, the 49 x 49 edge-word lattice of tests/field_cases.py and 2^16 seeded uniform pairs --
against exact Python integers: gl_mul_wide (both words exact), gl_mulw, gl_mul and gl_mul_addw (canonical value exact) through
tests/devfield, and gl_mulw_k, the form the S-boxes use, through tests/devfield_mulk (canonical value exact, and word for word what
gl_mulw returns: both reduce the same 128-bit integer). Every comparison happens on the host."""
import numpy as np
import pytest

import devfield as D
import devfield_mulk as K
import mul_carry_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    a, b = C.pairs()
    return a, b, [x * y for x, y in zip(a.tolist(), b.tolist())]


def _report(what, bad, *cols):
    assert not bad, "%s: %d wrong, first at %d: %s" % (what, len(bad), bad[0], " ".join("%#x" % int(c[bad[0]]) for c in cols))


def test_gl_mul_wide(pairs):
    a, b, _ = pairs
    lo, hi = D.scalar("gl_mul_wide", a, b)
    _report("gl_mul_wide", C.bad_wide(a, b, lo, hi), a, b, lo, hi)


def test_gl_mulw(pairs):
    a, b, want = pairs
    out, canon = D.scalar("gl_mulw", a, b)
    _report("gl_mulw", C.bad_weak(want, out, canon), a, b, out, canon)


def test_gl_mul(pairs):
    a, b, want = pairs
    out, _ = D.scalar("gl_mul", a, b)
    _report("gl_mul", C.bad_canon(want, out), a, b, out)


def test_gl_mul_addw():
    a, b, c = C.triples()
    want = [x * y + z for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())]
    out, canon = D.scalar("gl_mul_addw", a, b, c)
    _report("gl_mul_addw", C.bad_weak(want, out, canon), a, b, c, out, canon)


def test_gl_mulw_k(pairs):
    a, b, want = pairs
    out, canon = K.mulw_k(a, b)
    _report("gl_mulw_k", C.bad_weak(want, out, canon), a, b, out, canon)
    plain, _ = D.scalar("gl_mulw", a, b)
    differ = np.nonzero(out != plain)[0].tolist()
    _report("gl_mulw_k against gl_mulw", differ, a, b, out, plain)
