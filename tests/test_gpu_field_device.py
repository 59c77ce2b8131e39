"""The DEVICE bodies of csrc/gl.cuh, gl5.cuh, poseidon.cuh, poseidon_wave.cuh and ntt_arith.cuh, one routine at a time, on the edge-word
lattice of tests/field_cases.py plus 2^16 seeded uniform operands, against exact Python integers (tests/field_checks.py). The routines
run through tests/devfield (libmp2g_devfield.so); every comparison happens on the host, bit-exact, with no tolerance.
tests/test_field_host.py runs the same checks on the portable bodies."""
import pytest

import devfield as D
import field_cases as F
import field_checks as C

pytestmark = pytest.mark.gpu

VEC_OPS = {"gl2_mul", "gl2_inv", "gl2_scale", "gl5_mul", "gl5_sqr", "gl5_small", "gl5_mul_kz", "gl5_frob1", "gl5_frob2", "gl5_inv",
           "gl5_norm", "gl5_sqrt", "gl5_is_square", "gl5_sgn0", "p2_external", "p2_external_rc", "p2_internal", "poseidon_mds",
           "poseidon_mds_rc", "poseidon2_perm", "poseidon_perm", "two_to_one_p2", "two_to_one_p", "wp2_external", "wp2_internal", "wp2_perm"}


def test_harness_exposes_every_operation():
    assert set(D.scalar_ops()) == set(F.OPS)
    assert set(D.vec_ops()) == VEC_OPS


@pytest.mark.parametrize("name", sorted(F.OPS))
def test_scalar_operation(name):
    C.scalar_operation(D, name)


@pytest.mark.parametrize("terms,f", F.COLS_SHAPES)
def test_gl_cols(terms, f):
    C.gl_cols(D, terms, f)


def test_gl2():
    C.gl2(D)


def test_gl5_mul_sqr():
    C.gl5_mul_sqr(D)


@pytest.mark.parametrize("k", C.GL5_SMALL_K)
def test_gl5_small(k):
    C.gl5_small(D, k)


@pytest.mark.parametrize("k", C.GL5_KZ_K)
def test_gl5_mul_kz(k):
    C.gl5_mul_kz(D, k)


def test_gl5_frobenius_norm_sgn0():
    C.gl5_frobenius_norm_sgn0(D)


def test_gl5_inv():
    C.gl5_inv(D)


def test_gl5_sqrt_and_is_square():
    C.gl5_sqrt_and_is_square(D)


def test_p2_external_layers():
    C.p2_external_layers(D, wave=True)


def test_p2_internal_layers():
    C.p2_internal_layers(D, wave=True)


def test_poseidon_mds_layers():
    C.poseidon_mds_layers(D)


def test_permutations_and_two_to_one():
    """poseidon2_perm, poseidon_perm, wp2_perm and two_to_one against the oracle's permutation on the same canonical states"""
    C.permutations(D, device=True)
