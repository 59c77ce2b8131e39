"""mp2g_partial_products_and_zs (csrc/zperm.hip: zpp_chunk_kernel, zpp_scan_kernel) on edge operands, at the limits of zpp_compute
and with zero numerators and denominators planted, against the oracle (and, at the two smallest shapes, Python integers). The
case lists are those of tests/edge_inputs.py; tests/test_argument_edge_inputs.py checks, on the reference alone, that equality
with these expected outputs says something."""
import ctypes

import numpy as np
import pytest

import edge_inputs as E
import oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("recipe", E.PERM_RECIPES)
@pytest.mark.parametrize("shape", E.PERM_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_partial_products_on_edge_operands(ctx, mp2, shape, recipe):
    wires, sigmas, betas, gammas, want = E.perm_case(shape, recipe)
    got = mp2.partial_products_and_zs(ctx, wires, sigmas, betas, gammas, shape[2])
    assert np.array_equal(got, want)
    if shape in E.PERM_EXACT_SHAPES:
        assert np.array_equal(got, E.perm_exact(wires, sigmas, betas, gammas, shape[2]))


@pytest.mark.parametrize("shape", E.PERM_PLANTED_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_planted_zero_denominator_and_numerator(ctx, mp2, shape):
    """inverse-or-zero of one chunk's denominator (challenge 0) and a zero numerator (challenge 1): Z of that challenge dies after
    the planted row and nowhere else, and the chunks sharing the batched inversion with the zero one keep their values"""
    log_n, num_routed, degree, nc = shape
    wires, sigmas, betas, gammas, plant = E.perm_planted_case(shape)
    got = mp2.partial_products_and_zs(ctx, wires, sigmas, betas, gammas, degree)
    assert np.array_equal(got, O.partial_products_and_zs(wires, sigmas, betas, gammas, degree))
    assert np.array_equal(got, E.perm_exact(wires, sigmas, betas, gammas, degree))
    num_prods = num_routed // degree - 1
    for c, (row, chunk) in plant.items():
        z, pp = got[c], got[nc + c * num_prods:nc + (c + 1) * num_prods]
        assert (z[:row + 1] != 0).all() and (z[row + 1:] == 0).all()
        assert (pp[:, :row] != 0).all() and (pp[:chunk, row] != 0).all() and (pp[chunk:, row] == 0).all() and (pp[:, row + 1:] == 0).all()


def raw_call(mp2, ctx, wires, sigmas, betas, gammas, num_routed, degree):
    """mp2g_partial_products_and_zs with num_routed and degree as given (the Python wrapper derives num_routed from the sigmas
    and divides by degree); the output buffer is sized for the limits, whatever is asked for"""
    n = sigmas.shape[1]
    out = np.zeros((betas.size * 64, n), dtype=np.uint64)
    rc = mp2.load().mp2g_partial_products_and_zs(ctx.h, O.p(wires), wires.shape[0], O.p(sigmas), n.bit_length() - 1, num_routed, degree,
                                                 O.p(betas), O.p(gammas), betas.size, O.p(out))
    return rc, out


def test_refusals_leave_the_context_usable(ctx, mp2):
    """the four refusals of zpp_compute / mp2g_partial_products_and_zs, each followed by a call that must still be right"""
    n = 16
    wires, sigmas = O.arr(O.rand_field((300, n), 31)), O.arr(O.rand_field((300, n), 32))
    betas, gammas = O.arr(O.rand_field(2, 33)), O.arr(O.rand_field(2, 34))
    good = O.partial_products_and_zs(wires, sigmas[:16], betas, gammas, 8)
    # degree 0; num_routed no multiple of degree; 17 chunks; 264 routed wires in 33 chunks, and in 11 chunks (past ZP_MAX_ROUTED alone)
    for num_routed, degree in [(16, 0), (12, 8), (136, 8), (264, 8), (264, 24)]:
        rc, _ = raw_call(mp2, ctx, wires, sigmas, betas, gammas, num_routed, degree)
        assert rc != 0, (num_routed, degree)
        with pytest.raises(mp2.Mp2gError):
            mp2._ck(rc)
        assert np.array_equal(mp2.partial_products_and_zs(ctx, wires, sigmas[:16], betas, gammas, 8), good)
    # the largest shapes that are not refused, through the same raw entry
    for num_routed, degree in [(128, 8), (256, 16)]:
        rc, out = raw_call(mp2, ctx, wires, sigmas, betas, gammas, num_routed, degree)
        assert rc == 0
        want = O.partial_products_and_zs(wires, sigmas[:num_routed], betas, gammas, degree)
        assert np.array_equal(out[:want.shape[0]], want)
