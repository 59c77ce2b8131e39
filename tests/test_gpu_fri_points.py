"""The opening pipeline of csrc/fri.hip (ext_powers_kernel, openings_kernel, compose_kernel, divide_kernel, combine_kernel,
fold_coeffs_kernel) at chosen opening points -- 0, 1, -1, X, -1 - X, -X and one uniform point -- instead of transcript-drawn
ones, on coefficients of p - 1 and of the edge lattice: PolynomialBatch.eval_ext against Python integers, mp2g_fri_prove against
orc_fri_prove over a transcript fed identically to both sides."""
import ctypes

import numpy as np
import pytest

import edge_inputs as E
import oracle as O

pytestmark = pytest.mark.gpu
P = O.P


def coefficients(kind, w, n, seed):
    return np.full((w, n), P - 1, dtype=np.uint64) if kind == "p-1" else E.edge_rows((w, n), seed)


@pytest.mark.parametrize("kind", ["p-1", "lattice"])
@pytest.mark.parametrize("w", [1, 4, 5, 135])    # OP_POLYS = 4 polynomials per block: every remainder
@pytest.mark.parametrize("log_n", [3, 8, 13])    # 1, 1 and 32 gl_cols terms per lane
def test_eval_ext_against_python_integers(ctx, mp2, log_n, w, kind):
    coeffs = coefficients(kind, w, 1 << log_n, 600 + log_n + w)
    b = mp2.PolynomialBatch.from_coeffs_dev(ctx, ctx.to_device(coeffs), log_n, w)
    assert np.array_equal(b.coeffs, coeffs)
    for point in E.OPENING_POINTS:
        got = b.eval_ext(np.array(point, dtype=np.uint64))
        assert np.array_equal(got, E.ext_eval_exact(coeffs, point)), point
    b.free()


def test_eval_ext_refuses_a_non_canonical_point(ctx, mp2):
    coeffs = coefficients("lattice", 3, 8, 1)
    b = mp2.PolynomialBatch.from_coeffs_dev(ctx, ctx.to_device(coeffs), 3, 3)
    for point in [(P, 0), (0, P), (1, 0xFFFFFFFFFFFFFFFF)]:
        with pytest.raises(mp2.Mp2gError):
            b.eval_ext(np.array(point, dtype=np.uint64))
    assert np.array_equal(b.eval_ext(np.array((P - 1, 0), dtype=np.uint64)), E.ext_eval_exact(coeffs, (P - 1, 0)))
    b.free()


# log_n 3: no FRI layer; 7: one; 10: divide_kernel with 1024 lanes of one coefficient; 12: four coefficients per lane.
# The standard widths with every coefficient p - 1 put 255 terms of (p - 1) alpha^m into compose_kernel's gl_cols.
@pytest.mark.parametrize("log_n,ws,kind", [(3, (5, 9, 4, 3), "lattice"), (7, (5, 9, 4, 3), "lattice"), (10, (5, 9, 4, 3), "lattice"),
                                            (12, (5, 9, 4, 3), "lattice"), (7, (84, 135, 20, 16), "p-1")])
def test_fri_prove_at_chosen_points(ctx, mp2, log_n, ws, kind):
    ofp = O.standard_params(log_n, ws, pow_bits=6, num_queries=4)
    fp = mp2.FriParams()
    ctypes.memmove(ctypes.byref(fp), ctypes.byref(ofp), ctypes.sizeof(fp))
    n = 1 << log_n
    coeffs = [coefficients(kind, w, n, 700 + log_n + i) for i, w in enumerate(ws)]
    batches = [mp2.PolynomialBatch.from_coeffs_dev(ctx, ctx.to_device(c), log_n, w) for c, w in zip(coeffs, ws)]
    committed = O.fri_commit(ofp, coeffs)
    for b, levels in zip(batches, committed[2]):
        assert np.array_equal(b.cap, O.merkle_cap(levels, ofp.cap_height))
    head = O.rand_field(8, 5)
    for point in E.OPENING_POINTS:
        zeta = np.array(point, dtype=np.uint64)
        # the transcript before the FRI tail: eight words and the openings at zeta, the same on both sides
        openings = np.concatenate([E.ext_eval_exact(c, point) for c in coeffs])
        ch, och = mp2.Challenger(ctx), O.Challenger()
        for words in (head, openings.reshape(-1)):
            ch.observe_elements(words)
            och.observe(words)
        got = mp2.fri_prove(ctx, fp, batches, zeta, ch)
        assert np.array_equal(got, O.fri_prove(ofp, committed, zeta, och)), point
        ch.free()
    for b in batches:
        b.free()
