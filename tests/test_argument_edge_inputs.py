"""The case lists of tests/edge_inputs.py for the permutation, lookup and opening tests, checked on the reference alone (no GPU):
equality with an expected output proves something only if that output has not collapsed, the planted zeros sit where the GPU
test says they do, and the lookup geometries still put the scan's run boundaries where the GPU test wants them."""
import numpy as np
import pytest

import circuits as C
import edge_inputs as E
import oracle as O

P = O.P
shape_id = lambda s: "-".join(map(str, s))


def test_gammas_of_recipe_a():
    lattice = set(E.F.EC)
    assert len(E.GAMMAS_A) == 26 and {2**31 - 1, 2**31, 2**32 - 2} <= {int(g) for g in E.GAMMAS_A}
    assert all((P - int(g)) % P not in lattice for g in E.GAMMAS_A)
    for betas, gammas in E.PERM_B_FIXED:
        assert betas[0] != 0
    assert {0, 1, P - 1} <= {b for bs, _ in E.PERM_B_FIXED for b in bs} and {0, 1, P - 1} <= {g for _, gs in E.PERM_B_FIXED for g in gs}


@pytest.mark.parametrize("recipe", E.PERM_RECIPES)
@pytest.mark.parametrize("shape", E.PERM_SHAPES, ids=shape_id)
def test_unplanted_outputs_are_informative(shape, recipe):
    log_n, num_routed, degree, nc = shape
    wires, sigmas, betas, gammas, want = E.perm_case(shape, recipe)
    lattice = set(E.F.EC)
    drawn = [{int(v) for v in a.ravel()} <= lattice for a in (wires, sigmas, betas, gammas)]
    assert drawn == ([True, True, False, True] if recipe[0] == "A" else [False, False, True, True])  # never all four
    assert want.shape == (nc * (num_routed // degree), 1 << log_n)
    assert (want != 0).all()                     # Z has not collapsed
    assert (want >= np.uint64(1 << 63)).any()    # and the values are not all small
    assert (want[:nc, 0] == 1).all()
    if shape in E.PERM_EXACT_SHAPES:
        assert np.array_equal(want, E.perm_exact(wires, sigmas, betas, gammas, degree))


@pytest.mark.parametrize("shape", E.PERM_PLANTED_SHAPES, ids=shape_id)
def test_planted_zeros_are_where_the_gpu_test_expects_them(shape):
    log_n, num_routed, degree, nc = shape
    n, chunks = 1 << log_n, num_routed // degree
    wires, sigmas, betas, gammas, plant = E.perm_planted_case(shape)
    want = O.partial_products_and_zs(wires, sigmas, betas, gammas, degree)
    assert np.array_equal(want, E.perm_exact(wires, sigmas, betas, gammas, degree))
    xs = [pow(E.root_of_unity(log_n), i, P) for i in range(n)]

    def factors(c, i, k, which):
        b, g = int(betas[c]), int(gammas[c])
        return [(int(wires[j, i]) + b * (pow(O.MULT_GEN, j, P) * xs[i] if which == "num" else int(sigmas[j, i])) + g) % P
                for j in range(k * degree, (k + 1) * degree)]

    assert plant[0][0] != plant[1][0]
    for c, (row, chunk) in plant.items():
        assert 3 * n // 4 <= row < n - 1 and 0 < chunk < chunks  # last quarter, rows after it, chunks before it
        # exactly one zero factor over all rows and chunks of this challenge: the planted one, on the planted side
        zeros = [(i, k, which) for i in range(n) for k in range(chunks) for which in ("num", "den") if 0 in factors(c, i, k, which)]
        assert zeros == [(row, chunk, "den" if c == 0 else "num")]
        z, pp = want[c], want[nc + c * (chunks - 1):nc + (c + 1) * (chunks - 1)]
        assert (z[:row + 1] != 0).all() and (z[row + 1:] == 0).all()
        assert (pp[:, :row] != 0).all() and (pp[:chunk, row] != 0).all() and (pp[chunk:, row] == 0).all() and (pp[:, row + 1:] == 0).all()
    assert int((want == 0).sum()) < want.size // 4  # most of the output still carries information


def straddlers(total, lut_rows):
    """lanes whose run holds both a LookupTable row (walk position < lut_rows) and a LookupGate row"""
    return [l for l, (t0, t1) in enumerate(E.scan_runs(total)) if t0 < lut_rows < t1]


@pytest.mark.parametrize("L,k,log_n,total,lut_rows", E.SCAN_CASES)
def test_lookup_geometries(L, k, log_n, total, lut_rows):
    ckt = C.build(log_n, C.ALL_KINDS + C.LOOKUP_KINDS, 5, luts=[(E.scan_table(L), k)])
    assert E.scan_rows(ckt.luts[0]) == (total, lut_rows)
    assert lut_rows == -(-L // C.NUM_LUT_SLOTS) and total - lut_rows == max(1, -(-k // C.NUM_LU_SLOTS))
    runs = E.scan_runs(total)
    assert runs[0][0] == 0 and all(a[1] == b[0] for a, b in zip(runs, runs[1:])) and runs[-1][1] == total
    lens = [t1 - t0 for t0, t1 in runs]
    expect = {64: (1, [], [1] * 64), 65: (2, [31], [2] * 32 + [1] + [0] * 31), 130: (3, [42], [3] * 43 + [1] + [0] * 20),
              2: (1, [], [1, 1] + [0] * 62)}[total]
    assert (max(lens), straddlers(total, lut_rows), lens) == expect


def test_two_table_circuit_geometry():
    ckt = C.build(8, C.ALL_KINDS + C.LOOKUP_KINDS, 5, luts=[(E.scan_table(1638), 80), (E.scan_table(1), 3)])
    assert [E.scan_rows(t) for t in ckt.luts] == [(65, 63), (2, 1)]  # the rows kernel's grid: two blocks, the small table needs one lane pair


def test_exact_extension_evaluation_and_oracle_fri_wrapper():
    """E.ext_eval_exact equals the oracle's openings, and O.fri_prove continues a transcript as orc_pcs_prove does: with
    pcs_prove's own transcript replayed it returns pcs_prove's proof"""
    log_n, ws = 6, (5, 9, 4, 3)
    fp = O.standard_params(log_n, ws, pow_bits=6, num_queries=4)
    vals = [O.rand_field((w, 1 << log_n), 100 + i) for i, w in enumerate(ws)]
    cd, ph = O.rand_field(4, 1), O.rand_field(4, 2)
    caps, openings, proof = O.pcs_prove(fp, vals, cd, ph)
    coeffs = [O.fft(v, inverse=True) for v in vals]
    committed = O.fri_commit(fp, coeffs)
    assert all(np.array_equal(O.merkle_cap(l, fp.cap_height).reshape(-1), caps[o]) for o, l in enumerate(committed[2]))
    ch = O.Challenger()
    ch.observe(cd), ch.observe(ph)
    ch.observe(caps[1]), ch.get(4)  # betas, gammas
    ch.observe(caps[2]), ch.get(2)  # alphas
    ch.observe(caps[3])
    zeta = ch.get(2)
    assert np.array_equal(np.concatenate([E.ext_eval_exact(c, zeta) for c in coeffs]), openings[:sum(ws)])
    ch.observe(openings)
    assert np.array_equal(O.fri_prove(fp, committed, zeta, ch), proof)
    for point in E.OPENING_POINTS:
        assert all(0 <= v < P for v in point)
    assert E.ext_eval_exact(np.array([[3, 5, P - 1]], dtype=np.uint64), (0, 1)).tolist() == [[(3 + 7 * (P - 1)) % P, 5]]
