"""Guards the operand tables of tests/field_cases.py: a model of the device sequences, evaluated on the operands alone, must find every
branch class that the device arithmetic can take, and the references must agree with slower independent forms."""
import field_cases as F

P = F.P


def test_lattice_definitions():
    assert len(F.W) == 7 and len(F.E) == 49
    assert all(e < P for e in F.EC) and {0, 1, P - 1, P - 2} <= set(F.EC)
    assert {P, P + 1, (1 << 64) - 1} <= set(F.EANY)
    assert set(F.E) <= set(F.EANY) and set(F.EC) <= set(F.EANY)
    cols, n_lattice = F.scalar_cases("gl_mul_add_wide")
    assert n_lattice == len(F.EANY) ** 2 * len(F.S3) and all(len(c) == n_lattice + F.N_UNIFORM for c in cols)
    assert int(F.scalar_cases("gl_add")[0][0].max()) < P and int(F.scalar_cases("gl_reduce96w")[0][1].max()) < 1 << 32


def test_every_branch_class_is_present():
    bc = F.branch_classes()
    assert all(bc["reduce128w_cb"].get(k, 0) > 0 for k in [(0, 0), (0, 1), (1, 0), (1, 1)]), bc
    assert bc["reduce96w_c"].get(0, 0) > 0 and bc["reduce96w_c"].get(1, 0) > 0, bc
    assert bc["reduce128_high"] > 0 and bc["mul_high"] > 0 and bc["mul_small_high"] > 0, bc
    # gl_add takes t = s - p when (carry | s + EPS carries): no carry and s < p, no carry and s >= p, carry
    assert all(bc["add_select"].get(k, 0) > 0 for k in [(0, 0), (0, 1), (1, 0)]), bc
    for name in ("gl_sub", "gl_sub_mul_2p48", "gl_sub_mul_2p72"):
        assert bc[name + "_borrow"][0] > 0 and bc[name + "_borrow"][1] > 0, bc
    assert any(v > 0 for v in bc["cols_top"].values()) and bc["cols_top"][(25, 0)] > 0 and bc["cols_top"][(3, 6)] > 0, bc
    for name in ("p2_external", "poseidon_mds"):
        assert bc["layer_c"][name][0] > 0 and bc["layer_c"][name][1] > 0, bc


def test_uniform_operands_miss_the_rare_branches():
    """why the lattice is needed: 2^16 uniform pairs never borrow in gl_reduce128w (probability 2^-32 each)"""
    lo, hi = (c[-F.N_UNIFORM:].tolist() for c in F.scalar_cases("gl_reduce128w")[0])
    assert all(F.model_reduce128w(x, y)[1] == 0 for x, y in zip(lo, hi))


def test_tables_catch_a_dropped_borrow_correction():
    """gl_reduce128w with the addend c EPS instead of (c - b) EPS: wrong on every (c, b) = (0, 1) case of the lattice and on nothing
    else -- with c = b = 1 the stray + EPS wraps past 2^64, which subtracts p, so that class stays congruent -- and on none of the
    2^16 uniform cases, which never borrow"""
    cols, n_lattice = F.scalar_cases("gl_reduce128w")
    wrong = {}
    for i, (lo, hi) in enumerate(zip(cols[0].tolist(), cols[1].tolist())):
        c, b, r = F.model_reduce128w(lo, hi, borrow_correction=False)
        if r % P != (lo + (hi << 64)) % P:
            assert i < n_lattice
            wrong[(c, b)] = wrong.get((c, b), 0) + 1
    assert wrong == {(0, 1): F.branch_classes()["reduce128w_cb"][(0, 1)]} and wrong[(0, 1)] > 0


def gl5_pow(x, e):
    r = [1, 0, 0, 0, 0]
    while e:
        if e & 1:
            r = F.gl5_mul(r, x)
        x = F.gl5_mul(x, x)
        e >>= 1
    return r


def test_references_against_slower_forms():
    xs = F.elements(5, True, 5)[40:52].tolist()
    for x in xs:
        assert F.gl5_frob(x, 1) == gl5_pow(x, P) and F.gl5_frob(x, 2) == gl5_pow(gl5_pow(x, P), P)
        assert [F.gl5_norm(x), 0, 0, 0, 0] == gl5_pow(x, (P ** 5 - 1) // (P - 1))
    # the matrices against the additions-only forms of the reference implementations
    s = F.elements(12, False, 12)[45].tolist()
    ext = F.mat_apply(F.P2_EXTERNAL, [s])[0]
    blocks = [[sum(F.M4[i][j] * s[4 * b + j] for j in range(4)) for i in range(4)] for b in range(3)]
    assert ext == [(blocks[i // 4][i % 4] + sum(blocks[b][i % 4] for b in range(3))) % P for i in range(12)]
    d = F.header_table("POSEIDON2_DIAG_M1")
    assert F.mat_apply(F.p2_internal_matrix(), [s])[0] == [(d[i] * s[i] + sum(s)) % P for i in range(12)]
    circ, diag = F.header_table("POSEIDON_MDS_CIRC"), F.header_table("POSEIDON_MDS_DIAG")
    assert circ == F.MDS_CIRC and diag == [8] + [0] * 11
    assert F.mat_apply(F.POSEIDON_MDS, [s])[0] == [(sum(circ[i] * s[(i + r) % 12] for i in range(12)) + diag[r] * s[r]) % P for r in range(12)]
    assert F.gl2_mul([3, 5], [7, 11]) == [3 * 7 + 7 * 5 * 11, 3 * 11 + 5 * 7]
