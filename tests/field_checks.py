"""The checks of the field-arithmetic routines against tests/field_cases.py, written once for two back ends: tests/devfield (the device
bodies on the GPU, test_gpu_field_device.py) and the host program of test_field_host.py (the portable bodies). A back end `D` offers
scalar(name, *cols), cols(terms, f, a, b) and vec(name, x, y=, rc=, k=) as tests/devfield.py does.

Bit-exact throughout: canonical outputs equal the reference, weak outputs are congruent to it and their gl_canon equals it, widening
products equal the integer, inverses and roots are checked by the exact product."""
import numpy as np

import field_cases as F
import oracle as O

P = F.P


def rows(a):
    return a.tolist() if isinstance(a, np.ndarray) else a  # lists hold Python integers already (numpy would turn >= 2^63 into floats)


def canon(D, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return D.scalar("gl_canon", a.ravel())[0].reshape(a.shape)


def assert_rows(name, got, want, ins):
    got, want = rows(got), rows(want)
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d cases differ; first: case %d in %s got %s want %s" % (
        name, len(bad), len(want), bad[0], [hex(int(v)) for v in np.ravel(ins[bad[0]])], got[bad[0]], want[bad[0]])


def assert_weak_rows(D, name, got, want, ins):
    """weak outputs: congruent to the reference, and the back end's gl_canon of them equals it"""
    assert_rows(name + " (mod p)", [[v % P for v in r] for r in rows(got)], want, ins)
    assert_rows(name + " (gl_canon)", canon(D, got), want, ins)


def scalar_failures(D, name):
    """(indices of the failing cases, number of lattice cases, columns, o0, o1)"""
    cols, n_lattice = F.scalar_cases(name)
    o0, o1 = D.scalar(name, *cols)
    return F.check_scalar(name, cols, o0, o1), n_lattice, cols, o0, o1


def scalar_operation(D, name):
    bad, n_lattice, cols, o0, o1 = scalar_failures(D, name)
    if bad:
        i = bad[0]
        lat = sum(1 for j in bad if j < n_lattice)
        raise AssertionError("%s: %d lattice and %d uniform cases wrong; first: case %d, operands %s -> (%#x, %#x)" % (
            name, lat, len(bad) - lat, i, [hex(int(c[i])) for c in cols], int(o0[i]), int(o1[i])))


def gl_cols(D, terms, f):
    a, b = F.cols_inputs(terms, f)
    assert_rows("gl_cols %d x%d" % (terms, f), D.cols(terms, f, a, b), F.cols_ref(terms, f), np.concatenate([a, b], axis=1))


def gl2(D):
    a, b = F.element_pairs(2, 0)
    ab = np.concatenate([a, b], axis=1)
    assert_rows("gl2_mul", D.vec("gl2_mul", a, y=b)[0], [F.gl2_mul(x, y) for x, y in zip(rows(a), rows(b))], ab)
    assert_rows("gl2_scale", D.vec("gl2_scale", a, y=b)[0], [[x[0] * y[0] % P, x[1] * y[0] % P] for x, y in zip(rows(a), rows(b))], ab)
    x = np.concatenate([F.elements(2, True, 1), a])
    xi = D.vec("gl2_inv", x)[0]
    assert int(xi.max()) < P
    assert_rows("gl2_inv", [F.gl2_mul(u, v) for u, v in zip(rows(x), rows(xi))], [[int(any(u)), 0] for u in rows(x)], x)


def x5():
    return F.elements(5, True, 5)


def gl5_mul_sqr(D):
    a, b = F.element_pairs(5, 0)
    assert_rows("gl5_mul", D.vec("gl5_mul", a, y=b)[0], [F.gl5_mul(x, y) for x, y in zip(rows(a), rows(b))], np.concatenate([a, b], axis=1))
    assert_rows("gl5_sqr", D.vec("gl5_sqr", a)[0], [F.gl5_mul(x, x) for x in rows(a)], a)


GL5_SMALL_K = [2, 263, 0xFFFFFFFF]
GL5_KZ_K = [1, 263, 0x55555555]  # 3 k < 2^32


def gl5_small(D, k):
    x = x5()
    assert_rows("gl5_small", D.vec("gl5_small", x, k=k)[0], [[v * k % P for v in r] for r in rows(x)], x)


def gl5_mul_kz(D, k):
    x = x5()
    assert_rows("gl5_mul_kz", D.vec("gl5_mul_kz", x, k=k)[0], [F.gl5_mul(r, [0, k, 0, 0, 0]) for r in rows(x)], x)


def gl5_frobenius_norm_sgn0(D):
    x = x5()
    xs = rows(x)
    assert_rows("gl5_frob1", D.vec("gl5_frob1", x)[0], [F.gl5_frob(r, 1) for r in xs], x)
    assert_rows("gl5_frob2", D.vec("gl5_frob2", x)[0], [F.gl5_frob(r, 2) for r in xs], x)
    assert_rows("gl5_norm", D.vec("gl5_norm", x)[0], [[F.gl5_norm(r), 0, 0, 0, 0] for r in xs], x)
    assert rows(D.vec("gl5_sgn0", x)[1]) == [F.gl5_sgn0(r) for r in xs]


def gl5_inv(D):
    x = x5()
    xi = D.vec("gl5_inv", x)[0]
    assert int(xi.max()) < P
    assert_rows("gl5_inv", [F.gl5_mul(u, v) for u, v in zip(rows(x), rows(xi))], [[int(any(u)), 0, 0, 0, 0] for u in rows(x)], x)


def gl5_sqrt_and_is_square(D):
    # the squares of every other input (by the reference) join the table, so that both outcomes are well represented
    x = x5()
    x = np.concatenate([x, np.array([F.gl5_mul(v, v) for v in rows(x[::2])], dtype=np.uint64)])
    xs = rows(x)
    want_flag = [int(F.is_square(F.gl5_norm(v))) for v in xs]  # Euler's criterion on the norm
    assert 0 < sum(want_flag) < len(want_flag)
    root, flag = D.vec("gl5_sqrt", x)
    assert rows(flag) == want_flag
    assert rows(D.vec("gl5_is_square", x)[1]) == want_flag
    assert int(root.max()) < P
    assert_rows("gl5_sqrt squared", [F.gl5_mul(r, r) for r in rows(root)], [v if s else [0] * 5 for v, s in zip(xs, want_flag)], x)
    # which of the two roots: the oracle's (orc_gl5_sqrt)
    want = np.zeros_like(x)
    for i, v in enumerate(x):
        buf = np.zeros(5, dtype=np.uint64)
        if O.lib().orc_gl5_sqrt(O.p(np.ascontiguousarray(v)), O.p(buf)):
            want[i] = buf
    assert_rows("gl5_sqrt root choice", root, want, x)


def weak_states():
    return F.elements(12, False, 12)


def canonical_states():
    return F.elements(12, True, 13)


def p2_external_layers(D, wave):
    w = weak_states()
    s = rows(w)
    plain = F.mat_apply(F.P2_EXTERNAL, s)
    assert_weak_rows(D, "p2_external_rc<false>", D.vec("p2_external", w)[0], plain, w)
    if wave:
        assert_weak_rows(D, "wp2_external", D.vec("wp2_external", w)[0], plain, w)
    ext = F.header_table("POSEIDON2_RC_EXT")
    for k in (0, 7):
        assert_weak_rows(D, "p2_external_rc<true> round %d" % k, D.vec("p2_external_rc", w, k=k)[0],
                         F.mat_apply(F.P2_EXTERNAL, s, ext[12 * k:12 * k + 12]), w)
    assert_weak_rows(D, "p2_external_rc<true> all p-1", D.vec("p2_external_rc", w, rc=[P - 1] * 12)[0],
                     F.mat_apply(F.P2_EXTERNAL, s, [P - 1] * 12), w)


def p2_internal_layers(D, wave):
    w = weak_states()
    want = F.mat_apply(F.p2_internal_matrix(), rows(w))
    assert_weak_rows(D, "p2_internal", D.vec("p2_internal", w)[0], want, w)
    if wave:
        assert_weak_rows(D, "wp2_internal", D.vec("wp2_internal", w)[0], want, w)


def poseidon_mds_layers(D):
    w = weak_states()
    s = rows(w)
    assert_weak_rows(D, "poseidon_mds_rc<false>", D.vec("poseidon_mds", w)[0], F.mat_apply(F.POSEIDON_MDS, s), w)
    rc = F.header_table("POSEIDON_RC")
    for k in (1, 29):
        assert_weak_rows(D, "poseidon_mds_rc<true> round %d" % k, D.vec("poseidon_mds_rc", w, k=k)[0],
                         F.mat_apply(F.POSEIDON_MDS, s, rc[12 * k:12 * k + 12]), w)
    assert_weak_rows(D, "poseidon_mds_rc<true> all p-1", D.vec("poseidon_mds_rc", w, rc=[P - 1] * 12)[0],
                     F.mat_apply(F.POSEIDON_MDS, s, [P - 1] * 12), w)


def permutations(D, device):
    c = canonical_states()
    want = [np.array([O.perm(s, v) for s in c]) for v in (0, 1)]
    assert_rows("poseidon2_perm", D.vec("poseidon2_perm", c)[0], want[0], c)
    assert_rows("poseidon_perm", D.vec("poseidon_perm", c)[0], want[1], c)
    if device:
        assert_rows("wp2_perm", D.vec("wp2_perm", c)[0], want[0], c)
        lr = c.copy()
        lr[:, 8:] = 0
        for v, name in ((0, "two_to_one_p2"), (1, "two_to_one_p")):
            w21 = np.array([O.perm(s, v) for s in lr])
            w21[:, 4:] = 0
            # the harness reads l || r from the first eight limbs and ignores the rest
            assert_rows(name, D.vec(name, c)[0], w21, c)
