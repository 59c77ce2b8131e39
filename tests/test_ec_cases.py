"""The case lists of tests/ec_cases.py for the Ecgfp5 group kernels, checked on the references alone (no GPU): the oracle that the
GPU test compares with agrees with an exact restatement on Python integers on every small case, the shortcut that gives the large
sums their expected values equals a plain sum, the simple_swu inputs reach every branch of the map, and the one branch they
cannot reach is shown to be unreachable."""
import numpy as np
import pytest

import ec_cases as K
import oracle as O

P = O.P


def same(exact, orc):
    return exact is not None and orc is not None and exact[0] == orc[0].tolist() and exact[1] == orc[1].tolist()


def test_exact_field_and_curve_constants():
    u = tuple(int(x) for x in O.rand_field(5, 0xEC10))
    v = tuple(int(x) for x in O.rand_field(5, 0xEC11))
    assert K.mul(u, K.inv(u)) == K.ONE and K.inv(K.ZERO) == K.ZERO
    assert K.mul(K.power(u, P), K.ONE) == K.frob(u) and K.norm(K.mul(u, v)) == K.norm(u) * K.norm(v) % P
    assert K.is_square(K.sqr(u)) and K.sqrt(K.sqr(u)) in (u, K.neg(u)) and K.sgn0(K.sqrt(K.sqr(u))) == 0
    assert K.is_square(u) == (K.power(u, (K.ORDER - 1) // 2) == K.ONE)  # the norm's symbol is Euler's criterion
    assert [K.sgn0(x) for x in ((0, 0, 0, 0, 0), (0, 0, 3, 2, 2), (0, 2, 1, 1, 1), (P - 1, 1, 1, 1, 1))] == [0, 1, 0, 0]
    # the Weierstrass model carries the curve: (x, y) -> (x + 2/3, y)
    pt = K.decode(K.el(K.base_points(1)[0]))
    assert K.on_curve(pt) and K.sqr(pt[1]) == K.g_sw(K.add(pt[0], K.TWO_THIRDS))
    assert K.mul(K.scale(K.TWO_THIRDS, 3), K.ONE) == K.A and K.g_sw(K.TWO_THIRDS) == K.ZERO
    # N is the curve's only point of order two, so 2/3 is the only root of g
    assert not K.is_square(K.sub(K.sqr(K.A), K.scale(K.B, 4)))
    assert not K.is_square(K.Z_SW) and not K.is_square(K.B)
    assert K.decode(K.ZERO) == K.N and K.to_weierstrass(K.N) == K.NEUTRAL_WEI.tolist()


@pytest.mark.parametrize("i", range(len(K.SUM_LABELS)), ids=lambda i: K.SUM_LABELS[i].replace(" ", "_"))
def test_sum_cases_oracle_equals_exact(i):
    label, pts = K.sum_cases()[i]
    orc = K.orc_sum(pts)
    assert same(K.exact_sum(pts), orc), label
    if "inverse pairs only" in label:
        assert np.array_equal(orc[0], K.NEUTRAL_W) and np.array_equal(orc[1], K.NEUTRAL_WEI)


def test_sum_cases_hold_what_they_say():
    cases = dict(K.sum_cases())
    assert [len(cases[k]) for k in ("P,P", "P,P,P", "128xP", "129xP")] == [2, 3, 128, 129]
    planted = [k for k in cases if k.startswith("P,-P at lanes")]
    assert len(planted) == 14
    dist = set()
    for k in planted:
        pts = cases[k]
        rows = {tuple(r): a for a, r in enumerate(pts.tolist()) if any(r)}
        pairs = [(a, rows[tuple(K.negate(pts[a]).tolist())]) for a in range(128) if pts[a].any() and tuple(K.negate(pts[a]).tolist()) in rows]
        pairs = [(a, b) for a, b in pairs if a < b]
        assert len(pts) == 128 and len(pairs) == 1 and pairs[0][0] < pairs[0][1] - pairs[0][0]  # t < s: they meet at level s
        dist.add(pairs[0][1] - pairs[0][0])
        assert int((~pts.any(axis=1)).sum()) == (126 if "neutral" in k else 0)
    assert dist == {1, 2, 4, 8, 16, 32, 64}
    big = cases["256: block 0 cancels, block 1 random"]
    assert len(big) == 256 and np.array_equal(K.orc_sum(big[:128])[0], K.NEUTRAL_W) and K.orc_sum(big[128:])[0].any()
    assert np.array_equal(K.orc_sum(big)[0], K.orc_sum(big[128:])[0])
    for name, i in (("first", 0), ("middle", 64), ("last", 128)):
        pts = cases["129: encoding 0 at the %s index" % name]
        assert len(pts) == 129 and [j for j in range(129) if not pts[j].any()] == [i]
    # every point of every case decodes
    for label, pts in K.sum_cases():
        assert all(K.orc_valid(w) for w in pts), label


def test_range_cases_oracle_equals_exact():
    pts, ranges = K.range_cases()
    assert pts.shape == (200, 5) and {int(hi - lo) for lo, hi in ranges} >= set(K.RANGE_LENGTHS)
    assert all(lo <= hi <= 200 for lo, hi in ranges)
    neutral = 0
    for lo, hi in ranges:
        orc = K.orc_sum(pts[lo:hi])
        assert same(K.exact_sum(pts[lo:hi]), orc), (lo, hi)
        neutral += not orc[0].any()
    assert neutral == 3 + 2  # the empty ranges and the two that hold only P, -P
    inverse = [(i, j) for i in range(200) for j in range(i + 1, 200) if np.array_equal(pts[j], K.negate(pts[i]))]
    equal = [(i, j) for i in range(200) for j in range(i + 1, 200) if np.array_equal(pts[j], pts[i])]
    assert inverse == [(20, 21), (30, 94), (40, 72), (84, 85), (150, 151)] and equal == [(10, 11), (100, 101)]


def test_scalar_cases_oracle_equals_exact():
    pts, ks = K.scalar_cases()
    want_w, want_wei = K.scalar_expected()
    assert len(ks) == pts.shape[0] == max(K.SCALAR_COUNTS) and all(0 <= k < 1 << 128 for k in ks)
    p = K.base_points(1)[0]
    assert ks[:34] == list(range(34)) and all(np.array_equal(w, p) for w in pts[:34])
    assert ks[34:68] == list(range(34)) and all(np.array_equal(w, K.negate(p)) for w in pts[34:68])
    assert ks[68:73] == [9 << 28, 9 << 60, 9 << 92, 9 << 124, (1 << 128) - 1]
    assert not pts[73:77].any() and all(ks[73:77]) and not want_w[73:77].any() and (want_wei[73:77] == K.NEUTRAL_WEI).all()
    assert len(K.SCALAR_EXACT) == 8
    for i in K.SCALAR_EXACT:
        assert same(K.exact_scalar_mul(pts[i], ks[i]), (want_w[i], want_wei[i])), i
    # k (-P) = -(k P), and the small multiples are distinct points
    assert np.array_equal(want_w[34:68], K.negate(want_w[:34]))
    assert len({tuple(w) for w in want_w[:34].tolist()}) == 34


def test_multiplicity_shortcut_equals_the_plain_sum():
    for label, pts, terms in K.big_sum_cases():
        assert sum(m for _, m in terms) == len(pts)
        if label == "16385":
            short, plain = K.big_sum_expected(terms), K.orc_sum(pts)
            assert np.array_equal(short[0], plain[0]) and np.array_equal(short[1], plain[1]) and plain[0].any()
        if "P,-P" in label:
            i, j = K.BIG_PLANT, K.BIG_PLANT + K.BIG_LANE_STRIDE
            assert j < len(pts) and pts[i].any() and np.array_equal(pts[j], K.negate(pts[i]))
            assert (i % K.BIG_LANE_STRIDE) == (j % K.BIG_LANE_STRIDE)  # the same lane of sum_kernel's capped grid


@pytest.fixture(scope="module")
def swu_traces():
    return [K.simple_swu_trace(K.el(u)) for u in K.swu_inputs()]


def test_swu_inputs_oracle_equals_exact(swu_traces):
    u = K.swu_inputs()
    assert u.shape == (278, 5) and (u < np.uint64(P)).all() and not u[21].any() and (u[20] == np.uint64(P - 1)).all()
    ow, owei = K.orc_swu(u[:64])
    for i in range(64):
        pt = swu_traces[i][0]
        assert list(K.encode(pt)) == ow[i].tolist() and K.to_weierstrass(pt) == owei[i].tolist(), i


def test_swu_inputs_reach_every_branch(swu_traces):
    """the counts are of the exact reference's own decisions; a seed that falls short is changed in ec_cases.SWU_SEED"""
    facts = [f for _, f in swu_traces]
    combos = {(a, b): sum(f["gx1_square"] == a and f["x_cand_square"] == b for f in facts) for a in (True, False) for b in (True, False)}
    flips = sum(f["flip"] for f in facts)
    print("simple_swu branches (g(x1) square, x_cand square):", combos, "sgn0 differs:", flips, "agrees:", len(facts) - flips)
    assert min(combos.values()) >= 8
    assert flips >= 8 and len(facts) - flips >= 8
    assert not any(f["degenerate"] for f in facts)
    # the sgn0 ladder: leading zero limbs with an odd and an even first non-zero limb, at every position
    u = K.swu_inputs()[:20]
    assert [K.sgn0(K.el(r)) for r in u] == [1, 0, 0, 1] * 5 and [int((r != 0).argmax()) for r in u] == [i // 4 for i in range(20)]


def test_degenerate_branch_of_simple_swu_is_unreachable():
    """simple_swu falls back to the general decode when w = 0 or x_cand = 0. Both need X = 2/3, the only root of g (w = Y / x_cand
    with Y^2 = g(X)). With t = Z u^2 and m = (2/3) / (-B/A): x1 = 2/3 means t^2 + t - 1 / (m - 1) = 0 and x2 = t x1 = 2/3 means
    t^2 + (1 - m) t + (1 - m) = 0. Neither quadratic has a square discriminant, so neither has a root in the field. The
    denominator t^2 + t = t (t + 1) is zero only for u = 0: t = -1 needs u^2 = -1 / Z, a non-square. u = 0 takes the constant x1,
    which is not 2/3 either. So nobody needs to look for an input to that branch."""
    m = K.mul(K.TWO_THIRDS, K.inv(K.NEG_B_DIV_A))
    one_minus_m = K.sub(K.ONE, m)
    c1 = K.neg(K.inv(K.sub(m, K.ONE)))
    disc1 = K.sub(K.ONE, K.scale(c1, 4))                          # 1 - 4 c, c = -1 / (m - 1)
    disc2 = K.sub(K.sqr(one_minus_m), K.scale(one_minus_m, 4))    # (1 - m)^2 - 4 (1 - m)
    assert not K.is_square(disc1) and not K.is_square(disc2)
    assert not K.is_square(K.NEG_Z_INV) and K.mul(K.NEG_Z_INV, K.Z_SW) == K.neg(K.ONE)
    # the equations are the right ones: a root of either quadratic in an extension would give x = 2/3 -- checked the other way
    # round, on a field element t: x1(t) = 2/3 exactly when the first quadratic vanishes at t
    t = K.el(O.rand_field(5, 0xEC12))
    x1 = K.mul(K.add(K.inv(K.add(K.sqr(t), t)), K.ONE), K.NEG_B_DIV_A)
    q1 = K.add(K.add(K.sqr(t), t), c1)
    assert K.sub(x1, K.TWO_THIRDS) == K.mul(K.mul(q1, K.inv(K.add(K.sqr(t), t))), K.mul(K.NEG_B_DIV_A, one_minus_m))
    q2 = K.add(K.add(K.sqr(t), K.mul(one_minus_m, t)), one_minus_m)
    assert K.sub(K.mul(t, x1), K.TWO_THIRDS) == K.mul(K.mul(q2, K.inv(K.add(t, K.ONE))), K.NEG_B_DIV_A)
    # u = 0
    pt, facts = K.simple_swu_trace(K.ZERO)
    assert not facts["degenerate"] and K.mul(K.NEG_Z_INV, K.NEG_B_DIV_A) != K.TWO_THIRDS and pt != K.N


def test_refusal_inputs():
    bad = K.bad_encodings(4)
    assert (bad < np.uint64(P)).all() and not any(K.orc_valid(w) for w in bad) and all(K.decode(K.el(w)) is None for w in bad)
    assert all(K.orc_valid(w) for w in K.refusal_batch()) and K.refusal_batch().shape == (300, 5)
    non = K.NONCANONICAL
    assert non.shape == (16, 5) and ((non >= np.uint64(P)).sum(axis=1) == 1).all()
    assert sorted({int(x) for x in non[non >= np.uint64(P)]}) == [P, P + 5, K.U64_MAX]
    assert non[15].tolist() == [P, 0, 0, 0, 0]
    assert {int((r >= np.uint64(P)).argmax()) for r in non[:15]} == {0, 1, 2, 3, 4}
