"""The operand tables of tests/mul_carry_cases.py, without a GPU: the model of gl_mulw_k's columns reproduces the exact product, the tables
put the middle accumulator on both sides of 2^64 and at its ends, every column bound that the routine's comment states is attained by
some operand and exceeded by none, and the comment itself states those bounds."""
import os
import re

import field_cases as F
import mul_carry_cases as C

M, M64 = C.M, C.M64


def _pair_list():
    a, b = C.pairs(n_uniform=4096)
    return list(zip(a.tolist(), b.tolist()))


def test_model_is_the_exact_product():
    for a, b in _pair_list():
        col = C.columns(a, b)
        assert col["lo"] + (col["hi"] << 64) == a * b
        assert col["lo"] <= M64 and col["hi"] <= M64
    a, b, c = C.triples(n_uniform=4096)
    for x, y, z in zip(a.tolist(), b.tolist(), c.tolist()):
        col = C.columns_add(x, y, z)
        assert col["lo"] + (col["hi"] << 64) == x * y + z
        assert col["lo"] <= M64 and col["hi"] <= M64


def test_accumulator_on_both_sides_of_2p64():
    at = C.columns(*C.ACC_EXACTLY_2P64)
    assert at["m2"] == 1 << 64 and at["k"] == 1 and at["q"] == 0
    below = C.columns(*C.ACC_JUST_BELOW)
    assert below["m2"] == (1 << 64) - 2 and below["k"] == 0
    top = C.columns(*C.ACC_MAXIMUM)
    assert top["m2"] == C.BOUND_M2 and top["k"] == 1
    assert C.columns(0, 0)["m2"] == 0
    ks = [C.columns(a, b)["k"] for a, b in _pair_list()]
    assert set(ks) == {0, 1}
    carry_ks = [C.columns(a, b)["k"] for a, b in C.CARRY_PAIRS]
    assert carry_ks.count(0) >= 3 and carry_ks.count(1) >= 3, "the hand-made pairs alone take both branches: 2^64 itself, above it, the maximum"
    lattice_ks = ks[len(C.CARRY_PAIRS):len(C.CARRY_PAIRS) + 49 * 49]
    assert lattice_ks.count(1) >= 100 and lattice_ks.count(0) >= 100


def test_column_bounds_attained_and_respected():
    cols = [C.columns(a, b) for a, b in _pair_list()]
    for name, bound in (("P", C.BOUND_P), ("m1", C.BOUND_M1), ("m2", C.BOUND_M2), ("hi", C.BOUND_HI)):
        assert max(c[name] for c in cols) == bound, name
    assert C.BOUND_M1 == (1 << 64) - (1 << 32) - 1 and C.BOUND_M1 < 1 << 64, "m1 fits its register pair"
    assert C.BOUND_M2 < 1 << 65, "the accumulator carries one bit at most"
    assert all(c["k"] in (0, 1) and c["q"] <= M64 for c in cols)
    a, b, c = C.triples(n_uniform=4096)
    adds = [C.columns_add(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())]
    assert max(t["P"] for t in adds) == C.BOUND_ADD_P == (1 << 64) - (1 << 32)
    assert max(t["m1"] for t in adds) == C.BOUND_ADD_M1 == M64
    assert all(t["m2"] <= M64 for t in adds)
    at = C.columns_add(*C.ADD_COLUMNS_AT_BOUND)
    assert at["P"] == C.BOUND_ADD_P and at["m1"] == C.BOUND_ADD_M1


def test_tables_hold_what_the_gpu_test_counts_on():
    a, b = C.pairs()
    assert len(a) == len(C.CARRY_PAIRS) + 49 * 49 + C.N_UNIFORM
    x, y, z = C.triples()
    assert len(x) == len(y) == len(z) == len(C.ADD_CASES) + len(a)
    for v in (F.P - 1, F.P, F.P + 1, 0, M64):
        assert any(v in pr for pr in C.CARRY_PAIRS)


def test_comment_states_the_bounds():
    src = open(os.path.join(F.CSRC, "gl.cuh")).read()
    body = src[src.index("// gl_mulw for the S-boxes"):src.index("GLHD u64 gl_mulw_k")]
    flat = re.sub(r"\s+", " ", body.replace("//", " "))
    for text, value in (("M^2 = 2^64 - 2^33 + 1", C.BOUND_P), ("M^2 + M - 1 = 2^64 - 2^32 - 1", C.BOUND_M1), ("M^2 + 2 M - 1 = 2^64 - 2", C.BOUND_HI)):
        assert text in flat, text
        lhs, rhs = text.split(" = ", 1)
        ev = lambda s: eval(s.replace("^", "**").replace("2 M", "2*M"), {"M": M})
        assert ev(lhs) == ev(rhs) == value
    assert "2 M^2 + M - 1 < 2^65" in flat and 2 * M * M + M - 1 == C.BOUND_M2
