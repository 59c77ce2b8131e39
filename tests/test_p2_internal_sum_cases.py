"""The states of tests/p2_internal_sum_cases.py, without a GPU: the model of the device's limb sum (p2_limb_sum, csrc/poseidon.cuh)
reproduces the exact sum on every state, the structured rows reach every value of the low words' carry and of the top word in 0..11,
put the subtract that recovers the carry on both sides of its wrap and the high words at their maximum; the portable body of
p2_internal (the host harness of tests/test_field_host.py) agrees with exact Python integers on the same rows; and the routine's
comment states the bounds the model finds."""
import os
import re

import field_cases as F
import field_checks as C
import p2_internal_sum_cases as S
from test_field_host import H, exe  # noqa: F401  (fixtures: the host program and its back end)

M32, M64 = S.M32, S.M64


def _structured_models():
    return [(label, st, S.model(st)) for label, st in S.structured()]


def test_model_is_the_exact_sum():
    for st in S.states(n_uniform=4096).tolist():
        m = S.model(st)
        assert m["W"] + (m["top"] << 64) == sum(st)
        assert m["c"] == sum(x & M32 for x in st) >> 32
        assert m["c"] <= 11 and m["top"] <= 11 and m["H"] <= 12 * M32


def test_structured_rows_reach_every_carry_and_top_word():
    ms = _structured_models()
    full = [m for label, _, m in ms if label.endswith("limbs 2^64-1")]
    assert [m["top"] for m in full] == [0, 0] + list(range(1, 12))
    low = [m for label, _, m in ms if label.endswith("limbs 2^32-1")]
    assert [m["c"] for m in low] == [0, 0] + list(range(1, 12)) and all(m["H"] == 0 and m["top"] == 0 for m in low)
    counts_c = {v: sum(1 for _, _, m in ms if m["c"] == v) for v in range(12)}
    counts_top = {v: sum(1 for _, _, m in ms if m["top"] == v) for v in range(12)}
    assert all(counts_c[v] >= 2 for v in range(12)), counts_c
    assert all(counts_top[v] >= 2 for v in range(12)), counts_top
    top_h = [m for label, _, m in ms if label == "all high words full"]
    assert len(top_h) == 1 and top_h[0]["H"] == 12 * M32 and top_h[0]["c"] == 0 and top_h[0]["top"] == 11


def test_carry_subtract_on_both_sides_of_its_wrap():
    for total in (M32, M32 + 1):
        ms = [m for label, _, m in _structured_models() if label == "H = %#x" % total]
        assert len(ms) == 12 and all(m["H"] == total for m in ms)
        assert {0, 1, 11} <= {m["c"] for m in ms}
    at = [m for label, _, m in _structured_models() if label == "H = %#x" % M32]
    assert any(m["wraps"] for m in at) and any(not m["wraps"] for m in at), "lo32(H) = 2^32 - 1: the subtract wraps for every c > 0"
    assert all(m["wraps"] == (m["c"] > 0) for m in at)
    over = [m for label, _, m in _structured_models() if label == "H = %#x" % (M32 + 1)]
    assert not any(m["wraps"] for m in over) and {m["top"] for m in over} == {1}
    assert {m["top"] for m in at if m["c"] > 0} == {1} and {m["top"] for m in at if m["c"] == 0} == {0}


def test_tables_hold_what_the_gpu_test_counts_on():
    st = S.states()
    assert st.shape == (len(S.structured()) + 12 * len(F.EANY) + S.N_UNIFORM, 12)
    lat = S.lattice_rows().tolist()
    for i in range(12):
        assert {r[i] for r in lat[i * len(F.EANY):(i + 1) * len(F.EANY)]} == set(F.EANY)
    rows = [s for _, s in S.structured()]
    for v in (F.P - 1, F.P, F.P + 1):
        assert [v] * 12 in rows and all([v if j == i else 0 for j in range(12)] in rows for i in range(12))


def test_portable_body_on_the_same_rows(H):  # noqa: F811
    states, want = S.reference(n_uniform=4096)
    C.assert_weak_rows(H, "p2_internal (host)", H.vec("p2_internal", states)[0], want, states)


def test_comment_states_the_bounds():
    src = open(os.path.join(F.CSRC, "poseidon.cuh")).read()
    body = src[src.index("// The sum S of the twelve limbs"):src.index("GLD u64 p2_limb_sum")]
    flat = re.sub(r"\s+", " ", body.replace("//", " "))
    for text in ("c = L >> 32 <= 11", "T = H + c <= 12 M + 11", "T >> 32 <= 11", "c = (hi32(W) - lo32(H)) mod 2^32"):
        assert text in flat, text
    assert (12 * M32 + 11) >> 32 == 11 and (12 * M32) >> 32 == 11
