"""The forged proofs of forged_fri_cases.py on the CPU oracle alone: the oracle's verifier gives the predicted first failing check
for every case, the tamper hook is one-shot, and the list reaches what the device test (test_gpu_forged_proofs.py) is there for --
the final-polynomial check, every layer's consistency check, the check after a tampered layer, accepted forgeries, and cases a
verifier that ordered its failures position-major would get wrong. The reach conditions are conditions on the inputs: the device
test cannot lose them without this file failing."""
import numpy as np
import pytest

import circuits as C
import forged_fri_cases as FF
import fri_param_cases as FC
import oracle as O

IDS = [s.name for s in FF.SHAPES]


def oracle_status(shape, f):
    ckt = FF.circuit(shape)
    return int(C.verify(ckt, FF.params(shape), FF.digest(), ckt.pi_hash, f.caps, f.openings, f.proof))


def test_shapes_are_the_ones_named():
    by = {s.name: FF.params(s) for s in FF.SHAPES}
    assert len(by) == len(FF.SHAPES) == 10
    assert FF.layers(by["std5"]) == [] and FF.layers(by["std6"]) == [4]
    assert (by["std6"].pow_bits, by["std6"].num_queries, by["std6"].cap_height) == (16, 28, 4)
    assert FF.layers(by["all6_arity2-v0"]) == FF.layers(by["all6_arity2-v1"]) == [2, 2]
    assert FF.layers(by["all6_arity1"]) == [1, 1, 1] and FF.layers(by["all7_arity3"]) == [3]
    assert FF.layers(by["all5_cap_is_tree"]) == [] and FF.layers(by["lookup7_arity2"]) == [2, 2]
    assert FF.layers(by["all7_mixed-v0"]) == FF.layers(by["all7_mixed-v1"]) == [3, 2, 1]
    assert {s.variant for s in FF.SHAPES if s.name.startswith(("all6_arity2", "all7_mixed"))} == {0, 1}
    assert by["lookup7_arity2"].num_lookup_polys > 0 and FF.circuit(next(s for s in FF.SHAPES if s.name == "lookup7_arity2")).luts


def test_plans_and_layout():
    """the plans of a layer by hand, and the layout against the oracle's proof size"""
    assert FF.plans(16, 4) == [(0, 16, 1), (0, 4, 4), (1, 4, 4), (3, 4, 4), (0, 4, 1), (4, 4, 1), (12, 4, 1), (0, 8, 1), (8, 8, 1), (5, 1, 1), (15, 1, 1)]
    assert len(FF.plans(512, 2)) == 10  # places 1 and arity - 1 are one plan
    for s in FF.SHAPES:
        fp = FF.params(s)
        L = FF.layout(fp)
        assert L.final_off + 2 * FF.final_len(fp) + 1 == FC.proof_sizes(fp)[0], s.name
        assert L.n_sib[0] == FC.n_siblings(fp)[0] and L.n_sib[fp.n_oracles:] == FC.n_siblings(fp)[1:]


def test_the_hook_is_one_shot_and_guarded():
    """an honest proof made right after a forged one is the honest proof made before it; a hook that names nothing the proof
    has changes nothing and says so"""
    shape = FF.SHAPES[2]
    ckt, fp = FF.circuit(shape), FF.params(shape)
    before = C.prove(ckt, fp, FF.digest())[:3]
    O.set_fri_tamper(0, 3, 5, 7, (1, 2))
    forged = C.prove(ckt, fp, FF.digest())[:3]
    assert O.fri_tamper_applied() == 5
    after = C.prove(ckt, fp, FF.digest())[:3]
    assert O.fri_tamper_applied() == 5, "an unarmed proof must leave the count of the last consumed hook alone"
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(a, b) for a, b in zip(before, FF.honest(shape)))
    assert all(np.array_equal(a, b) for a, b in zip(before[:2], forged[:2])) and not np.array_equal(before[2], forged[2])
    for stage, first in ((0, FF.layer_len(fp, 0)), (fp.n_layers, FF.final_len(fp)), (fp.n_layers + 1, 0)):
        O.set_fri_tamper(stage, first, 4, 1, (1, 1))
        noop = C.prove(ckt, fp, FF.digest())[:3]
        assert O.fri_tamper_applied() == 0, (stage, first)
        assert all(np.array_equal(a, b) for a, b in zip(before, noop)), (stage, first)
    # positions past the end of the layer are skipped, the ones before it are changed
    O.set_fri_tamper(0, FF.layer_len(fp, 0) - 2, 5, 1, (0, 1))
    C.prove(ckt, fp, FF.digest())
    assert O.fri_tamper_applied() == 2


@pytest.mark.parametrize("shape", FF.SHAPES, ids=IDS)
def test_oracle_verifier_agrees_with_the_prediction(shape):
    fp = FF.params(shape)
    ckt = FF.circuit(shape)
    hc, ho, hp = FF.honest(shape)
    assert C.verify(ckt, fp, FF.digest(), ckt.pi_hash, hc, ho, hp) == 0
    assert FF.query_indices(shape, hc, ho, hp) == FF.query_indices(shape, hc, ho, hp.copy()) and len(FF.query_indices(shape, hc, ho, hp)) == fp.num_queries
    cat = FF.catalogue(shape)
    bad = []
    for f in cat:
        got, want = oracle_status(shape, f), FF.status(f.fails)
        assert np.array_equal(f.caps, hc) and np.array_equal(f.openings, ho), "a forged proof differs from the honest one outside FRI"
        if got != want or (got != 0) != bool(f.fails):
            bad.append((FF.label(f), got, f.fails[:1]))
    t = FF.tally(shape)
    print(shape.name, "layers", FF.layers(fp), t)
    assert not bad, f"(plan, delta, bump), oracle, predicted: {bad[:10]}"

    # ---- what the shape must reach (by the oracle alone: the statuses above are the oracle's)
    plain = [f for f in cat if f.bump is None]
    n = fp.n_layers
    assert any(f.case.stage == n and f.fails[0] == (0, 1 + 2 * n, 5) for f in plain), "code 5 from the final stage"
    assert all(FF.status(f.fails) == 5 for f in plain if f.case.stage == n)
    for li in range(n):
        assert any(f.case.stage == li and f.fails and f.fails[0][1:] == (1 + 2 * li, 3) for f in plain), f"layer {li}: code 3 at its own check"
    if n:
        nxt = [f for f in plain if f.case.stage < n and f.fails and f.fails[0][1] == 1 + 2 * (f.case.stage + 1)]
        assert nxt, "no case whose first failure is the check after the tampered layer"
        assert any(f.fails[0][2] == 5 for f in nxt), "no wrong fold caught by the final polynomial"
        assert n == 1 or any(f.fails[0][2] == 3 for f in nxt), "no wrong fold caught by the next layer"
        assert any(not f.fails for f in plain), "no accepted forgery"
        if fp.num_queries >= 5:
            assert t["order_sensitive"] >= 1, "no case that tells a query-major minimum from a position-major one"
            assert t["first_failure_past_query_0"] >= 1
            kinds = {f.bump[0] for f in cat if f.bump}
            assert {"initial path of the query before", "initial path of the query after"} <= kinds
            assert any(f.bump and FF.status(f.fails) == 2 for f in cat)


def test_catalogue_reach_in_all():
    ts = [FF.tally(s) for s in FF.SHAPES]
    assert sum(t["order_sensitive"] for t in ts) >= 20
    assert sum(t["first_failure_past_query_0"] for t in ts) >= 20
    codes = set().union(*(t["codes"] for t in ts))
    assert codes == {0, 2, 3, 4, 5}
    cats = [f for s in FF.SHAPES for f in FF.catalogue(s)]
    kinds = {f.bump[0] for f in cats if f.bump}
    assert kinds == {"initial path of the query before", "initial path of the query after", "the failing layer's own path", "an earlier layer's path"}
    # a bump after the failing check, or in a later query, changes nothing; one before it takes the report over
    by_kind = {k: {FF.status(f.fails) for f in cats if f.bump and f.bump[0] == k} for k in kinds}
    assert by_kind["initial path of the query before"] == {2} and by_kind["an earlier layer's path"] == {4}
    assert by_kind["initial path of the query after"] <= {3, 5} and by_kind["the failing layer's own path"] == {3}
    print("all shapes:", sum(t["cases"] for t in ts), "cases,", sum(t["order_sensitive"] for t in ts), "order-sensitive,",
          sum(t["first_failure_past_query_0"] for t in ts), "with the first failure past query 0")
