"""Host-side parts of the device verifier that need no GPU: the proof store's verified read, the proof-word layout, and the number
of line points T the verifier evaluates a gate table at."""
import importlib

import pytest

import circuits as C

PS = importlib.import_module("mapreduce-plonky2_amd.proofstore")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")


def test_get_proof_verified(tmp_path):
    store = PS.ProofStore(str(tmp_path))
    key, missing = PS.ProofKey.row("t", 3, "k"), PS.ProofKey.row("t", 4, "k")
    store.store_proof(key, b"proof bytes")
    seen = []
    assert store.get_proof_verified(key, lambda b: seen.append(b) or 0) == b"proof bytes"
    assert seen == [b"proof bytes"]
    with pytest.raises(ValueError) as e:
        store.get_proof_verified(key, lambda b: 3)
    assert key.canonical() in str(e.value) and "status 3" in str(e.value)
    with pytest.raises(KeyError) as e1:
        store.get_proof_exact(missing)
    with pytest.raises(KeyError) as e2:
        store.get_proof_verified(missing, lambda b: 0)
    assert str(e1.value) == str(e2.value)
    assert store.get_proof_exact(key) == b"proof bytes"  # unchanged: no check


SHAPES = [(5, "ALL_KINDS", False), (6, "ALL_KINDS", False), (12, "ALL_KINDS", False), (7, "ALL_KINDS", True), (12, "VERIFIER_KINDS", False),
          (13, "LEAF_KINDS", False)]


@pytest.mark.parametrize("log_n,kinds,lookups", SHAPES)
def test_proof_word_layout(mp2, log_n, kinds, lookups):
    """public inputs | caps of oracles 1..3 | openings | FRI words, from FriParams alone (no circuit is built: the widths are those of
    the circuits of the GPU tests -- 6 / 5 / 4 selectors + 2 gate constants (+ 6 lookup selectors) + 80 sigmas)"""
    sel = {"ALL_KINDS": 6, "LEAF_KINDS": 5, "VERIFIER_KINDS": 4}[kinds]
    nlp = C.NUM_LOOKUP_POLYS if lookups else 0
    fp = mp2.standard_recursion_params(log_n, (sel + (6 if lookups else 0) + 2 + 80, 135, 2 * (10 + nlp), 16), num_lookup_polys=nlp)
    assert fp.n_layers == {5: 0, 6: 1, 7: 1, 12: 2, 13: 2}[log_n]
    for n_pi in (mp2.PI_HASH_GIVEN, 0, 9):
        parts = mp2.verifier_part_words(fp, n_pi)
        assert parts == [4 if n_pi == mp2.PI_HASH_GIVEN else n_pi, 3 * 64, 2 * fp.n_openings, fp.proof_words]
    assert fp.n_openings == sum(fp.oracle_w[i] for i in range(4)) + 2 + 2 * nlp


def line_points(gates, num_selectors):
    """the rule restated: 1 + the largest filtered degree = gate degree + (selector group size - 1) + (1 when num_selectors > 1)"""
    return 1 + max(C.gate_degree(g) + (g.group_end - g.group_start - 1) + (1 if num_selectors > 1 else 0) for g in gates)


@pytest.mark.parametrize("kinds,lookups,want", [("ALL_KINDS", False, 10), ("ALL_KINDS", True, 10), ("LEAF_KINDS", False, 10), ("VERIFIER_KINDS", False, 9)])
def test_line_points(mp2, kinds, lookups, want):
    luts = [(t, 100) for t in C.bits_lookup_tables()] if lookups else None
    ckt = C.build(7 if lookups else 5, getattr(C, kinds) + (C.LOOKUP_KINDS if lookups else []), 3, luts=luts)
    assert line_points(ckt.gates, ckt.num_selectors) == want
    assert mp2.gate_table_line_points(ckt.gates, ckt.num_selectors) == want


def test_line_points_of_a_single_gate(mp2):
    for kind, p0, p1 in ((C.ARITHMETIC, 20, 0), (C.POSEIDON2, 0, 0), (C.BASE_SUM, 20, 4)):
        g = mp2.Gate(kind, p0, p1, 0, 0, 0, 1)
        assert mp2.gate_table_line_points([g], 1) == C.gate_degree(g) + 1
    assert mp2.gate_table_line_points([mp2.Gate(99, 0, 0, 0, 0, 0, 1)], 1) == 0  # unknown kind
