"""The parameter cases of fri_param_cases.py on the CPU oracle alone: it proves each, accepts its own proof and rejects every
mutation of the case's catalogue -- the reference is sound at these parameters before any device result is compared with it -- and
the list reaches every branch the device tests are there for. The last is a condition on the inputs: the device tests cannot shrink
without this file failing."""
import ctypes

import pytest

import circuits as C
import fri_param_cases as FC
import oracle as O


def test_cases_reach_every_branch():
    fps = [FC.pcs_params(c) for c in FC.PCS_CASES] + [C.oracle_params(FC.circuit(c.log_n, c.kinds), **dict(c.kw)) for c in FC.CIRCUIT_CASES]
    arities = {fp.arity_bits[i] for fp in fps for i in range(fp.n_layers)}
    assert arities == {1, 2, 3, 4}
    assert any(s == 0 for fp in fps for s in FC.n_siblings(fp)[1:]), "no FRI layer whose cap is its leaf digests"
    assert any(FC.n_siblings(fp)[0] == 0 for fp in fps), "no initial tree whose cap is its leaf digests"
    assert {0, 8} <= {fp.n_layers for fp in fps}
    assert any(len({fp.arity_bits[i] for i in range(fp.n_layers)}) > 1 for fp in fps), "no layers of unequal arity"
    assert {1, 8} <= {fp.n_oracles for fp in fps}
    assert any(fp.zs_count == 0 for fp in fps)
    assert {0, 1, 64} <= {fp.num_queries for fp in fps}
    assert {1, 2, 3, 4, 5, 6} <= {fp.rate_bits for fp in fps}
    assert {0, 1} == {c.variant for c in FC.PCS_CASES if c.name.startswith(("cap", "arity"))}
    assert max(fp.log_n for fp in fps) >= 14
    assert len({c.name for c in FC.PCS_CASES}) == len(FC.PCS_CASES)
    # every case the batched device test proves exists under the name that test selects by
    assert {c.name for c in FC.PCS_CASES if c.batched} == {"cap0-v0", "cap0-v1", "eight_layers-v0", "mixed-v0", "eight_oracles-v0", "two_pass14-v0"}
    # circuits: every arity below 4, a cap as tall as the tree, the lookup polynomials
    cfps = fps[len(FC.PCS_CASES):]
    assert {1, 2, 3} <= {fp.arity_bits[i] for fp in cfps for i in range(fp.n_layers)}
    assert any(fp.cap_height == fp.log_n + fp.rate_bits for fp in cfps) and any(fp.num_lookup_polys for fp in cfps)
    assert all(fp.rate_bits == 3 for fp in cfps)


def test_layer_structures():
    """the shapes the cases are named for (ConstantArityBits by hand) and three proof sizes (counted by hand from the layout)"""
    by = {c.name: FC.pcs_params(c) for c in FC.PCS_CASES}
    layers = lambda fp: [fp.arity_bits[i] for i in range(fp.n_layers)]
    assert layers(by["arity1-v0"]) == [1, 1, 1, 1] and layers(by["arity2-v0"]) == [2, 2] and layers(by["arity3-v1"]) == [3, 3]
    assert layers(by["eight_layers-v0"]) == [1] * 8 and layers(by["mixed-v0"]) == [4, 3, 2, 1]
    assert layers(by["cap7-v0"]) == [] and layers(by["cap10-v0"]) == [] and layers(by["tiny1-v0"]) == [] and layers(by["tiny2-v0"]) == []
    assert layers(by["final0-v0"]) == [4, 4] and layers(by["final7-v0"]) == [4] and layers(by["rate1-v0"]) == [4]
    assert FC.n_siblings(by["rate1-v0"]) == [4, 0] and FC.n_siblings(by["cap10-v0"]) == [0]
    assert FC.proof_sizes(by["eight_layers-v0"])[0] == 1380
    assert FC.proof_sizes(by["mixed-v0"])[0] == 1006
    assert FC.proof_sizes(by["queries64-v0"])[0] == 10129
    # no queries: layer caps, final polynomial, PoW witness
    assert FC.proof_sizes(by["queries0-v0"])[0] == 1 * (4 << 4) + 2 * (1 << 3) + 1


def check_mutations(fp, verify, caps, openings, proof, cap_stride=5):
    """every catalogue entry is rejected. With no queries the PoW response is the verifier's only check, and a changed transcript
    passes it with probability 2^-pow_bits: there a mutation ends in 0 or 1 and nothing more can be asked of any verifier."""
    cat = FC.catalogue(fp, openings.shape[0], proof.size, cap_stride)
    assert {"openings", "fri"} <= {part for part, _ in cat} and (fp.n_oracles == 1 or ("caps", 4 << fp.cap_height) in cat)
    tally = {}
    for part, idx in cat:
        st = verify(*FC.mutated(caps, openings, proof, part, idx))
        tally[st] = tally.get(st, 0) + 1
        if fp.num_queries == 0:
            assert st in (0, 1), (part, idx, st)
        else:
            assert st != 0, f"the oracle accepts the proof with {part}[{idx}] changed"
    return tally


@pytest.mark.parametrize("case", FC.PCS_CASES, ids=[c.name for c in FC.PCS_CASES])
def test_oracle_pcs_case(case):
    fp, vals, cd, ph, caps, openings, proof = FC.pcs_oracle(case)
    words, n_open = FC.proof_sizes(fp)
    assert proof.shape == (words,) and openings.shape == (n_open, 2) and n_open == sum(case.ws) + fp.zs_count
    assert O.pcs_verify(fp, cd, ph, caps, openings, proof) == 0
    assert proof.max() < O.P and caps.max() < O.P and openings.max() < O.P
    # a cap word is bound through the transcript wherever it lies: at least 16 per cap, every 5th while the cap is small (the
    # circuit cases, which the device verifier is compared on, keep every 5th throughout)
    stride = max(5, (4 << fp.cap_height) // 16 + 1)
    tally = check_mutations(fp, lambda c, o, p: O.pcs_verify(fp, cd, ph, c, o, p), caps, openings, proof, stride)
    print(case.name, "layers", [fp.arity_bits[i] for i in range(fp.n_layers)], "words", words, "mutations", tally)


@pytest.mark.parametrize("case", FC.CIRCUIT_CASES, ids=[c.name for c in FC.CIRCUIT_CASES])
def test_oracle_circuit_case(case):
    ckt = FC.circuit(case.log_n, case.kinds)
    fp = C.oracle_params(ckt, **dict(case.kw))
    cd = O.rand_field(4, 0xD16E57)  # any digest: the oracle takes the verifier data as given
    caps, openings, proof, _ = C.prove(ckt, fp, cd)
    assert C.verify(ckt, fp, cd, ckt.pi_hash, caps, openings, proof) == 0
    tally = check_mutations(fp, lambda c, o, p: int(C.verify(ckt, fp, cd, ckt.pi_hash, c, o, p)), caps, openings, proof)
    print(case.name, "layers", [fp.arity_bits[i] for i in range(fp.n_layers)], "words", proof.size, "mutations", tally)


def test_oracle_reduction_rule_is_total():
    """orc_reduction_arity_bits over the whole grid: it returns (no wrap of the u32, nothing past out[8]) and is plonky2's
    ConstantArityBits loop wherever that loop neither asserts nor gives more than 8 layers"""
    out = (ctypes.c_uint32 * 9)()
    f = O.lib().orc_reduction_arity_bits
    points = agree = 0
    for log_n in range(1, 21):
        for r in range(1, 7):
            for c in range(0, log_n + r + 1):
                for a in range(1, 5):
                    for fin in range(0, 8):
                        out[8] = 0xDEAD
                        n = f(log_n, r, c, a, fin, out)
                        assert n <= 8 and out[8] == 0xDEAD and all(out[i] == a for i in range(n))
                        points += 1
                        want = FC.constant_arity_bits(log_n, r, c, a, fin)
                        if want is not None and len(want) <= 8:
                            assert n == len(want), (log_n, r, c, a, fin)
                            agree += 1
    assert points == 57600 and agree == 51520

