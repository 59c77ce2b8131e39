"""The gates over the quadratic extension algebra -- CosetInterpolation, Reducing, ReducingExtension, ArithmeticExtension,
MulExtension -- against the oracle, one circuit per gate and parameterisation: constraint values at arbitrary points, complete proofs
word for word, and the witness check on H. CosetInterpolationGate runs at every subgroup size 2^2..2^5 with the smallest and the
largest legal degree:
  * smallest: the first degree whose intermediate wires still fit the 135 wire columns (2 for 4..16 points, 3 for 32 points);
  * largest: min(2^bits, 8). The quotient is committed at degree 8 n (CircuitConfig::max_quotient_degree_factor) and the selector
    groups are formed for constraints of degree at most 9 (gates/selectors.rs), so a gate of higher degree has neither a selector
    group nor a proof, in the reference as here; 2^bits is one chunk without intermediates.
Every table runs alone (num_selectors == 1: no selector filter at all) and inside the full gate set."""
import ctypes

import numpy as np
import pytest

import circuits as C
import oracle as O

pytestmark = pytest.mark.gpu
P = O.P


def smallest_degree(bits):
    n = 1 << bits
    return next(d for d in range(2, n + 1) if 1 + 2 * n + 6 + 4 * ((n - 2) // (d - 1)) <= C.NUM_WIRES)


COSET = [(C.COSET_INTERPOLATION, b, d, 0) for b in range(2, 6) for d in (smallest_degree(b), min(1 << b, C.MAX_DEGREE))]
EXT_GATES = [(C.REDUCING, 43, 0, 0), (C.REDUCING_EXT, 32, 0, 0), (C.ARITHMETIC_EXT, 10, 0, 0), (C.MUL_EXT, 13, 0, 0)]


def full_set(kind):
    """the full gate set with its CosetInterpolationGate replaced by `kind` (the other four gates under test are in every full set)"""
    if kind[0] != C.COSET_INTERPOLATION:
        return list(C.ALL_KINDS)
    return [kind if k[0] == C.COSET_INTERPOLATION else k for k in C.ALL_KINDS]


TABLES = [pytest.param([k], id="alone-%d-%d-%d" % k[:3]) for k in COSET + EXT_GATES] + \
         [pytest.param(full_set(k), id="full-%d-%d-%d" % k[:3]) for k in COSET]


def gpu_gates(mp2, ckt):
    return [mp2.Gate(g.kind, g.p0, g.p1, g.p2, g.selector_index, g.group_start, g.group_end) for g in ckt.gates]


def test_degrees_are_the_legal_extremes():
    assert [smallest_degree(b) for b in range(2, 6)] == [2, 2, 2, 3]
    for k in COSET:
        g = C.Gate(*k, 0, 0, 0)
        assert C.gate_num_constraints(g) <= 160 and 2 <= g.p1 <= 1 << g.p0


@pytest.mark.parametrize("kinds", TABLES)
def test_constraints_match_oracle(ctx, mp2, kinds):
    """mp2g_eval_gate_constraints == the oracle's evaluators: random points, the wires all 0 / 1 / p - 1, and points mixing the four"""
    ckt = C.build(5, kinds, 23)
    assert (ckt.num_selectors == 1) == (len(kinds) == 1)
    gates = gpu_gates(mp2, ckt)
    npts = 257
    consts = O.rand_field((ckt.num_constants, npts), 3)
    consts[:ckt.num_selectors, :100] = np.arange(100, dtype=np.uint64)[None, :] % np.uint64(len(ckt.gates) + 1)
    rnd = O.rand_field((C.NUM_WIRES, npts), 4)
    pick = np.random.default_rng(5).integers(0, 4, size=rnd.shape)
    edge = np.array([0, 1, P - 1], dtype=np.uint64)
    mixed = np.where(pick < 3, edge[np.minimum(pick, 2)], rnd)
    seen = False
    for wires in (rnd, np.zeros_like(rnd), np.ones_like(rnd), np.full_like(rnd, P - 1), mixed):
        got = mp2.eval_gate_constraints(ctx, gates, ckt.num_selectors, consts, wires, ckt.pi_hash)
        want = C.eval_on_points(ckt, consts, wires)
        assert np.array_equal(got, want)
        seen |= bool(got.any())
    assert seen
    # and on H with the circuit's own witness: every constraint vanishes
    assert not mp2.eval_gate_constraints(ctx, gates, ckt.num_selectors, ckt.pre[:ckt.num_constants], ckt.wires, ckt.pi_hash).any()


@pytest.mark.parametrize("rounds", [2, 1])
@pytest.mark.parametrize("kinds", TABLES)
def test_proofs_match_oracle(ctx, mp2, kinds, rounds):
    """prove() == the oracle's proof of the same witness, word for word, with one and two challenge rounds; the oracle verifies it"""
    log_n = 5
    ckt = C.build(log_n, kinds, 29)
    assert (ckt.num_selectors == 1) == (len(kinds) == 1)
    widths = (int(ckt.pre.shape[0]), C.NUM_WIRES, 10 * rounds, 8 * rounds)
    ofp = O.standard_params(log_n, widths, zs_count=rounds, pow_bits=4, num_queries=3)
    fp = mp2.FriParams()
    ctypes.memmove(ctypes.byref(fp), ctypes.byref(ofp), ctypes.sizeof(fp))
    cd = O.rand_field(4, 6)
    pr = mp2.BatchedProver(ctx, fp, 1)
    pr.set_preprocessed(ctx.to_device(ckt.pre))
    pr.enable_permutation(C.NUM_ROUTED, 8)
    pr.enable_quotient()
    pr.set_gates(gpu_gates(mp2, ckt), ckt.num_selectors)
    pr.enable_witness_check()
    pr.prove([ctx.to_device(ckt.wires[None]), None, None], ctx.to_device(cd), ctx.to_device(ckt.pi_hash[None]))
    assert pr.witness_status().tolist() == [0]
    caps, openings, proofs = pr.results()
    oc, oo, op, chal = C.prove(ckt, ofp, cd)
    assert np.array_equal(caps[0], oc) and np.array_equal(openings[0], oo) and np.array_equal(proofs[0], op)
    assert C.verify(ckt, ofp, cd, ckt.pi_hash, caps[0], openings[0], proofs[0]) == 0
    assert C.identity_check(ckt, ofp, openings[0], chal) == 0
    pr.free()


def output_wire(g):
    """a wire of the gate that one constraint pins and nothing else reads"""
    if g.kind == C.COSET_INTERPOLATION:
        return 3 + 2 * (1 << g.p0)  # evaluation value
    return {C.REDUCING: 0, C.REDUCING_EXT: 0, C.ARITHMETIC_EXT: 6, C.MUL_EXT: 4}[g.kind]


@pytest.mark.parametrize("kind", [pytest.param(k, id="%d-%d-%d" % k[:3]) for k in COSET[::2] + EXT_GATES])
def test_witness_check_flags_one_violated_constraint(ctx, mp2, kind):
    """the witness check on H (gate_check) flags a witness with one constraint of the gate violated, and only that witness"""
    log_n = 5
    ckt = C.build(log_n, full_set(kind), 31)
    ofp = O.standard_params(log_n, (int(ckt.pre.shape[0]), C.NUM_WIRES, 20, 16), pow_bits=3, num_queries=2)
    fp = mp2.FriParams()
    ctypes.memmove(ctypes.byref(fp), ctypes.byref(ofp), ctypes.sizeof(fp))
    gi = next(i for i, g in enumerate(ckt.gates) if (g.kind, g.p0, g.p1) == kind[:3])
    row, col = ckt.instances.index(gi), output_wire(ckt.gates[gi])
    bad = ckt.wires.copy()
    bad[col, row] = (int(bad[col, row]) + 1) % P
    # exactly one constraint of the gate is non-zero there
    out = mp2.eval_gate_constraints(ctx, gpu_gates(mp2, ckt), ckt.num_selectors, ckt.pre[:ckt.num_constants], bad, ckt.pi_hash)
    assert np.count_nonzero(out[:, row]) == 1 and not np.delete(out, row, axis=1).any()
    pr = mp2.BatchedProver(ctx, fp, 2)
    pr.set_preprocessed(ctx.to_device(ckt.pre))
    pr.enable_permutation(C.NUM_ROUTED, 8)
    pr.enable_quotient()
    pr.set_gates(gpu_gates(mp2, ckt), ckt.num_selectors)
    pr.enable_witness_check()
    pr.prove([ctx.to_device(np.stack([ckt.wires, bad])), None, None], ctx.to_device(O.rand_field(4, 1)),
             ctx.to_device(np.stack([ckt.pi_hash] * 2)))
    with pytest.raises(mp2.Mp2gError, match="proof 1 of the batch violates.* a gate constraint") as e:
        pr.witness_status()
    assert e.value.flags[0] == 0 and e.value.flags[1] & 2  # bit 0 may join: the wire is routed in some of these gates
    pr.free()
