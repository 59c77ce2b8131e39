"""The quotient's gate kernels -- gate_constraints_lde_kernel<K>, gate_constraints_lde_light_kernel and the host logic of
gate_constraints_lde -- run alone through mp2g_eval_gate_constraints_lde and compared bit for bit with the CPU oracle's constraints,
alpha-reduced on Python integers (tests/gate_lde_cases.py; tests/test_gate_lde_cases.py guards the cases). These kernels evaluate
eval_gate<true>, the body on weak representatives, which no other test reaches away from whole proofs: here the wires, the gate
constants, the selectors, the public-inputs hash and the challenges sit on the lattice of 32-bit edge words, every point on its own.
Beside the oracle the result is held to the kernels' own algebra: linear in the gates whatever the launches (first / accumulate, the
fused light launch, its overflow), blind to the lookup-selector rows, the same per challenge with one or two of them, and equal to the
canonical evaluator of mp2g_eval_gate_constraints."""
import numpy as np
import pytest

import circuits as C
import gate_lde_cases as G

pytestmark = pytest.mark.gpu
P = G.P
SENTINEL = 0xDEADBEEFDEADBEEF


def run(mp2, ctx, c, nc=2, gates=None, **kw):
    return mp2.eval_gate_constraints_lde(ctx, gates or c.table.gates, c.table.num_selectors, c.consts, c.wires, c.alphas[:, :nc], c.pi_hash, **kw)


def cases_of(name):
    """(operand set, log_points, proofs) of a table: every set at the standard shape, and on the cross tables every other shape too"""
    out = [(s, *G.REST_SHAPE) for s in G.SETS]
    if name in G.CROSS_TABLES:
        out += [(s, lg, b) for lg, b in G.CROSS_SHAPES if (lg, b) != G.REST_SHAPE for s in ("uniform", "both-lattice")]
    return out


@pytest.mark.parametrize("name", list(G.TABLES))
def test_matches_the_reference(ctx, mp2, name):
    """every operand set, bit for bit; with one challenge the result is the first row of the two-challenge result"""
    for opset, lg, batch in cases_of(name):
        c = G.case(name, opset, lg, batch)
        got = run(mp2, ctx, c)
        assert got.shape == (batch, 2, 1 << lg)
        msg = G.first_mismatch(c, got)
        assert msg is None, msg
        if name in G.ZERO_TABLES:
            assert not got.any()
        if name in G.CROSS_TABLES or opset == "both-lattice":
            one = run(mp2, ctx, c, nc=1)
            msg = G.first_mismatch(c, one)
            assert msg is None, "nc = 1, " + msg
            assert np.array_equal(one, got[:, :1])


@pytest.mark.parametrize("name", ["all", "light-14"])
def test_edge_challenges(ctx, mp2, name):
    """alpha = 0, 1 and p - 1, a different pair per proof"""
    c = G.case(name, "both-lattice", 9, 3, "edge")
    msg = G.first_mismatch(c, run(mp2, ctx, c))
    assert msg is None, msg


@pytest.mark.parametrize("name", ["interleave", "all", "all+interleave"] + list(G.LIGHT_COUNTS))
def test_result_is_the_sum_of_its_gates_run_alone(ctx, mp2, name):
    """a table's result = the field sum of the results of its gates, each run in a table where the others are Noops that keep their
    selector fields (same index, group and filter): the first / accumulate path and the fused launch against the per-kind kernels"""
    c = G.case(name, "both-lattice", 9, 3)
    whole = run(mp2, ctx, c)
    total = np.zeros(whole.shape, dtype=object)
    for i, gates in G.single_gate_tables(c.table):
        part = run(mp2, ctx, c, gates=gates)
        assert part.any(), (name, i)
        total = (total + part.astype(object)) % P
    bad = np.nonzero(total.astype(np.uint64) != whole)
    assert not bad[0].size, "%s: proof %d, challenge %d, output column %d" % (G.describe(c), bad[0][0], bad[1][0], bad[2][0])


@pytest.mark.parametrize("name", ["all", "light-14", "alone-1-2-0-0", "alone-3-20-0-0", "alone-11-5-2-2"])
def test_lookup_selector_rows_are_skipped(ctx, mp2, name):
    """five rows between the selectors and the gate constants, num_lookup_selectors = 5: the gates read their constants past them"""
    c = G.case(name, "both-lattice", 9, 3)
    ns = c.table.num_selectors
    dummy = np.random.default_rng(5).integers(0, P, size=(5, c.consts.shape[1]), dtype=np.uint64)
    wide = np.concatenate([c.consts[:ns], dummy, c.consts[ns:]])
    got = mp2.eval_gate_constraints_lde(ctx, c.table.gates, ns, wide, c.wires, c.alphas, c.pi_hash, num_lookup_selectors=5)
    assert np.array_equal(got, run(mp2, ctx, c))
    msg = G.first_mismatch(c, got)
    assert msg is None, msg


@pytest.mark.parametrize("name", list(G.CROSS_TABLES) + ["interleave", "all+interleave", "light-12"])
def test_points_kernel_agrees(ctx, mp2, name):
    """eval_gate<false> on the same inputs (mp2g_eval_gate_constraints), alpha-reduced on the host = the LDE kernels' output"""
    c = G.case(name, "both-lattice", 8, 3)
    got = run(mp2, ctx, c)[:, :, G.bitrev_perm(c.log_points)]
    for b in range(c.batch):
        cj = mp2.eval_gate_constraints(ctx, c.table.gates, c.table.num_selectors, c.consts, c.wires[b], c.pi_hash[b])
        for a in range(2):
            assert np.array_equal(G.alpha_reduce(cj, c.alphas[b, a]), got[b, a]), "%s: proof %d, challenge %d" % (G.describe(c), b, a)


def test_refusals(ctx, mp2):
    """a word equal to p in each input, nc = 3, B = 0, a malformed table: an error that names the argument, `out` untouched"""
    c = G.case("light-2", "uniform", 3, 3)
    t = c.table
    args = {"consts": c.consts, "wires": c.wires, "alphas": c.alphas, "pi_hash": c.pi_hash}
    out = np.full(3 * 3 * 8, SENTINEL, dtype=np.uint64)  # room for what the nc = 3 call asks for

    def refused(match, gates=t.gates, num_selectors=t.num_selectors, **over):
        a = dict(args, **over)
        with pytest.raises(mp2.Mp2gError, match=match):
            mp2.eval_gate_constraints_lde(ctx, gates, num_selectors, a["consts"], a["wires"], a["alphas"], a["pi_hash"], out=out)
        assert (out == SENTINEL).all()

    for name, arr in args.items():
        bad = arr.copy()
        bad.ravel()[bad.size - 1] = P  # the last word: the whole argument is read
        refused(name + ": word %d is not canonical" % (bad.size - 1), **{name: bad})
        bad = arr.copy()
        bad.ravel()[0] = 2 ** 64 - 1
        refused(name + ": word 0 is not canonical", **{name: bad})
    refused("nc must be 1 or 2", alphas=np.zeros((3, 3), dtype=np.uint64))
    refused("B must be", wires=c.wires[:0], alphas=c.alphas[:0], pi_hash=c.pi_hash[:0])
    unknown = [C.Gate(g.kind, g.p0, g.p1, g.p2, g.selector_index, g.group_start, g.group_end) for g in t.gates]
    unknown[1].kind = 99
    refused(r"invalid gate table: gate 1 \(kind 99\): unknown gate kind", gates=unknown)
    refused("invalid gate table: num_selectors", num_selectors=0)
    refused(r"invalid gate table: gate \d+ .*more constants", consts=c.consts[:t.num_selectors])  # no room for the gate constants
    refused(r"invalid gate table: gate \d+ .*more wires", wires=c.wires[:, :3])
    # and the same arguments unchanged run, into the array given
    out = np.full(c.want.shape, SENTINEL, dtype=np.uint64)
    got = mp2.eval_gate_constraints_lde(ctx, t.gates, t.num_selectors, c.consts, c.wires, c.alphas, c.pi_hash, out=out)
    assert got is out and G.first_mismatch(c, out) is None
