"""Guards of tests/gate_lde_cases.py, without a GPU: the tables cover the kinds, the parameters and the light-gate counts the device
test is about; the reference of every case is non-trivial (non-zero at most points, every gate's filter both live and zero somewhere);
the reduction is the one the kernels are held to."""
import types

import numpy as np
import pytest

import circuits as C
import gate_lde_cases as G

P = G.P
# MP2G_CONSTRAINT_GATES (csrc/gate_shape.h), restated: every kind with constraints of its own
CONSTRAINT_KINDS = set(range(C.CONSTANT, C.UNINTERLEAVE_TO_U32 + 1)) - {C.LOOKUP, C.LOOKUP_TABLE}


def test_tables_cover_every_kind_at_both_parameter_ends():
    alone = [k for k in G.ALONE]
    assert {k[0] for k in alone} == CONSTRAINT_KINDS
    for kind in CONSTRAINT_KINDS - {C.PUBLIC_INPUT, C.POSEIDON2, C.POSEIDON, C.POSEIDON_MDS}:  # these four take no parameter
        assert len({k for k in alone if k[0] == kind}) >= 2, kind
    for k in alone:
        t = G.table("alone-%d-%d-%d-%d" % k)
        assert len(t.gates) == 1 and t.num_selectors == 1 and (t.gates[0].group_start, t.gates[0].group_end) == (0, 1)
        assert 0 < G.n_constraints(t) <= 160
    assert [g.kind for g in G.table("interleave").gates] == [C.U32_INTERLEAVE, C.UNINTERLEAVE_TO_B32, C.UNINTERLEAVE_TO_U32]
    assert len(G.table("all").gates) == 24 and G.n_constraints(G.table("all")) == 134
    both = G.table("all+interleave")
    assert len(both.gates) == 27 <= 32 and sum(g.kind in (C.U32_INTERLEAVE, C.UNINTERLEAVE_TO_B32, C.UNINTERLEAVE_TO_U32) for g in both.gates) == 6
    for name in G.ZERO_TABLES:
        assert G.n_constraints(G.table(name)) == 0
    assert {g.kind for g in G.table("lookup-only").gates} == {C.LOOKUP, C.LOOKUP_TABLE}
    assert all(name in G.TABLES for name in G.CROSS_TABLES)


def test_light_gate_counts_straddle_the_fused_launch():
    cap = G.max_light_gates()
    assert sorted(G.LIGHT_COUNTS.values()) == [0, 1, 2, cap, cap + 1, cap + 2]
    for name, n in G.LIGHT_COUNTS.items():
        t = G.table(name)
        assert len(G.light_gates(t)) == n, name
        assert any(g.kind not in G.LIGHT_KINDS and C.gate_num_constraints(g) for g in t.gates), name  # a heavy gate next to them
    # the overflow is real: in table order the 13th and 14th light gates come after the twelve the fused launch takes
    t = G.table("light-14")
    assert len(t.gates) == 16 and t.num_selectors == 4 and len(set(G.light_gates(t)[cap:])) == 2


def test_constraint_counts_are_the_library_s(mp2):
    """the light count above rests on gate_num_constraints: the same numbers as mp2g_gate_num_constraints for every gate of every table"""
    for name in G.TABLES:
        for g in G.table(name).gates:
            assert mp2.Gate(g.kind, g.p0, g.p1, g.p2, 0, 0, 1).num_constraints == C.gate_num_constraints(g), (name, g.kind)


def test_single_gate_tables_keep_index_group_and_selector():
    t = G.table("all")
    singles = G.single_gate_tables(t)
    assert [i for i, _ in singles] == [i for i, g in enumerate(t.gates) if g.kind != C.NOOP]
    for i, gates in singles:
        assert [(g.selector_index, g.group_start, g.group_end) for g in gates] == [(g.selector_index, g.group_start, g.group_end) for g in t.gates]
        assert [j for j, g in enumerate(gates) if g.kind != C.NOOP] == [i] and gates[i].p0 == t.gates[i].p0


def shapes_of(name):
    return G.CROSS_SHAPES if name in G.CROSS_TABLES else [G.REST_SHAPE]


@pytest.mark.parametrize("name", [n for n in G.TABLES if n not in G.ZERO_TABLES])
def test_references_are_not_trivial(name):
    """per table, at the shapes the device test runs it: the lattice sets give a non-zero reference at more than half of the points;
    every gate with constraints has a non-zero filter at N/8 points or more and -- where the filter is not the empty product of a
    table with one gate and one selector -- a zero filter at one point at least"""
    t = G.table(name)
    for lg, batch in shapes_of(name):
        for opset in G.LATTICE_SETS:
            c = G.case(name, opset, lg, batch)
            assert c.want.shape == (batch, 2, 1 << lg)
            assert np.count_nonzero(c.want) * 2 > c.want.size, (name, opset, lg, batch)
            assert max(int(a.max()) for a in (c.consts, c.wires, c.alphas, c.pi_hash)) < P
            f = G.filters(t, c.consts)
            for i, g in enumerate(t.gates):
                if not C.gate_num_constraints(g):
                    continue
                live = sum(1 for x in f[i] if x)
                assert live * 8 >= 1 << lg, (name, opset, lg, i)
                if len(t.gates) > 1 or t.num_selectors > 1:
                    assert live < 1 << lg, (name, opset, lg, i)
                else:
                    assert live == 1 << lg


def test_operand_sets_are_what_they_say():
    lat = set(G.EC)
    c = G.case("light-14", "both-lattice", 8, 3)
    assert set(c.wires.ravel().tolist()) <= lat and set(c.consts[4:].ravel().tolist()) <= lat and set(c.pi_hash.ravel().tolist()) <= lat
    assert len(set(c.wires.ravel().tolist())) == len(lat)  # every lattice value occurs
    sel = c.consts[:4]
    n_gates = len(c.table.gates)
    for row in sel:
        unused = int(np.count_nonzero(row == C.UNUSED_SELECTOR))
        assert unused >= 256 // 3 and int(np.count_nonzero(row <= n_gates)) >= 256 // 3
        assert len(set(row.tolist()) & lat) > 10
    u = G.case("light-14", "uniform", 8, 3)
    assert not set(u.wires.ravel().tolist()) & lat and len({tuple(w.ravel()[:8].tolist()) for w in u.wires}) == 3
    assert len({tuple(a) for a in u.alphas.tolist()}) == 3 and len({tuple(h) for h in u.pi_hash.tolist()}) == 3
    for name, v in (("wires-0", 0), ("wires-1", 1), ("wires-p-1", P - 1)):
        assert set(G.case("light-14", name, 8, 1).wires.ravel().tolist()) == {v}
    assert G.case("all", "uniform", 9, 3, "edge").alphas.tolist() == [list(a) for a in G.EDGE_ALPHAS]


def test_alpha_zero_reduces_to_the_first_constraint_and_one_to_the_sum():
    c = G.case("all", "both-lattice", 9, 3, "edge")
    for b, (a0, a1) in enumerate(G.EDGE_ALPHAS):
        cj = G.constraints(c.table, c.consts, c.wires[b], c.pi_hash[b])
        for a, alpha in enumerate((a0, a1)):
            if alpha == 0:
                assert np.array_equal(c.want[b, a], cj[0])
            elif alpha == 1:
                assert c.want[b, a].tolist() == [sum(col) % P for col in cj.T.tolist()]
            else:  # alpha = -1: the alternating sum
                assert c.want[b, a].tolist() == [sum(x if j % 2 == 0 else -x for j, x in enumerate(col)) % P for col in cj.T.tolist()]


def test_reference_is_the_filtered_sum_of_single_gate_references():
    """the reference is linear in the gates: what the device test's launch-order check relies on"""
    c = G.case("light-14", "both-lattice", 8, 1)
    total = np.zeros(c.want.shape, dtype=object)
    for i, gates in G.single_gate_tables(c.table):
        one = types.SimpleNamespace(gates=gates, gate_array=(C.Gate * len(gates))(*gates), num_selectors=c.table.num_selectors)
        total = (total + G.reference(one, c.consts, c.wires, c.alphas, c.pi_hash).astype(object)) % P
    assert np.array_equal(total.astype(np.uint64), c.want)


def test_bitrev_perm():
    assert G.bitrev_perm(3).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]
    for lg in G.LOG_POINTS:
        r = G.bitrev_perm(lg)
        assert np.array_equal(r[r], np.arange(1 << lg))


def test_a_wrong_word_is_named():
    c = G.case("light-2", "uniform", 3, 1)
    got = np.ascontiguousarray(c.want[:, :, G.bitrev_perm(3)])
    assert G.first_mismatch(c, got) is None and G.first_mismatch(c, got[:, :1]) is None
    got[0, 1, G.bitrev_perm(3)[5]] ^= np.uint64(1)
    msg = G.first_mismatch(c, got)
    assert "light-2" in msg and "proof 0, challenge 1" in msg and "point 5 " in msg and "1 of 16 words" in msg
