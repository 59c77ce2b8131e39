"""Lookup tables on the device: prove()'s set_lookup_wires as a kernel (csrc/lookup_wires.hip: mp2g_prover_lookup_wires_dev and the
pass mp2g_witness_program_run_dev runs after the tape), MP2G_OP_LOOKUP in the device replay, and the byte-realignment leaf of
recursion.column_realign_logic through the chain, the device verifier and a forest. The CPU side of the same feature is
tests/test_lookup_framework.py."""
import importlib

import numpy as np
import pytest

import circuits as C
import oracle as O
from test_lookup_framework import extract_leaf, framework_circuits, leaf_inputs

pytestmark = pytest.mark.gpu
R = importlib.import_module("mapreduce-plonky2_amd.recursion")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
LUT = importlib.import_module("mapreduce-plonky2_amd.lut")
SMALL_KINDS = [(C.NOOP, 0, 0, 0), (C.CONSTANT, 2, 0, 0), (C.PUBLIC_INPUT, 0, 0, 0), (C.ARITHMETIC, 20, 0, 0)] + C.LOOKUP_KINDS


def scrub(w, luts, rng):
    """a copy of the wire matrix w [135][n] with every cell set_lookup_wires writes -- the padding slots of the LookupGate rows, the
    78 table wires of the LookupTableGate rows -- replaced by random field elements"""
    w = w.copy()
    for t in luts:
        for j in range(t["n_lookups"], (t["last_lut_row"] - t["last_lu_row"]) * LUT.NUM_LU_SLOTS):
            r, c = t["last_lu_row"] + j // LUT.NUM_LU_SLOTS, 2 * (j % LUT.NUM_LU_SLOTS)
            w[c:c + 2, r] = rng.integers(0, O.P, 2, dtype=np.uint64)
        n_rows = t["first_lut_row"] - t["last_lut_row"] + 1
        w[:3 * LUT.NUM_LUT_SLOTS, t["last_lut_row"]:t["first_lut_row"] + 1] = rng.integers(0, O.P, (3 * LUT.NUM_LUT_SLOTS, n_rows), dtype=np.uint64)
    return w


def refill(ctx, cp, ckt, wires, seed):
    """scrub every matrix of wires [B][135][n], run mp2g_prover_lookup_wires_dev on the batch, return what comes back"""
    rng = np.random.default_rng(seed)
    bad = np.stack([scrub(w, ckt.luts, rng) for w in wires])
    assert not np.array_equal(bad, wires)
    d_w = ctx.to_device(bad)
    cp.pr.lookup_wires_dev([t["n_lookups"] for t in ckt.luts], d_w, len(wires))
    return d_w, d_w.download(wires.shape)


@pytest.mark.parametrize("B", [1, 3, 48])
def test_lookup_wires_dev_restores_synthetic_and_leaf_witnesses(ctx, mp2, B):
    ckt = C.build(8, C.ALL_KINDS + C.LOOKUP_KINDS, 41, luts=list(zip(C.bits_lookup_tables(), (100, 57))))
    cp = FW.CircuitProver(ctx, ckt, B, witness_check=True, pow_bits=4, num_queries=3)
    wires = np.stack([ckt.wires] * B)
    d_w, got = refill(ctx, cp, ckt, wires, 7 + B)
    assert np.array_equal(got, wires)
    cp.prove(d_w, ctx.to_device(np.stack([ckt.pi_hash] * B)))
    assert cp.pr.witness_status().tolist() == [0] * B
    cp.free()
    leaves = [extract_leaf(leaf_inputs(100 + b)) for b in range(B)]
    cp = FW.CircuitProver(ctx, leaves[0], B, witness_check=True, pow_bits=4, num_queries=3)
    wires = np.stack([c.wires for c in leaves])
    d_w, got = refill(ctx, cp, leaves[0], wires, 11 + B)
    assert np.array_equal(got, wires)
    cp.prove(d_w, ctx.to_device(np.stack([c.pi_hash for c in leaves])))
    assert cp.pr.witness_status().tolist() == [0] * B
    cp.free()


def test_lookup_wires_dev_one_entry_and_65536_entry_tables(ctx, mp2):
    one = C.build(6, SMALL_KINDS, 5, luts=[([(5, 9)], 3)])
    assert one.luts[0]["first_lut_row"] == one.luts[0]["last_lut_row"]
    big_table = [(v, (v * 40503 + 7) & 0xFFFF) for v in range(65536)]
    big = C.build(13, SMALL_KINDS, 6, luts=[(big_table, 100)])
    assert big.luts[0]["last_lut_row"] - big.luts[0]["last_lu_row"] == 3 and big.luts[0]["first_lut_row"] - big.luts[0]["last_lut_row"] + 1 == 2521
    for ckt in (one, big):
        cp = FW.CircuitProver(ctx, ckt, 2, witness_check=True, pow_bits=4, num_queries=3)
        wires = np.stack([ckt.wires] * 2)
        d_w, got = refill(ctx, cp, ckt, wires, 3)
        assert np.array_equal(got, wires)
        cp.prove(d_w, ctx.to_device(np.stack([ckt.pi_hash] * 2)))
        assert cp.pr.witness_status().tolist() == [0, 0]
        # every row of RE and of the partial sums, not only where they end: the proof is the oracle's, word for word
        caps, openings, proofs = cp.results()
        oc, oo, op, _ = C.prove(ckt, C.oracle_params(ckt, pow_bits=4, num_queries=3), cp.circuit_digest)
        for b in range(2):
            assert np.array_equal(caps[b], oc) and np.array_equal(openings[b], oo) and np.array_equal(proofs[b], op)
        cp.free()


def test_lookup_wires_dev_does_not_count_a_pair_outside_the_table(ctx, mp2):
    ckt = C.build(8, C.ALL_KINDS + C.LOOKUP_KINDS, 43, luts=list(zip(C.bits_lookup_tables(), (100, 57))))
    cp = FW.CircuitProver(ctx, ckt, 3, witness_check=True, pow_bits=4, num_queries=3)
    wires = np.stack([ckt.wires] * 3)
    r = ckt.luts[1]["last_lu_row"]
    wires[1, 1, r] = (int(wires[1, 1, r]) + 1) % O.P  # proof 1, table 1, slot 0: an output that is not the table's
    want = wires.copy()
    for t in ckt.luts:
        LUT.fill_wires(want[1], t)  # the rule restated in Python: that slot counts for nothing, every other count stands
    assert int(want[1, :, ckt.luts[1]["last_lut_row"]:ckt.luts[1]["first_lut_row"] + 1][2:78:3].sum()) == 2 * LUT.NUM_LU_SLOTS - 1
    assert np.array_equal(want[0], ckt.wires) and np.array_equal(want[2], ckt.wires)
    d_w, got = refill(ctx, cp, ckt, wires, 19)
    assert np.array_equal(got, want)
    cp.prove(d_w, ctx.to_device(np.stack([ckt.pi_hash] * 3)))
    with pytest.raises(mp2.Mp2gError) as e:
        cp.pr.witness_status()
    assert e.value.flags.tolist() == [0, 4, 0]
    # refused: more lookups than the table's rows hold
    with pytest.raises(mp2.Mp2gError):
        cp.pr.lookup_wires_dev([121, 57], d_w, 3)
    cp.free()


def test_device_replay_equals_host_replay_with_an_input_outside_the_tables(ctx, mp2):
    ins = np.array([leaf_inputs(200 + b) for b in range(5)], dtype=np.uint64)
    ins[2, 7] = 300  # no table holds it: proof 2 fails the lookup argument, nothing else does
    ckt = extract_leaf(ins[0])
    prog = mp2.WitnessProgram(ckt)
    wires, pi_hash, pis = prog.run(ins)
    n = 1 << ckt.log_n
    d_w, d_pr = ctx.alloc(5 * 135 * n * 8), ctx.alloc(5 * prog.probe.size * 8)
    prog.run_dev(ctx, ctx.to_device(ins), 5, d_w, d_pr)
    assert np.array_equal(d_w.download((5, 135, n)), wires)
    assert np.array_equal(d_pr.download((5, prog.probe.size)), np.concatenate([pi_hash, pis], axis=1))
    for b in (0, 1, 3, 4):
        assert np.array_equal(wires[b], extract_leaf(ins[b]).wires)
    cp = FW.CircuitProver(ctx, ckt, 5, witness_check=True, pow_bits=4, num_queries=3)
    cp.prove(d_w, ctx.to_device(pi_hash))
    with pytest.raises(mp2.Mp2gError) as e:
        cp.pr.witness_status()
    assert e.value.flags.tolist() == [0, 0, 4, 0, 0]
    cp.free()


def pack(proof):
    """a proof (caps, openings, fri, public inputs) in a parent's input order, as mp2g_forest_proof returns it"""
    caps, openings, fri, pis = proof
    return np.concatenate([np.asarray(pis, dtype=np.uint64).ravel(), np.asarray(caps, dtype=np.uint64)[1:].ravel(),
                           np.asarray(openings, dtype=np.uint64).ravel(), np.asarray(fri, dtype=np.uint64).ravel()])


def test_chain_verifier_and_forest_with_the_lookup_leaf(ctx, mp2):
    prover = FW.GpuProver(ctx)
    fw = R.RecursiveCircuits(framework_circuits(), prover, FW.circuit_fri_params)
    assert {k: [c[0].log_n for c in v] for k, v in fw.chains.items()} == {"extract": [8, 12], "merge": [13, 12]}
    ins = [leaf_inputs(300 + i) for i in range(8)]
    cap = []
    leaves = fw.generate_proofs_batch("extract", [([], [], x) for x in ins[:2]], capture=cap)
    (parent,) = fw.generate_proofs_batch("merge", [(leaves, ["extract"] * 2, None)], capture=cap)
    assert len(cap) == 2 * 2 + 2
    # every step of both chains is the oracle's proof of the same witness, word for word
    for name, step, ckt, digest, w, ph, c, o, p in cap:
        oc, oo, op, _ = C.prove_witness(ckt, C.oracle_params(ckt), digest, w, ph)
        assert np.array_equal(c, oc) and np.array_equal(o, oo) and np.array_equal(p, op), (name, step)
    assert [int(x) for x in leaves[0][3][:8]] == R.column_realign_value(ins[0][:32], ins[0][32])
    # the device verifier: the base proofs of the leaf (its tables given) and the final proofs
    base = [x for x in cap if x[0] == "extract" and x[1] == 0]
    assert prover.verify_batch(base[0][2], [x[6:9] for x in base], [x[5] for x in base]).tolist() == [0, 0]
    for name, proofs in (("extract", leaves), ("merge", [parent])):
        final = fw.chains[name][-1][0]
        assert prover.verify_batch(final, [p[:3] for p in proofs], [O.hash_n_to_m_no_pad(p[3], 4) for p in proofs]).tolist() == [0] * len(proofs)
    bad = base[0][7].copy()
    bad[fw.chains["extract"][0][0].pre.shape[0] + 135 + 20 + 16 + 3, 0] ^= np.uint64(1)  # a lookup opening at zeta
    assert prover.verify_batch(base[0][2], [(base[0][6], bad, base[0][8])], [base[0][5]]).tolist()[0] != 0

    # a forest of 8 leaves and 7 parents (mp2g_forest_*) against generate_proofs_batch level by level
    level = fw.generate_proofs_batch("extract", [([], [], x) for x in ins])
    names = ["extract"] * 8
    while len(level) > 1:
        level = fw.generate_proofs_batch("merge", [([level[2 * i], level[2 * i + 1]], names[2 * i:2 * i + 2], None) for i in range(len(level) // 2)])
        names = ["merge"] * len(level)
    set_digest = np.asarray(fw.set_digest, dtype=np.uint64)
    pw = pack(level[0]).size
    heads = {}
    for cn in ("extract", "merge"):
        vd = fw.vds[cn]
        bits, sib = fw.membership(vd[1])
        heads[cn] = (np.concatenate([np.asarray(vd[0], dtype=np.uint64).ravel(), np.asarray(vd[1], dtype=np.uint64).ravel()]),
                     np.concatenate([np.asarray(bits, dtype=np.uint64).ravel(), np.asarray(sib, dtype=np.uint64).ravel()]))
    per_child = heads["extract"][0].size + pw + heads["extract"][1].size
    offs = [4 + heads["extract"][0].size + k * per_child for k in range(2)]
    progs = {cn: fw.witness_programs(cn) for cn in ("extract", "merge")}
    desc = [(progs["extract"][0].n_inputs, [], progs["extract"][0].n_inputs), (progs["merge"][0].n_inputs, offs, progs["merge"][0].n_inputs - 2 * pw)]
    assert desc[1][0] == 4 + 2 * per_child
    chains = [prover._chain([c[0] for c in fw.chains[cn]], progs[cn], 8) for cn in ("extract", "merge")]
    forest = mp2.Forest([ctx], desc, [chains], pw, 16)
    forest.add_nodes(0, list(range(1, 9)), None, np.stack([np.concatenate([set_digest, np.asarray(x, dtype=np.uint64)]) for x in ins]))
    kids = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14]]
    kinds = [["extract"] * 2] * 4 + [["merge"] * 2] * 3
    consts = np.stack([np.concatenate([set_digest] + [heads[k][i] for k in kk for i in (0, 1)]) for kk in kinds])
    forest.add_nodes(1, list(range(9, 16)), kids, consts, keep=[0] * 6 + [1])
    forest.prove([list(range(1, 16))])
    assert forest.proved == 15
    assert np.array_equal(forest.proof_words(15), pack(level[0]))
    forest.free()
    prover.free()
