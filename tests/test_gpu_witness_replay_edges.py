"""The device witness replay (mp2g_witness_program_run_dev: csrc/witness_dev.hip with the opcode bodies of csrc/witness_ops.h) on the
families of tests/witness_edge_cases.py: every base opcode on edge operands, the Poseidon2 gate bodies (the 16-lane cooperative one
and the one-lane one) on lattice states, and the branches of the level loop through each kernel instance. The reference is the
builder's Python integers, one build per vector; the host replay is compared with them too, so that a mismatch tells the two sides
apart. Every replay runs between guard bands. The shapes these tests rest on are asserted in tests/test_witness_edge_cases.py."""
import importlib

import numpy as np
import pytest

import circuits as C
import witness_edge_cases as E
from test_gpu_ntt_merkle import _At

pytestmark = pytest.mark.gpu
R = importlib.import_module("mapreduce-plonky2_amd.recursion")
GUARD = 1 << 12  # words
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)


class Banded:
    """the wire buffer and the probe buffer of a batch, each between two guard bands of a sentinel"""

    def __init__(self, ctx, prog, log_n, batch):
        self.ctx, self.prog, self.batch, self.n = ctx, prog, batch, 1 << log_n
        self.words = (batch * 135 * self.n, batch * prog.probe.size)
        self.bufs = [ctx.to_device(np.full(w + 2 * GUARD, SENTINEL, dtype=np.uint64)) for w in self.words]

    def run(self, a):
        """replay the batch a [B][n_inputs] into the buffers -> (wires [B][135][n], probe [B][4 + public inputs]); the bands must
        come back untouched"""
        assert a.shape[0] == self.batch
        d_in = self.ctx.to_device(a)
        self.prog.run_dev(self.ctx, d_in, self.batch, _At(self.bufs[0], GUARD * 8), _At(self.bufs[1], GUARD * 8))
        out = []
        for buf, w in zip(self.bufs, self.words):
            got = buf.download((w + 2 * GUARD,))
            assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), "the replay wrote outside its buffer"
            out.append(got[GUARD:-GUARD])
        d_in.free()
        return out[0].reshape(self.batch, 135, self.n), out[1].reshape(self.batch, self.prog.probe.size)

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.fixture(scope="module")
def programs(mp2):
    """one WitnessProgram per family and its host replay of the whole family, made when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            a, ckts = E.family(name)
            prog = mp2.WitnessProgram(ckts[0])
            made[name] = (a, ckts, prog, prog.run(a))
        return made[name]

    yield get
    for _, _, prog, _ in made.values():
        prog.free()


def check(got_w, got_pr, ckts, host, order):
    """device replay == builder and host replay == builder, word for word, for the vectors `order` of the family"""
    host_w, host_h, host_pi = host
    for k, v in enumerate(order):
        c = ckts[v]
        assert np.array_equal(host_w[v], c.wires), f"host replay != builder (vector {v}): {E.mismatch(host_w[v], c.wires)}"
        assert np.array_equal(host_h[v], c.pi_hash) and np.array_equal(host_pi[v], c.public_inputs), f"host replay != builder (vector {v})"
        assert np.array_equal(got_w[k], c.wires), f"device replay != builder (vector {v}): {E.mismatch(got_w[k], c.wires)}"
        assert np.array_equal(got_pr[k, :4], c.pi_hash), f"device public-inputs hash != builder (vector {v})"
        assert np.array_equal(got_pr[k, 4:], c.public_inputs), f"device public inputs != builder (vector {v})"


def replay_twice(ctx, a, ckts, prog, host):
    """the whole family as one batch, then the same vectors in reverse order into the same buffers: the slot table and the staging
    matrix are set up per run, so the second run gives the second vectors' wires exactly. -> the first run's wires"""
    band = Banded(ctx, prog, ckts[0].log_n, len(ckts))
    order = list(range(len(ckts)))
    got_w, got_pr = band.run(a)
    check(got_w, got_pr, ckts, host, order)
    again_w, again_pr = band.run(np.ascontiguousarray(a[::-1]))
    check(again_w, again_pr, ckts, host, order[::-1])
    band.free()
    return got_w


def test_every_base_opcode_on_edge_operands(ctx, programs):
    """the opcode circuit on all-0, all-1, all-(p - 1), all-u32::MAX, lattice draws, the domain vector and the two corner vectors:
    device == builder == host. On the domain vector the device's wires also make every gate constraint vanish under the oracle's
    evaluators, which owe nothing to the builder."""
    a, ckts, prog, host = programs("opcodes")
    got_w = replay_twice(ctx, a, ckts, prog, host)
    d = E.DOMAIN_VECTOR
    assert E.gate_constraints_hold(ckts[d], got_w[d], C.eval_on_points), "a gate constraint does not vanish on the device's wires"


@pytest.mark.parametrize("name", ["p2_coop", "p2_lanes", "poseidon"])
def test_permutation_gate_bodies_on_lattice_states(ctx, programs, name):
    """exec_p2_coop (8 rows on level 1), exec_p2 (65 rows) and exec_poseidon on raw lattice words, every state of twelve equal lattice
    words among them: each wire of each round against the builder, and the outputs of the rows with swap 0 or 1 against the oracle's
    permutation"""
    a, ckts, prog, host = programs(name)
    op = R.OP_POSEIDON if name == "poseidon" else R.OP_P2
    assert E.levels_by_opcode(ckts[0].tape)[1][op] == E.P2_ROWS[name]
    got_w = replay_twice(ctx, a, ckts, prog, host)
    E.check_permutations(name, a, ckts[0], got_w)


@pytest.mark.parametrize("batch", [1, 3, len(E.chain_vectors())])
@pytest.mark.parametrize("instance", E.INSTANCES)
def test_level_loop_boundaries_in_every_kernel_instance(ctx, programs, instance, batch):
    """the chain of levels with 1, 31, 32, 33, 63, 64 and 65 Poseidon2 rows, companions on both sides of them in opcode order and two
    levels of more than 512 instructions, through the plain, GF(p^5), wide and lookup instances of the kernel"""
    a, ckts, prog, host = programs("chain_" + instance)
    assert prog.n_levels == E.check_chain_shape(ckts[0], instance)
    if batch == len(ckts):
        replay_twice(ctx, a, ckts, prog, host)
        return
    order = list(range(len(ckts) - batch, len(ckts)))  # the narrow batches take the last vectors: the draws, not the all-zero one
    band = Banded(ctx, prog, ckts[0].log_n, batch)
    got_w, got_pr = band.run(np.ascontiguousarray(a[order]))
    check(got_w, got_pr, ckts, host, order)
    band.free()
