"""Gate tables, operand sets and the exact reference for the quotient-side gate evaluator (mp2g_eval_gate_constraints_lde:
gate_constraints_lde_kernel<K>, gate_constraints_lde_light_kernel and the host logic that orders their launches).

The LDE kernels run eval_gate<true>, the body on weak representatives, which whole proofs reach only at uniform operands: a carry or
borrow branch of gl_subw / gl_addw / gl_reduce96w / gl_mul_small_w is then taken about once in 2^32 operations. Here every point of
a case is drawn on its own, the wires, the gate constants, the selectors and the public-inputs hash from the lattice of 32-bit
edge words (field_cases.EC) as well as uniformly.

Reference: want[b][a][p] = sum_j alpha_{b,a}^j C_j(p) mod p with C_j from circuits.eval_on_points (the CPU oracle's evaluator, which
already sums filter_g c_{g,j} over the gates), reduced on Python integers. Exact: no tolerance. `p` is the column of the input
matrices; the device writes the point's value to column bitrev(p) (bitrev_perm).

tests/test_gate_lde_cases.py guards these tables without a GPU, tests/test_gpu_gates_lde.py runs them."""
import functools
import os
import re
import types
import zlib

import numpy as np

import circuits as C
from field_cases import EC, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kinds of the fused launch (MP2G_LIGHT_GATES, csrc/gate_shape.h), restated
LIGHT_KINDS = (C.CONSTANT, C.PUBLIC_INPUT, C.ARITHMETIC, C.BASE_SUM, C.ARITHMETIC_EXT, C.MUL_EXT)


def max_light_gates():
    """MP2G_MAX_LIGHT_GATES, read from the source that defines it"""
    src = open(os.path.join(ROOT, "mapreduce-plonky2_amd", "csrc", "gates.hip")).read()
    return int(re.search(r"#define MP2G_MAX_LIGHT_GATES (\d+)", src).group(1))


# Every kind of MP2G_CONSTRAINT_GATES alone (one selector, no filter, one launch with first = 1), at the smallest and the largest
# parameters tests/test_gpu_gates.py::test_gate_parameter_fuzz and tests/test_gpu_gates_extension.py draw from; the interleave
# gates at one operation and at the most that fit 135 wires.
ALONE = [
    (C.CONSTANT, 1, 0, 0), (C.CONSTANT, 2, 0, 0), (C.PUBLIC_INPUT, 0, 0, 0), (C.ARITHMETIC, 1, 0, 0), (C.ARITHMETIC, 20, 0, 0),
    (C.BASE_SUM, 1, 2, 0), (C.BASE_SUM, 63, 2, 0), (C.BASE_SUM, 63, 5, 0), (C.ARITHMETIC_EXT, 1, 0, 0), (C.ARITHMETIC_EXT, 10, 0, 0),
    (C.MUL_EXT, 1, 0, 0), (C.MUL_EXT, 13, 0, 0), (C.POSEIDON2, 0, 0, 0), (C.EXPONENTIATION, 1, 0, 0), (C.EXPONENTIATION, 66, 0, 0),
    (C.REDUCING, 1, 0, 0), (C.REDUCING, 43, 0, 0), (C.REDUCING_EXT, 1, 0, 0), (C.REDUCING_EXT, 32, 0, 0),
    (C.RANDOM_ACCESS, 1, 1, 0), (C.RANDOM_ACCESS, 5, 2, 2), (C.POSEIDON, 0, 0, 0), (C.POSEIDON_MDS, 0, 0, 0),
    (C.COSET_INTERPOLATION, 2, 2, 0), (C.COSET_INTERPOLATION, 5, 3, 0), (C.COSET_INTERPOLATION, 5, 8, 0),
    (C.U32_ARITHMETIC, 1, 0, 0), (C.U32_ARITHMETIC, 3, 0, 0), (C.U32_RANGE_CHECK, 1, 0, 0), (C.U32_RANGE_CHECK, 7, 0, 0),
    (C.U32_SUBTRACTION, 1, 0, 0), (C.U32_SUBTRACTION, 6, 0, 0), (C.U32_ADD_MANY, 1, 1, 0), (C.U32_ADD_MANY, 8, 4, 0),
    (C.COMPARISON, 4, 4, 0), (C.COMPARISON, 32, 16, 0),
    (C.U32_INTERLEAVE, 1, 0, 0), (C.U32_INTERLEAVE, 3, 0, 0), (C.UNINTERLEAVE_TO_B32, 1, 0, 0), (C.UNINTERLEAVE_TO_B32, 2, 0, 0),
    (C.UNINTERLEAVE_TO_U32, 1, 0, 0), (C.UNINTERLEAVE_TO_U32, 2, 0, 0),
]
INTERLEAVE = C.EXTRACTION_KINDS[:3]
NOOP = (C.NOOP, 0, 0, 0)
# twelve light gates -- exactly MP2G_MAX_LIGHT_GATES --, then a thirteenth and a fourteenth: the overflow goes the ordinary way
LIGHT = [(C.ARITHMETIC, k, 0, 0) for k in range(1, 8)] + [(C.CONSTANT, 1, 0, 0), (C.CONSTANT, 2, 0, 0), (C.PUBLIC_INPUT, 0, 0, 0),
                                                         (C.BASE_SUM, 5, 2, 0), (C.BASE_SUM, 7, 3, 0), (C.ARITHMETIC_EXT, 3, 0, 0),
                                                         (C.MUL_EXT, 2, 0, 0)]
HEAVY = (C.POSEIDON2, 0, 0, 0)

TABLES = {"alone-%d-%d-%d-%d" % k: [k] for k in ALONE}
TABLES["interleave"] = list(INTERLEAVE)
TABLES["all"] = list(C.ALL_KINDS)
# ALL_KINDS holds the interleave kinds already: the second copies run one operation each. 27 gates <= MP2G_MAX_GATES
TABLES["all+interleave"] = list(C.ALL_KINDS) + [(k, 1, 0, 0) for k, _, _, _ in INTERLEAVE]
# 0 light gates; 1 (demoted to an ordinary launch); 2 (the smallest fused launch); exactly 12; 13 and 14 (overflow)
TABLES["light-0"] = [NOOP, HEAVY, (C.EXPONENTIATION, 66, 0, 0)]
for _n in (1, 2, 12, 13, 14):
    TABLES["light-%d" % _n] = [NOOP] + LIGHT[:_n] + [HEAVY]
# no constraints at all: zeros. C.build deals rows to a gate that is no lookup gate, hence the Noop of "lookup"; "lookup-only" is
# that table without it
TABLES["noop"] = [NOOP]
TABLES["lookup"] = [NOOP] + C.LOOKUP_KINDS
TABLES["lookup-only"] = None
LIGHT_COUNTS = {"light-0": 0, "light-1": 1, "light-2": 2, "light-12": 12, "light-13": 13, "light-14": 14}
ZERO_TABLES = ("noop", "lookup", "lookup-only")

# operand sets: (wires, gate constants); "u" uniform, "l" from the lattice, an integer: that value everywhere
SETS = {"uniform": ("u", "u"), "wires-lattice": ("l", "u"), "consts-lattice": ("u", "l"), "both-lattice": ("l", "l"),
        "wires-0": (0, "u"), "wires-1": (1, "u"), "wires-p-1": (P - 1, "u")}
LATTICE_SETS = ("wires-lattice", "consts-lattice", "both-lattice")
LOG_POINTS = (3, 8, 9)  # one partial block, exactly one block, two blocks of 256 lanes
EDGE_ALPHAS = ((0, 1), (1, P - 1), (P - 1, 0))


@functools.lru_cache(maxsize=None)
def table(name):
    """the gate table of a name: an object with gates, gate_array, num_selectors, pi_hash (what circuits.eval_on_points reads)"""
    if name == "lookup-only":
        full = table("lookup")
        gates = [C.Gate(g.kind, g.p0, g.p1, g.p2, 0, 0, 2) for g in full.gates if g.kind != C.NOOP]
        return types.SimpleNamespace(gates=gates, gate_array=(C.Gate * 2)(*gates), num_selectors=1, pi_hash=full.pi_hash)
    return C.build(5, TABLES[name], 1 + zlib.crc32(name.encode()) % 1000)


def n_constraints(t):
    return max(C.gate_num_constraints(g) for g in t.gates)


def light_gates(t):
    """indices of the gates the fused launch may take"""
    return [i for i, g in enumerate(t.gates) if g.kind in LIGHT_KINDS and C.gate_num_constraints(g)]


def single_gate_tables(t):
    """(gate index, table) per gate with constraints: the table with every other gate turned into a Noop that keeps its selector
    fields, so that the gate's index, group and filter stay what they are in `t`"""
    out = []
    for i, g in enumerate(t.gates):
        if C.gate_num_constraints(g):
            gates = [C.Gate(*((x.kind, x.p0, x.p1, x.p2) if j == i else (C.NOOP, 0, 0, 0)), x.selector_index, x.group_start, x.group_end)
                     for j, x in enumerate(t.gates)]
            out.append((i, gates))
    return out


def bitrev_perm(lg):
    """perm[p] = bitrev(p, lg)"""
    p = np.arange(1 << lg)
    r = np.zeros_like(p)
    for k in range(lg):
        r |= ((p >> k) & 1) << (lg - 1 - k)
    return r


def _uniform(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _lattice(rng, shape):
    return np.array(EC, dtype=np.uint64)[rng.integers(0, len(EC), size=shape)]


def _draw(rng, how, shape):
    if how == "u":
        return _uniform(rng, shape)
    if how == "l":
        return _lattice(rng, shape)
    return np.full(shape, how, dtype=np.uint64)


def selector_rows(rng, t, n):
    """a third of the points hold a gate index 0..n_gates, a third UNUSED_SELECTOR, a third a lattice value: the evaluator is a
    polynomial in the selector, any field element is a legal argument"""
    rows = np.empty((t.num_selectors, n), dtype=np.uint64)
    for r in range(t.num_selectors):
        cls = rng.permutation(np.arange(n) % 3)
        idx = (rng.permutation(n) % (len(t.gates) + 1)).astype(np.uint64)
        rows[r] = np.where(cls == 0, idx, np.where(cls == 1, np.uint64(C.UNUSED_SELECTOR), _lattice(rng, n)))
    return rows


def filters(t, consts):
    """filter_g at every point as Python integers, [n_gates][N] (gates/gate.rs compute_filter)"""
    out = []
    for i, g in enumerate(t.gates):
        s = consts[g.selector_index].astype(object)
        f = np.ones(consts.shape[1], dtype=object)
        for r in range(g.group_start, g.group_end):
            if r != i:
                f = f * (r - s) % P
        if t.num_selectors > 1:
            f = f * (C.UNUSED_SELECTOR - s) % P
        out.append(f)
    return out


def alpha_reduce(cj, alpha):
    """sum_j alpha^j cj[j] mod p on Python integers: cj [J][N] -> uint64 [N]"""
    acc = np.zeros(cj.shape[1], dtype=object)
    for row in cj[::-1]:
        acc = (acc * int(alpha) + row.astype(object)) % P
    return acc.astype(np.uint64)


def constraints(t, consts, wires, pi_hash):
    """C_j of one proof at the points: [J][N]"""
    if not n_constraints(t):
        return np.zeros((0, wires.shape[1]), dtype=np.uint64)
    view = types.SimpleNamespace(gates=t.gates, gate_array=t.gate_array, num_selectors=t.num_selectors, pi_hash=pi_hash)
    return C.eval_on_points(view, consts, wires)


def reference(t, consts, wires, alphas, pi_hash):
    """want [B][nc][N], column p = the point of input column p"""
    want = np.zeros(alphas.shape + wires.shape[2:], dtype=np.uint64)
    for b in range(wires.shape[0]):
        cj = constraints(t, consts, wires[b], pi_hash[b])
        for a in range(alphas.shape[1]):
            want[b, a] = alpha_reduce(cj, alphas[b, a])
    return want


@functools.lru_cache(maxsize=24)
def case(name, opset, log_points, batch, alphas="uniform"):
    """one case, drawn from its own parameters alone: consts [ns + 2][N], wires [B][135][N], alphas [B][2], pi_hash [B][4] and
    want [B][2][N]; all read-only. nc = 1 is the first challenge of the same case: alphas[:, :1], want[:, :1]."""
    t = table(name)
    n = 1 << log_points
    rng = np.random.default_rng([zlib.crc32(("%s/%s/%s" % (name, opset, alphas)).encode()), log_points, batch])
    how_w, how_c = SETS[opset]
    c = types.SimpleNamespace(name=name, opset=opset, log_points=log_points, batch=batch, table=t)
    c.consts = np.concatenate([selector_rows(rng, t, n), _draw(rng, how_c, (2, n))])
    c.wires = _draw(rng, how_w, (batch, C.NUM_WIRES, n))
    if alphas == "uniform":
        c.alphas = _uniform(rng, (batch, 2))
    else:
        assert alphas == "edge" and batch == len(EDGE_ALPHAS)
        c.alphas = np.array(EDGE_ALPHAS, dtype=np.uint64)
    # the hash a PublicInputGate subtracts: from the lattice wherever the wires or the constants are
    c.pi_hash = _draw(rng, "l" if "l" in (how_w, how_c) else "u", (batch, 4))
    c.want = reference(t, c.consts, c.wires, c.alphas, c.pi_hash)
    for a in (c.consts, c.wires, c.alphas, c.pi_hash, c.want):
        a.setflags(write=False)
    return c


# shapes: the full cross product on three tables, one shape -- two blocks, three proofs -- on the rest
CROSS_TABLES = ("all", "light-14", "alone-7-0-0-0")
CROSS_SHAPES = [(lg, b) for lg in LOG_POINTS for b in (1, 3)]
REST_SHAPE = (9, 3)


def describe(c, t=None):
    t = t or c.table
    return "table %s (%s), set %s, 2^%d points, %d proofs" % (
        c.name, " ".join("%d:%d/%d/%d" % (g.kind, g.p0, g.p1, g.p2) for g in t.gates), c.opset, c.log_points, c.batch)


def first_mismatch(c, got):
    """None, or a message naming the table, the gate kinds, the proof, the challenge and the first wrong point with its selectors;
    got [B][nc][N] in the device's order (column bitrev(p))"""
    want = c.want[:, :got.shape[1]]
    got = got[:, :, bitrev_perm(c.log_points)]
    if np.array_equal(got, want):
        return None
    b, a, p = [int(x[0]) for x in np.nonzero(got != want)]
    return "%s: proof %d, challenge %d (alpha %#x), point %d (selectors %s): got %#x, want %#x; %d of %d words differ" % (
        describe(c), b, a, int(c.alphas[b, a]), p, " ".join("%#x" % int(s) for s in c.consts[:c.table.num_selectors, p]),
        int(got[b, a, p]), int(want[b, a, p]), int(np.count_nonzero(got != want)), want.size)
