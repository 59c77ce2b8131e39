"""Circuits and input vectors that put the witness replay (csrc/witness_ops.h, csrc/witness_dev.hip) on edge operands and on the
boundaries of the device's level loop. The reference is recursion.Builder(strict=False): it computes every wire eagerly in Python
integers while it records the tape, one build per input vector. Three kinds of family, each one tape replayed as one batch:

  "opcodes"                      one instruction or more of every base opcode 1..23, the gates at the limits of their parameters
  "p2_coop", "p2_lanes",         Poseidon2Gate / PoseidonGate rows whose inputs are raw input words (lattice states, not hash outputs):
  "poseidon"                     8 rows on level 1 (the 16-lane cooperative body), 65 rows (one lane per row), 8 PoseidonGate rows
  "chain_plain", "chain_gf5",    a chain of levels with 1, 31, 32, 33, 63, 64, 65 Poseidon2 rows, companions on both sides of
  "chain_wide", "chain_lookup"   MP2G_OP_P2 in opcode order on every level, two levels with more companions than the block has lanes;
                                 one instruction more selects the kernel instance

The CPU side is tests/test_witness_edge_cases.py, the device side tests/test_gpu_witness_replay_edges.py. Builds are cached here, per
family, for both."""
import functools
import importlib
import types

import numpy as np

import field_cases as FC
import oracle as O

R = importlib.import_module("mapreduce-plonky2_amd.recursion")
MP2 = importlib.import_module("mapreduce-plonky2_amd")
C = importlib.import_module("mapreduce-plonky2_amd.circuits")
P, EC, U32 = FC.P, FC.EC, 0xFFFFFFFF
G16 = R.root_of_unity(4)
N_DRAWS = 17  # seeded draws from the lattice per family of 24 vectors or more

# ---- 1. the opcode circuit ------------------------------------------------------------------------------------------------------------
# the input vector by name: (field, words); the Builder's input order is this order
OPCODE_LAYOUT = [("arith", 3), ("arith_ext", 6), ("state", 12), ("swap", 1), ("pstate", 12), ("pswap", 1), ("bits63", 1), ("ra_index", 1),
                 ("ra_values", 16), ("alpha", 2), ("base_terms", 44), ("ext_terms", 66), ("coset_shift", 1), ("coset_values", 32),
                 ("coset_point", 2), ("div_num", 2), ("div_den", 2), ("eq", 2), ("split64", 1), ("slh1", 1), ("slh63", 1), ("u32_arith", 3),
                 ("u32_sub", 3), ("add_many", 17), ("range_check", 1), ("cmp63", 2), ("cmp32", 2), ("cmp1", 2), ("cmp_same", 1),
                 ("base4", 1), ("mul_ext", 4), ("exp_base", 1), ("exp_bits", 66)]
OPCODE_WORDS = sum(n for _, n in OPCODE_LAYOUT)


def fields(vec):
    """an opcode-circuit input vector as {field: its words}"""
    out, at = {}, 0
    for name, n in OPCODE_LAYOUT:
        out[name] = [int(x) for x in vec[at:at + n]]
        at += n
    assert at == len(vec)
    return out


def flat(f):
    return [x for name, _ in OPCODE_LAYOUT for x in f[name]]


def _ext(ws):
    return [R.E(ws[i], ws[i + 1]) for i in range(0, len(ws), 2)]


def opcode_circuit(vec):
    """every base opcode of the tape in one circuit: the recursion circuits' gates and hints, the leaf circuits' gates at the limits of
    what mp2g_witness_program_create accepts (63-bit comparisons in 16 chunks and in one, 16 addends, 66 exponent bits, 31 base-4
    limbs), one parallel region; public inputs from every family of outputs"""
    v = fields(vec)
    b = R.Builder(strict=False)
    t = {name: [b.add_virtual(x) for x in v[name]] for name, _ in OPCODE_LAYOUT}
    a, e = t["arith"], _ext(t["arith_ext"])
    y0 = b.arithmetic(P - 1, a[0], a[1], P - 2, a[2])
    y1 = b.arithmetic(P - 2, y0, a[0], P - 1, a[1])
    z0 = b.arithmetic_ext(P - 2, e[0], e[1], P - 1, e[2])
    z1 = b.arithmetic_ext(P - 1, z0, e[0], P - 2, e[1])
    with b.parallel_sections() as region:
        with region.section():
            y2 = b.arithmetic(P - 1, a[2], a[0], P - 2, a[1])
        with region.section():
            z2 = b.arithmetic_ext(P - 2, e[2], e[0], P - 1, e[1])
    h = b.permute_swapped(t["state"], t["swap"][0])
    hp = b.permute_poseidon_swapped(t["pstate"], t["pswap"][0])
    bits = b.split_le_base2(t["bits63"][0], 63)
    ra = b.random_access(t["ra_index"][0], t["ra_values"])
    alpha = _ext(t["alpha"])[0]
    rb = b.reduce_base(alpha, t["base_terms"])
    rx = b.reduce_ext(alpha, _ext(t["ext_terms"]))
    ci = b.interpolate_coset(4, t["coset_shift"][0], _ext(t["coset_values"]), _ext(t["coset_point"])[0])
    q = b.div_ext(_ext(t["div_num"])[0], _ext(t["div_den"])[0])
    eq = b.is_equal(t["eq"][0], t["eq"][1])
    bits64 = b.split_le(t["split64"][0], 64)
    lo1, hi1 = b.split_low_high(t["slh1"][0], 1, 64)
    lo63, hi63 = b.split_low_high(t["slh63"][0], 63, 64)
    ulo, uhi = b.u32_arithmetic(*t["u32_arith"])
    sr, sb = b.u32_sub(*t["u32_sub"])
    am, ac = b.u32_add_many(t["add_many"][:16], t["add_many"][16], ops=1)
    b.u32_range_check(t["range_check"][0])
    c63 = b.comparison_le(t["cmp63"][0], t["cmp63"][1], 63, 16)
    c32 = b.comparison_le(t["cmp32"][0], t["cmp32"][1], 32, 16)
    c1 = b.comparison_le(t["cmp1"][0], t["cmp1"][1], 63, 1)
    cs = b.comparison_le(t["cmp_same"][0], t["cmp_same"][0], 32, 16)
    limbs = b.base_split(t["base4"][0], 2, 31)
    m = _ext(t["mul_ext"])
    me = b.mul_ext_gate(P - 1, m[0], m[1])
    ex = b.exponentiation(t["exp_base"][0], t["exp_bits"])
    b.register_public_inputs([y1, y2, z1.a, z1.b, z2.a, z2.b, h[0], h[11], hp[0], hp[11], bits[0], bits[62], ra, rb.a, rb.b, rx.a, rx.b, ci.a,
                              ci.b, q.a, q.b, eq, bits64[0], bits64[63], lo1, hi1, lo63, hi63, ulo, uhi, sr, sb, am, ac, c63, c32, c1, cs,
                              limbs[0], limbs[30], me.a, me.b, ex])
    return b.build()


def _draw(words, seed):
    rng = np.random.default_rng([0xED6E, seed])
    return [EC[int(i)] for i in rng.integers(0, len(EC), words)]


def _uniform(rng, n, hi=P):
    return [int(x) for x in rng.integers(0, hi, n, dtype=np.uint64)]


def domain_fields(seed=1):
    """a vector on which every gate's precondition holds: u32 words for the u32 gates, values below 2^63 (2^62 for the base-4
    split) for the splits and comparisons, an index below 16, boolean swaps and exponent bits, non-zero divisor and coset shift"""
    rng = np.random.default_rng([0xD03A, seed])
    f = {name: _uniform(rng, n) for name, n in OPCODE_LAYOUT}
    f["swap"], f["pswap"] = [1], [1]
    f["bits63"] = _uniform(rng, 1, 1 << 63)
    f["ra_index"] = [11]
    f["coset_shift"] = [f["coset_shift"][0] or 1]
    f["div_den"] = [f["div_den"][0] or 1, f["div_den"][1]]
    f["u32_arith"] = _uniform(rng, 3, 1 << 32)
    f["u32_sub"] = _uniform(rng, 2, 1 << 32) + [1]
    f["add_many"] = _uniform(rng, 16, 1 << 32) + [9]
    f["range_check"] = _uniform(rng, 1, 1 << 32)
    f["cmp63"], f["cmp1"] = _uniform(rng, 2, 1 << 63), _uniform(rng, 2, 1 << 63)
    f["cmp32"], f["cmp_same"] = _uniform(rng, 2, 1 << 32), _uniform(rng, 1, 1 << 32)
    f["base4"] = _uniform(rng, 1, 1 << 62)
    f["exp_bits"] = _uniform(rng, 66, 2)
    return f


def corner_fields():
    """two vectors that hold, whatever the draws give, the corners tests/test_witness_edge_cases.py asserts from the inputs alone"""
    a, b = domain_fields(2), domain_fields(3)
    a["div_den"], a["coset_shift"], a["ra_index"] = [0, 0], [0], [16 + 7]
    a["u32_sub"], a["u32_arith"], a["add_many"] = [0, U32, 1], [U32] * 3, [U32] * 16 + [1]
    a["cmp63"] = [a["cmp63"][0], a["cmp63"][0] ^ (1 << 62)]  # chunk 15 of 16 four-bit chunks
    a["cmp32"] = [a["cmp32"][0], a["cmp32"][0] ^ (1 << 31)]  # chunk 15 of 16 two-bit chunks
    a["exp_bits"] = [2, P - 1, U32] + a["exp_bits"][3:]
    a["swap"], a["pswap"] = [P - 1], [P - 1]
    b["coset_point"] = [b["coset_shift"][0] * pow(G16, 5, P) % P, 0]
    b["cmp63"] = [b["cmp63"][0], b["cmp63"][0] ^ 1]
    b["cmp32"] = [b["cmp32"][0], b["cmp32"][0] ^ 1]
    b["cmp1"] = [b["cmp1"][0], b["cmp1"][0]]
    b["ra_index"] = [P - 2]
    return a, b


DOMAIN_VECTOR = 4  # its place in opcode_vectors()


@functools.lru_cache(maxsize=None)
def opcode_vectors():
    vs = [[x] * OPCODE_WORDS for x in (0, 1, P - 1, U32)] + [flat(domain_fields())] + [flat(f) for f in corner_fields()]
    return vs + [_draw(OPCODE_WORDS, k) for k in range(N_DRAWS)]


def _chunks(x, bits, n):
    return [(x >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]


def _differ_only_in(pair, bits, n, where):
    ca, cb = _chunks(pair[0], bits, n), _chunks(pair[1], bits, n)
    return [i for i in range(n) if ca[i] != cb[i]] == [where]


# the corners of the opcodes themselves: name -> predicate over a vector's fields
CORNERS = {
    "zero div_ext denominator": lambda f: f["div_den"] == [0, 0],
    "zero coset shift": lambda f: f["coset_shift"] == [0],
    "interpolation point on the coset": lambda f: f["coset_shift"][0] != 0 and f["coset_point"][1] == 0 and
    f["coset_point"][0] in {f["coset_shift"][0] * pow(G16, i, P) % P for i in range(16)},
    "random-access index of 16 or more": lambda f: f["ra_index"][0] >= 16,
    "u32_sub of 0 - u32::MAX - 1": lambda f: f["u32_sub"] == [0, U32, 1],
    "u32_arithmetic of u32::MAX^2 + u32::MAX": lambda f: f["u32_arith"] == [U32] * 3,
    "sixteen addends of u32::MAX with carry 1": lambda f: f["add_many"] == [U32] * 16 + [1],
    "equal comparison operands": lambda f: f["cmp63"][0] == f["cmp63"][1] and f["cmp32"][0] == f["cmp32"][1] and f["cmp1"][0] == f["cmp1"][1],
    "comparison operands that differ in the top chunk only": lambda f: _differ_only_in(f["cmp63"], 4, 16, 15) and _differ_only_in(f["cmp32"], 2, 16, 15),
    "comparison operands that differ in the bottom chunk only": lambda f: _differ_only_in(f["cmp63"], 4, 16, 0) and _differ_only_in(f["cmp32"], 2, 16, 0),
    "exponent bits that are not 0 or 1": lambda f: any(x > 1 for x in f["exp_bits"]),
    "swap of p - 1": lambda f: f["swap"] == [P - 1] and f["pswap"] == [P - 1],
}


# ---- 2. Poseidon2 gate paths ------------------------------------------------------------------------------------------------------------
P2_WORDS = 24 + 4  # two states and four swaps


def p2_row_state(v, j):
    """what row j of a gate-path circuit permutes: the vector's first state in the even rows, its second in the odd ones, rotated by j"""
    return [v[12 * (j & 1) + (i + j) % 12] for i in range(12)]


def p2_row_swap(v, j):
    return v[24 + j % 4]


def p2_rows_circuit(vec, rows, poseidon=False):
    """`rows` Poseidon2Gate (or PoseidonGate) rows on level 1, each on raw input words"""
    b = R.Builder(strict=False)
    v = [b.add_virtual(int(x)) for x in vec]
    perm = b.permute_poseidon_swapped if poseidon else b.permute_swapped
    outs = [perm(p2_row_state(v, j), p2_row_swap(v, j)) for j in range(rows)]
    b.register_public_inputs(outs[0] + [o[j % 12] for j, o in enumerate(outs) if j])
    return b.build()


@functools.lru_cache(maxsize=None)
def p2_vectors():
    """the kinds of vector of the opcode circuit, then every state of twelve equal lattice words (two to a vector; the even rows see
    swaps 0 and 1, the odd ones 0 and p - 1)"""
    rng = np.random.default_rng(0x9A7E)
    vs = [[x] * P2_WORDS for x in (0, 1, P - 1, U32)] + [_uniform(rng, 24) + [0, 1, 1, 0]]
    vs += [_draw(24, 100 + k) + [0, 0] + _draw(2, 200 + k) for k in range(N_DRAWS - 1)]
    pairs = [(EC[i], EC[min(i + 1, len(EC) - 1)]) for i in range(0, len(EC), 2)]
    return vs + [[x] * 12 + [y] * 12 + [0, 0, 1, P - 1] for x, y in pairs]


def p2_expected_rows(vec, rows):
    """[(row j, the state the permutation sees)] for the rows whose swap is 0 or 1: what an independent permutation must reproduce"""
    out = []
    for j in range(rows):
        s, sw = p2_row_state(vec, j), p2_row_swap(vec, j)
        if sw == 0:
            out.append((j, s))
        elif sw == 1:
            out.append((j, s[4:8] + s[:4] + s[8:]))
    return out


# ---- 3. level-loop boundaries -----------------------------------------------------------------------------------------------------------
CHAIN_P2 = (1, 31, 32, 33, 63, 64, 65)  # Poseidon2 rows on levels 1..7: around one group, one round of 32 groups, two rounds
CHAIN_HEAVY = (3, 7)                     # the levels (32 rows: cooperative, 65 rows: a lane per row) with more than 512 companions
CHAIN_WORDS = 16
INSTANCES = ("plain", "gf5", "wide", "lookup")


def chain_circuit(vec, instance="plain"):
    """level k holds CHAIN_P2[k - 1] Poseidon2 rows, each on raw input words and exactly one output of level k - 1 (none on level 1),
    and companions that read one output of level k - 1 too: arithmetic and arithmetic_ext (opcodes below MP2G_OP_P2), a bit split,
    two random accesses and three range checks (above it). The instance's one instruction reads constants only."""
    b = R.Builder(strict=False)
    v = [b.add_virtual(int(x)) for x in vec]
    if instance == "gf5":
        b.quintic_quotient([b.constant(3 + i) for i in range(5)], [b.constant(P - 1 - i) for i in range(5)])
    elif instance == "wide":
        b.u32_interleave(b.constant(0x89ABCDEF))
    elif instance == "lookup":
        b.add_lookup_from_index(b.constant(0xA5), b.add_lookup_table_from_fn(lambda x: (x * 167 + 13) & 0xFFFF, range(256)))
    else:
        assert instance == "plain"
    prev = []
    for k, count in enumerate(CHAIN_P2, start=1):
        src = prev or v
        outs = []
        for j in range(count):
            s = [v[(i + j) % 12] for i in range(12)]
            if prev:
                s[j % 12] = prev[(5 * j) % len(prev)]
            outs += b.permute_swapped(s, v[12 + j % 4])
        x = lambda i: src[(7 * i + k) % len(src)]
        for i in range(2 + (520 if k in CHAIN_HEAVY else 0)):
            b.arithmetic(P - 1, x(i), v[i % 16], P - 2, v[(i + 3) % 16])
        for i in range(2):
            b.arithmetic_ext(P - 2, R.E(x(i), v[i]), R.E(v[i + 1], x(i + 1)), P - 1, R.E(v[i + 2], v[i + 3]))
        b.split_le_base2(x(0), 63)
        b.random_access(x(1), v)
        b.random_access(v[13], [x(2)] + v[1:])
        for i in range(3):
            b.u32_range_check(x(i))
        prev = outs
    b.register_public_inputs(prev[:8])
    return b.build()


@functools.lru_cache(maxsize=None)
def chain_vectors():
    rng = np.random.default_rng(0xC4A1)
    return [[x] * CHAIN_WORDS for x in (0, 1, P - 1, U32)] + [_uniform(rng, CHAIN_WORDS)] + [_draw(CHAIN_WORDS, 300 + k) for k in range(3)]


def level_schedule(tape):
    """[(tape position, opcode, level)] as the library schedules a program: level = 1 + the highest level of the slots read (inputs
    and constants sit on level 0)"""
    lvl, out = {}, []
    for pos, op in R.tape_instructions(tape):
        if op == R.OP_PAR:
            continue
        rd, wr, _, _ = R.instruction_slots(tape, pos)
        l = 1 + max([lvl.get(int(s), 0) for s in rd], default=0)
        for s in wr:
            lvl[int(s)] = l
        out.append((pos, op, l))
    return out


def levels_by_opcode(tape):
    """{level: {opcode: count}}"""
    out = {}
    for _, op, l in level_schedule(tape):
        out.setdefault(l, {})
        out[l][op] = out[l].get(op, 0) + 1
    return out


def check_chain_shape(ck, instance):
    """the shape of a chain circuit, from its tape alone, as the device's level loop sees it: the Poseidon2 rows of every level, companions
    on both sides of MP2G_OP_P2 in opcode order on each, more than 512 companions on the heavy levels and nowhere else, the instance's
    one instruction on level 1. -> the number of levels"""
    assert ck.log_n == 9
    levels = levels_by_opcode(ck.tape)
    n_chain = len(CHAIN_P2)
    assert [levels[l].get(R.OP_P2, 0) for l in sorted(levels)] == list(CHAIN_P2) + [1, 0]  # then the public-inputs hash and its wires
    for l in range(1, n_chain + 1):
        below = sum(c for op, c in levels[l].items() if op < R.OP_P2)
        above = sum(c for op, c in levels[l].items() if op > R.OP_P2)
        assert {R.OP_ARITH, R.OP_ARITH_EXT, R.OP_BASE_SUM, R.OP_RA, R.OP_U32_RANGE_CHECK} <= set(levels[l])
        assert below >= 4 and above >= 6
        assert (below + above > 512) == (l in CHAIN_HEAVY), (l, below, above)
    assert [CHAIN_P2[l - 1] for l in CHAIN_HEAVY] == [32, 65]
    extra = {"plain": None, "gf5": 33, "wide": 48, "lookup": 40}[instance]  # include/mp2g.h: MP2G_OP_QUINTIC_QUOTIENT, _U32_INTERLEAVE, _LOOKUP
    others = {op for l in levels for op in levels[l] if op >= 24}
    assert others == ({extra} if extra else set()) and (extra is None or levels[1][extra] == 1)
    return max(levels)


# ---- the families -----------------------------------------------------------------------------------------------------------------------
FAMILIES = ("opcodes", "p2_coop", "p2_lanes", "poseidon") + tuple("chain_" + i for i in INSTANCES)
P2_ROWS = {"p2_coop": 8, "p2_lanes": 65, "poseidon": 8}


@functools.lru_cache(maxsize=None)
def family(name):
    """(input vectors as uint64 [B][words], one built circuit per vector) of a family"""
    if name == "opcodes":
        vs, make = opcode_vectors(), opcode_circuit
    elif name in P2_ROWS:
        vs, make = p2_vectors(), lambda v: p2_rows_circuit(v, P2_ROWS[name], poseidon=name == "poseidon")
    else:
        vs, make = chain_vectors(), lambda v: chain_circuit(v, name[len("chain_"):])
    return np.array(vs, dtype=np.uint64), [make(v) for v in vs]


def p2_gate_rows(ckt, op):
    """the rows of a circuit's Poseidon2Gate (op = R.OP_P2) or PoseidonGate instructions, in tape order"""
    return [int(ckt.tape[pos + 1]) for pos, o in R.tape_instructions(ckt.tape) if o == op]


def mismatch(got, want):
    col, row = (int(x[0]) for x in np.nonzero(got != want))
    return f"wire {col} of row {row}: {int(got[col, row]):#x}, the builder has {int(want[col, row]):#x}"


def check_permutations(name, a, ck, wires):
    """outputs 12..23 of the rows whose swap is 0 or 1 against the oracle's permutation of the state"""
    rows, variant = P2_ROWS[name], 1 if name == "poseidon" else 0
    where = p2_gate_rows(ck, R.OP_POSEIDON if variant else R.OP_P2)
    seen = 0
    for k, vec in enumerate(a.tolist()):
        for j, state in p2_expected_rows(vec, rows):
            assert np.array_equal(wires[k][12:24, where[j]], O.perm(state, variant)), (k, j)
            seen += 1
    assert seen >= len(a) * rows // 2


# ---- a second opinion on the wire layout: the oracle's gate evaluators ---------------------------------------------------------------------
def comparison_row_holds(w, num_bits, num_chunks):
    """ComparisonGate's constraints ([dep] plonky2-u32 gates/comparison.rs) on one row's wires w, in Python integers, with each chunk's
    range product -- 2^chunk_bits factors, 2^63 of them for one chunk of 63 bits -- replaced by the range test it stands for"""
    w = [int(x) for x in w]
    nc, cb = num_chunks, (num_bits + num_chunks - 1) // num_chunks
    fc, sc, ed, ce, iv = (w[4 + k * nc:4 + (k + 1) * nc] for k in range(5))
    bits = w[4 + 5 * nc:4 + 5 * nc + cb + 1]
    ok = sum(c << (cb * i) for i, c in enumerate(fc)) % P == w[0] and sum(c << (cb * i) for i, c in enumerate(sc)) % P == w[1]
    msd = 0
    for i in range(nc):
        diff = (sc[i] - fc[i]) % P
        ok = ok and fc[i] < 1 << cb and sc[i] < 1 << cb and (diff * ed[i] - (1 - ce[i])) % P == 0 and ce[i] * diff % P == 0
        ok = ok and (iv[i] - ce[i] * msd) % P == 0
        msd = (iv[i] + (1 - ce[i]) * diff) % P
    ok = ok and w[3] == msd and all(x in (0, 1) for x in bits)
    return ok and ((1 << cb) + w[3] - sum(x << i for i, x in enumerate(bits))) % P == 0 and w[2] == bits[cb]


def gate_constraints_hold(ckt, wires, evaluate):
    """every gate constraint of ckt vanishes on `wires` [135][n] under evaluate = tests/circuits.py eval_on_points. A ComparisonGate
    whose chunks are wider than 4 bits has a constraint of 2^chunk_bits factors, which no evaluator runs through: the evaluator sees
    a Noop in its place (the same selector, so every other gate's filter is what it was) and its rows go to comparison_row_holds."""
    gates, ok = [], True
    for i, g in enumerate(ckt.gates):
        g2 = MP2.Gate(g.kind, g.p0, g.p1, g.p2, g.selector_index, g.group_start, g.group_end)
        if g.kind == C.COMPARISON and C.gate_degree(g) > 16:
            g2.kind, g2.p0, g2.p1 = C.NOOP, 0, 0
            rows = [r for r, inst in enumerate(ckt.instances) if inst == i]
            ok = ok and bool(rows) and all(comparison_row_holds(wires[:, r], g.p0, g.p1) for r in rows)
        gates.append(g2)
    view = types.SimpleNamespace(gates=gates, gate_array=(MP2.Gate * len(gates))(*gates), num_selectors=ckt.num_selectors, pi_hash=ckt.pi_hash)
    return ok and not evaluate(view, ckt.pre[:ckt.num_constants], wires).any()
