"""Proofs of a dishonest FRI prover, shared by the CPU-only test of the list (test_forged_fri_cases.py) and the device test
(test_gpu_forged_proofs.py). The oracle's prover, armed with orc_set_fri_tamper, changes some values of one committed FRI layer (or
one coefficient of the final polynomial) and then commits honestly to what it chose: every Merkle path of such a proof holds, the
transcript is the proof's own, and only the verifier's field checks -- layer consistency (3) and the final polynomial (5) -- can
reject it. A single-word mutation of a finished proof never gets that far: it breaks a path or the transcript first.

For every forged proof the first failing check is predicted here in plain Python from the tampered positions and the query indices
alone (predict), without folding anything: a verifier is compared with that prediction and with the oracle's verifier. A few forged
proofs also get one Merkle sibling bumped (siblings are not observed, so the indices stay), which puts a path failure (2, 4) before,
after or beside the field failure: which of several failures is reported is part of what is checked.

A helper module: nothing here touches the device. Proofs are made once per process and shared; treat the arrays as read-only."""
import functools
from collections import namedtuple

import numpy as np

import circuits as C
import fri_param_cases as FC
import oracle as O

P = O.P
OMP_TEAM = 4  # oracle threads per proof: some 700 proofs of 2^5 .. 2^7 rows are made here (see oracle.omp_threads)
DIGEST_SEED = 0xD16E57  # any four words: the oracle and CircuitVerifier(circuit_digest=) take the verifier data as given

# kw: keywords of C.oracle_params; layers: arity_bits set by hand after it (None: what ConstantArityBits gives)
Shape = namedtuple("Shape", "name log_n kinds variant kw layers")
MIXED_KW = (("cap_height", 2), ("num_queries", 6), ("pow_bits", 3))
SHAPES = (
    [Shape("std5", 5, "ALL_KINDS", 0, (), None), Shape("std6", 6, "ALL_KINDS", 0, (), None)]
    + [Shape(c.name + (f"-v{v}" if c.name == "all6_arity2" else ""), c.log_n, c.kinds, v, c.kw, None)
       for c in FC.CIRCUIT_CASES for v in ((0, 1) if c.name == "all6_arity2" else (0,))]
    + [Shape(f"all7_mixed-v{v}", 7, "ALL_KINDS", v, MIXED_KW, (3, 2, 1)) for v in (0, 1)]
)
DELTAS = ((1, 0), (0, 1), (P - 1, P - 1))
FINAL_DELTAS = ((1, 0), (0, 1))

# stage < n_layers: delta added to layer `stage` at first + k * stride, k < count; stage == n_layers: to final coefficient `first`
Case = namedtuple("Case", "stage first count stride delta")
# one entry of a shape's catalogue. bump: None or (kind, query, flat FRI word, the failure it adds); fails: every predicted failing
# (query, position, code), sorted, so fails[0] is what a verifier reports
Forged = namedtuple("Forged", "case bump caps openings proof indices fails")


def circuit(shape):
    return FC.circuit(shape.log_n, shape.kinds)


def params(shape):
    """a fresh oracle parameter struct of the shape (ctypes: not hashable, so not cached)"""
    fp = C.oracle_params(circuit(shape), shape.variant, **dict(shape.kw))
    if shape.layers is not None:
        fp.n_layers = len(shape.layers)
        for i in range(8):
            fp.arity_bits[i] = shape.layers[i] if i < len(shape.layers) else 0
    return fp


def digest():
    return O.rand_field(4, DIGEST_SEED)


def layers(fp):
    return [int(fp.arity_bits[i]) for i in range(fp.n_layers)]


def layer_len(fp, li):
    """values of layer li"""
    return 1 << (fp.log_n + fp.rate_bits - sum(layers(fp)[:li]))


def final_len(fp):
    return 1 << (fp.log_n - sum(layers(fp)))


Layout = namedtuple("Layout", "capw q_off q_words leaf_off sib_off n_sib final_off")


def layout(fp):
    """word offsets in the flat FRI proof (oracle/fri.c): the layer caps, then per query and path p (the n_oracles initial trees,
    then the layers) leaf_off[p], sib_off[p] inside the query's q_words and n_sib[p] siblings of 4 words; final polynomial; PoW"""
    capw = 4 << fp.cap_height
    lg = fp.log_n + fp.rate_bits
    leaf_off, sib_off, n_sib, at = [], [], [], 0
    for o in range(fp.n_oracles):
        leaf_off.append(at)
        sib_off.append(at + fp.oracle_w[o])
        n_sib.append(lg - fp.cap_height)
        at += fp.oracle_w[o] + 4 * n_sib[-1]
    cur = lg
    for ab in layers(fp):
        cur -= ab
        leaf_off.append(at)
        sib_off.append(at + (2 << ab))
        n_sib.append(cur - fp.cap_height)
        at += (2 << ab) + 4 * n_sib[-1]
    q_off = fp.n_layers * capw
    return Layout(capw, q_off, at, leaf_off, sib_off, n_sib, q_off + fp.num_queries * at)


def plans(m, arity):
    """[(first, count, stride)] for a layer of m values in cosets of `arity`; plans that name the same positions appear once"""
    cosets = m // arity
    out = [(0, m, 1)]
    out += [(w, cosets, arity) for w in (0, 1, arity - 1)]
    out += [(c * arity, arity, 1) for c in (0, cosets // 3, cosets - 1)]
    out += [(0, m // 2, 1), (m // 2, m // 2, 1)]
    out += [(m // 3, 1, 1), (m - 1, 1, 1)]
    seen, uniq = set(), []
    for pl in out:
        key = tuple(range(pl[0], pl[0] + pl[1] * pl[2], pl[2]))
        if key not in seen:
            seen.add(key)
            uniq.append(pl)
    return uniq


def cases(shape):
    fp = params(shape)
    out = []
    for li, ab in enumerate(layers(fp)):
        out += [Case(li, f, c, s, d) for (f, c, s) in plans(layer_len(fp, li), 1 << ab) for d in DELTAS]
    fl = final_len(fp)
    out += [Case(fp.n_layers, i, 1, 1, d) for i in sorted({0, fl // 2, fl - 1}) for d in FINAL_DELTAS]
    return out


def plan_size(fp, case):
    """how many values the hook must change"""
    if case.stage == fp.n_layers:
        return 1 if case.first < final_len(fp) else 0
    m = layer_len(fp, case.stage)
    return sum(1 for k in range(case.count) if case.first + k * case.stride < m)


def tampered(case, j):
    """is position j of the case's layer one the hook changed"""
    k, r = divmod(j - case.first, case.stride)
    return j >= case.first and r == 0 and k < case.count


@functools.lru_cache(maxsize=None)
def honest(shape):
    """(caps, openings, proof) of the oracle's honest prover"""
    with O.omp_threads(OMP_TEAM):
        return C.prove(circuit(shape), params(shape), digest())[:3]


@functools.lru_cache(maxsize=None)
def forged(shape, case):
    """(caps, openings, proof) of the oracle's prover with the tamper hook armed"""
    fp = params(shape)
    with O.omp_threads(OMP_TEAM):
        O.set_fri_tamper(case.stage, case.first, case.count, case.stride, case.delta)
        out = C.prove(circuit(shape), fp, digest())[:3]
    assert O.fri_tamper_applied() == plan_size(fp, case) > 0, (shape.name, case, O.fri_tamper_applied())
    return out


def query_indices(shape, caps, openings, proof):
    """the verifier's transcript replayed on the oracle's challenger: circuit digest, public-inputs hash, the caps with the betas /
    gammas (and, with lookups, 2 more per challenge round) and alphas drawn between them, zeta, the openings, FRI alpha, each layer
    cap and its beta, the final polynomial, the PoW witness and its response; then one index per query"""
    ckt, fp = circuit(shape), params(shape)
    L = layout(fp)
    nc = fp.zs_count
    ch = O.Challenger(fp.variant)
    ch.observe(digest())
    ch.observe(ckt.pi_hash)
    for o in range(1, fp.n_oracles):
        ch.observe(caps[o])
        if o == 1:
            ch.get((4 if ckt.luts and fp.num_lookup_polys else 2) * nc)
        elif o == 2:
            ch.get(nc)
    ch.get(2)
    ch.observe(openings)
    ch.get(2)
    for li in range(fp.n_layers):
        ch.observe(proof[li * L.capw:(li + 1) * L.capw])
        ch.get(2)
    ch.observe(proof[L.final_off:L.final_off + 2 * final_len(fp) + 1])  # the witness follows the coefficients
    ch.get(1)
    N = 1 << (fp.log_n + fp.rate_bits)
    return [int(x) % N for x in ch.get(fp.num_queries)]


def predict(fp, case, indices):
    """every failing (query, position, code) of the forged proof, sorted. Positions are the verifier's order inside a query:
    0 initial paths; 1 + 2 li consistency of layer li; 2 + 2 li its path; 1 + 2 n_layers the final polynomial. A query whose own
    place in the tampered layer was changed fails that layer's consistency check; one that reads another changed place of its
    coset folds it into a wrong value, which the next check -- the next layer's consistency, or the final polynomial -- refuses"""
    ab, n = layers(fp), fp.n_layers
    fails = []
    for q, x in enumerate(indices):
        if case.stage == n:
            fails.append((q, 1 + 2 * n, 5))
            continue
        li = case.stage
        j = x >> sum(ab[:li])
        arity = 1 << ab[li]
        if tampered(case, j):
            fails.append((q, 1 + 2 * li, 3))
        if any(tampered(case, c) for c in range(j & ~(arity - 1), (j | (arity - 1)) + 1) if c != j):
            fails.append((q, 1 + 2 * (li + 1), 3) if li + 1 < n else (q, 1 + 2 * n, 5))
    return sorted(fails)


def status(fails):
    """what a verifier reports: the code of the first failing check of the lowest failing query, 0 when nothing fails"""
    return min(fails)[2] if fails else 0


def status_position_major(fails):
    """what a verifier that ordered its failures by check first and query second would report"""
    return min((pos, q, code) for q, pos, code in fails)[2] if fails else 0


def path_bumps(fp, first_fail, num_queries):
    """[(kind, query, flat FRI word, added failure)] around a first failure (q, pos, code) with q >= 1: one word of one sibling
    each; kinds the shape has no sibling for are left out"""
    q, pos, _ = first_fail
    L = layout(fp)

    def word(query, p):
        return L.q_off + query * L.q_words + L.sib_off[p] + 4 * (L.n_sib[p] // 2) + 2

    out = []
    no = fp.n_oracles
    if L.n_sib[0]:
        out.append(("initial path of the query before", q - 1, word(q - 1, (q - 1) % no), (q - 1, 0, 2)))
        if q + 1 < num_queries:
            out.append(("initial path of the query after", q + 1, word(q + 1, (q + 1) % no), (q + 1, 0, 2)))
    li = (pos - 1) // 2  # the failing check is layer li's consistency, or (li == n_layers) the final polynomial
    if li < fp.n_layers and L.n_sib[no + li]:
        out.append(("the failing layer's own path", q, word(q, no + li), (q, 2 + 2 * li, 4)))
    earlier = [l for l in range(min(li, fp.n_layers)) if L.n_sib[no + l]]
    if earlier:
        l = earlier[-1]
        out.append(("an earlier layer's path", q, word(q, no + l), (q, 2 + 2 * l, 4)))
    return out


@functools.lru_cache(maxsize=None)
def catalogue(shape):
    """[Forged]: every case of the shape, then the path combinations of up to four of them"""
    fp = params(shape)
    out = []
    for case in cases(shape):
        caps, openings, proof = forged(shape, case)
        idx = query_indices(shape, caps, openings, proof)
        out.append(Forged(case, None, caps, openings, proof, idx, predict(fp, case, idx)))
    # up to four proofs whose first failure is in a query >= 1, one per failing position first
    late = [f for f in out if f.fails and f.fails[0][0] >= 1]
    chosen = []
    for f in late:
        if f.fails[0][1] not in {c.fails[0][1] for c in chosen}:
            chosen.append(f)
    chosen = (chosen + [f for f in late if all(f is not c for c in chosen)])[:4]
    for f in chosen:
        for bump in path_bumps(fp, f.fails[0], fp.num_queries):
            proof = f.proof.copy()
            FC.bump(proof, bump[2])
            out.append(Forged(f.case, bump, f.caps, f.openings, proof, f.indices, sorted(f.fails + [bump[3]])))
    return out


def label(f):
    """(plan, delta, bump) for a report"""
    c = f.case
    return ((c.stage, c.first, c.count, c.stride), tuple(int(d) for d in c.delta), f.bump[:2] if f.bump else None)


def tally(shape):
    """what the shape's catalogue holds: cases, predicted codes, and how many cases a position-major minimum would get wrong"""
    cat = catalogue(shape)
    codes = {}
    for f in cat:
        codes[status(f.fails)] = codes.get(status(f.fails), 0) + 1
    return {"cases": len(cat), "codes": dict(sorted(codes.items())),
            "order_sensitive": sum(status(f.fails) != status_position_major(f.fails) for f in cat),
            "first_failure_past_query_0": sum(bool(f.fails) and f.fails[0][0] >= 1 for f in cat)}
