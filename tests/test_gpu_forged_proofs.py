"""The device verifier (csrc/verifier.hip) on the forged proofs of forged_fri_cases.py: proofs of a dishonest FRI prover whose
Merkle paths all hold, so that only the field checks can reject them -- the layer consistency comparison (3), the fold it feeds into
the next check, the final-polynomial comparison (5) -- and, with one sibling bumped as well, proofs that fail several checks in
several queries, where the report is the first failing check of the lowest failing query (the key packed by query_fail and the low
byte kept by verifier_status_kernel). The device's status is compared with the CPU oracle's verifier and with the plain-Python
prediction of forged_fri_cases.predict, never with the device itself; test_forged_fri_cases.py shows on the CPU that the two
references agree and that the list reaches every one of these checks.
No device prover is needed: the verifier is given the oracle proof's own constants_sigmas cap and the digest the oracle proved under."""
import importlib

import numpy as np
import pytest

import circuits as C
import forged_fri_cases as FF
from test_gpu_fri import to_mp2

pytestmark = pytest.mark.gpu
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)  # no field element (>= p): what lies between the parts of two proofs


@pytest.mark.parametrize("shape", FF.SHAPES, ids=[s.name for s in FF.SHAPES])
def test_forged_proofs_get_the_oracles_code(ctx, mp2, shape):
    """every case of the shape between two honest proofs, in one call: as host words, and with the four parts of each proof in
    device buffers of their own at stride part_words + 3"""
    ckt, ofp = FF.circuit(shape), FF.params(shape)
    honest = FF.honest(shape)
    cat = FF.catalogue(shape)
    n = len(cat)
    rows = [honest] + [(f.caps, f.openings, f.proof) for f in cat] + [honest]
    caps, openings, proofs = (np.stack([r[i] for r in rows]) for i in range(3))
    ph = np.tile(np.asarray(ckt.pi_hash, dtype=np.uint64), (n + 2, 1))
    want = [0] + [int(C.verify(ckt, ofp, FF.digest(), ckt.pi_hash, f.caps, f.openings, f.proof)) for f in cat] + [0]
    predicted = [0] + [FF.status(f.fails) for f in cat] + [0]
    assert want == predicted, "the oracle's verifier and the prediction disagree (test_forged_fri_cases.py shows where)"

    fp = to_mp2(mp2, ofp)
    cv = FW.CircuitVerifier(ctx, ckt, n + 2, fp=fp, constants_sigmas_cap=honest[0][0], circuit_digest=FF.digest())
    words = cv.pack(caps, openings, proofs, ph)
    got = cv.verify_words(words).tolist()
    chal = cv.challenges(n + 2)
    # the same batch from four device buffers, each proof's part followed by three words that are no field elements
    offs = np.cumsum([0] + cv.v.part_words)
    assert offs[-1] == words.shape[1]
    bufs = []
    for k in range(4):
        part = np.full((n + 2, cv.v.part_words[k] + 3), SENTINEL, dtype=np.uint64)
        part[:, :-3] = words[:, offs[k]:offs[k + 1]]
        bufs.append(ctx.to_device(part))
    got_dev = cv.v.verify_dev(bufs, [w + 3 for w in cv.v.part_words], n + 2).tolist()
    for b in bufs:
        b.free()
    cv.free()

    tally = FF.tally(shape)
    tally["device"] = {c: got[1:-1].count(c) for c in sorted(set(got[1:-1]))}
    print("forged", shape.name, "layers", FF.layers(ofp), tally)
    bad = [(FF.label(f), got[1 + i], want[1 + i], f.fails[:1]) for i, f in enumerate(cat) if got[1 + i] != want[1 + i]]
    assert not bad, f"(plan, delta, bump), device, oracle, predicted triple: {bad[:10]}"
    assert got[0] == 0 and got[-1] == 0, "an honest proof beside the forged ones is rejected"
    assert all(got[1 + i] == 0 for i, f in enumerate(cat) if not f.fails), "an accepted forgery (no query reads what was changed) is rejected"
    bad = [(FF.label(cat[i - 1]) if 0 < i <= n else "honest", got_dev[i], got[i]) for i in range(n + 2) if got_dev[i] != got[i]]
    assert not bad, f"device buffers against host words: (case, verify_dev, verify) {bad[:10]}"
    # the indices the device drew are the ones the prediction was made from
    for i, r in enumerate(rows):
        idx = cat[i - 1].indices if 0 < i <= n else FF.query_indices(shape, *r)
        assert chal[i][-ofp.num_queries:].tolist() == idx, ("honest" if not 0 < i <= n else FF.label(cat[i - 1]))
