"""The prover, the LDE, the commitment and the verifier away from standard_recursion_config: other rates, caps from 0 to the
whole tree, arities 1..4 (mixed too), 0 and 8 layers, 1 and 8 oracles, 0 / 1 / 64 queries, transforms at every logK and coset
shifts other than the multiplicative generator. Everything is compared bit for bit with the CPU oracle at the parameters of
fri_param_cases.py (which test_fri_param_cases.py shows the oracle sound at), never with the device itself."""
import ctypes
import importlib

import numpy as np
import pytest

import circuits as C
import fri_param_cases as FC
import oracle as O
from test_gpu_fri import to_mp2
from test_gpu_ntt_merkle import _At
from test_gpu_verifier import oracle_status, prove_batch

pytestmark = pytest.mark.gpu
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
P = O.P


def device_params(mp2, ofp):
    """the oracle's struct carried across word for word, and the library's sizes of it against the oracle's"""
    fp = to_mp2(mp2, ofp)
    assert (fp.proof_words, fp.n_openings) == FC.proof_sizes(ofp)
    return fp


# ---- PCS prover ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FC.PCS_CASES, ids=[c.name for c in FC.PCS_CASES])
def test_pcs_prove_matches_oracle(ctx, mp2, case):
    ofp, vals, cd, ph, ocaps, oopen, oproof = FC.pcs_oracle(case)
    fp = device_params(mp2, ofp)
    caps, openings, proof = mp2.pcs_prove(ctx, fp, vals, cd, ph)
    assert np.array_equal(caps, ocaps)
    assert np.array_equal(openings, oopen)
    diff = np.flatnonzero(proof != oproof)
    assert diff.size == 0, f"{diff.size} of {proof.size} FRI words differ, the first at {diff[:8].tolist()}"
    assert O.pcs_verify(ofp, cd, ph, caps, openings, proof) == 0


BATCHED = [c for c in FC.PCS_CASES if c.batched]


@pytest.mark.parametrize("case", BATCHED, ids=[c.name for c in BATCHED])
def test_batched_prover_matches_oracle(ctx, mp2, case):
    """three proofs per call: the batch strides of the layer buffers, the caps and the query kernel; proof 0 has the witness of
    the single-proof case"""
    B = 3
    ofp, vals, cd, _, _, _, _ = FC.pcs_oracle(case)
    fp = device_params(mp2, ofp)
    n = 1 << case.log_n
    per = [vals[1:]] + [[O.rand_field((w, n), 1000 * b + i) for i, w in enumerate(case.ws[1:])] for b in range(1, B)]
    ph = O.rand_field((B, 4), 4)
    pr = mp2.BatchedProver(ctx, fp, B)
    pr.set_preprocessed(ctx.to_device(vals[0]))
    d_vals = [ctx.to_device(np.stack([per[b][i] for b in range(B)])) for i in range(len(case.ws) - 1)]
    pr.prove(d_vals, ctx.to_device(cd), ctx.to_device(ph))
    caps, openings, proofs = pr.results()
    for b in range(B):
        oc, oo, op = O.pcs_prove(ofp, [vals[0]] + per[b], cd, ph[b])
        assert np.array_equal(caps[b], oc) and np.array_equal(openings[b], oo), b
        assert np.array_equal(proofs[b], op), (b, np.flatnonzero(proofs[b] != op)[:8].tolist())
        assert O.pcs_verify(ofp, cd, ph[b], caps[b], openings[b], proofs[b]) == 0
    assert len({proofs[b].tobytes() for b in range(B)}) == B
    pr.free()


# ---- circuits: prover and verifier -----------------------------------------------------------------
@pytest.mark.parametrize("case", FC.CIRCUIT_CASES, ids=[c.name for c in FC.CIRCUIT_CASES])
def test_circuit_proofs_verify_and_mutations_are_rejected_code_for_code(ctx, mp2, case):
    """four device proofs of the circuit: accepted by the device verifier where they lie and as host words, and by the oracle;
    proof 0 equals the oracle's proof of the same witness; then the case's mutation catalogue, the device's status against the
    oracle's code for code (test_gpu_verifier.test_rejects_code_for_code's method)"""
    ckt, B = FC.circuit(case.log_n, case.kinds), 4
    cp, d_ph, ph, caps, openings, proofs = prove_batch(ctx, ckt, B, **FC.device_kw(case.kw))
    ofp, dig = C.oracle_params(ckt, **dict(case.kw)), cp.circuit_digest
    assert bytes(cp.fp) == bytes(ofp), "the two standard-parameter functions disagree"
    assert (cp.fp.proof_words, cp.fp.n_openings) == FC.proof_sizes(ofp)
    cv = cp.verifier()
    st_dev = cv.verify_prover_outputs(cp, B, d_ph).tolist()
    st_host = cv.verify(caps, openings, proofs, ph).tolist()
    want = [oracle_status(ckt, ofp, dig, ph[b], caps[b], openings[b], proofs[b]) for b in range(B)]
    print("accept", case.name, st_dev, st_host, want)
    assert want == [0] * B and st_dev == [0] * B and st_host == [0] * B
    assert len({proofs[b].tobytes() for b in range(B)}) == B
    cv.free()
    w0 = FW.witness_of(ckt, 0x5EED, 0)
    oc, oo, op, _ = C.prove_witness(ckt, ofp, dig, w0, ckt.pi_hash)
    assert np.array_equal(caps[0], oc) and np.array_equal(openings[0], oo) and np.array_equal(proofs[0], op)

    cat = FC.catalogue(ofp, openings.shape[1], proofs.shape[1])
    n = len(cat)
    cs, os_, ps, hs = np.tile(caps[0], (n, 1, 1)), np.tile(openings[0], (n, 1, 1)), np.tile(proofs[0], (n, 1)), np.tile(ph[0], (n, 1))
    for i, (part, idx) in enumerate(cat):
        FC.bump({"caps": cs, "openings": os_, "fri": ps}[part][i], idx)
    cv = cp.verifier(capacity=n)
    got = cv.verify(cs, os_, ps, hs).tolist()
    cv.free()
    want = [oracle_status(ckt, ofp, dig, hs[i], cs[i], os_[i], ps[i]) for i in range(n)]
    tally = {w: want.count(w) for w in sorted(set(want))}
    print("reject", case.name, n, "cases; oracle tally", tally)
    bad = [(cat[i], got[i], want[i]) for i in range(n) if got[i] != want[i]]
    assert not bad, f"(entry, device, oracle) {bad[:10]}"
    assert all(w != 0 for w in want), "the oracle accepts a mutated proof"
    cp.free()


# ---- LDE ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,w", [(3, 2), (6, 5), (12, 3), (13, 3), (14, 2)])
@pytest.mark.parametrize("rb", [1, 2, 4, 5, 6])
def test_lde_leaves_every_rate(ctx, rb, log_n, w):
    """logK other than 3 on both sides of the single-pass / two-pass boundary (2^12 | 2^13)"""
    c = O.rand_field((w, 1 << log_n), 31 + log_n + 100 * rb)
    assert np.array_equal(ctx.lde_leaves(c, rb), O.lde_leaves(c, rb))


def test_lde_two_pass_without_the_full_table(ctx):
    """2^18 coefficients at rate 6: 2^24 outputs, the smallest shape whose pre-scale is the pre_lo * pre_hi pair (K << log_n > 2^23)"""
    c = O.rand_field((1, 1 << 18), 0x1DE)
    got = ctx.lde_leaves(c, 6)
    want = O.lde_leaves(c, 6)
    assert got.shape == (1 << 24, 1) and np.array_equal(got, want)


@pytest.mark.parametrize("log_n,batch", [(6, 7), (13, 3)])
@pytest.mark.parametrize("rb", [1, 6])
def test_lde_stays_inside_its_buffers(ctx, rb, log_n, batch):
    """the LDE between guard bands of a sentinel pattern, a ragged batch: the bands come back untouched, the coefficients are
    not written, and what lies between is the oracle's LDE"""
    n, guard = 1 << log_n, 1 << 12  # words
    sentinel = np.uint64(0xDEADBEEFCAFEF00D)
    a = O.rand_field((batch, n), 5200 + log_n + rb)
    d_c = ctx.to_device(np.full(batch * n + 2 * guard, sentinel, dtype=np.uint64))
    d_v = ctx.to_device(np.full((batch * n << rb) + 2 * guard, sentinel, dtype=np.uint64))
    d_c.upload_at(a.ravel(), guard * 8)
    ctx.lde_dev(_At(d_c, guard * 8), log_n, batch, rb, _At(d_v, guard * 8))
    got = d_v.download(((batch * n << rb) + 2 * guard,))
    back = d_c.download((batch * n + 2 * guard,))
    d_c.free(); d_v.free()
    assert (got[:guard] == sentinel).all() and (got[-guard:] == sentinel).all()
    assert (back[:guard] == sentinel).all() and (back[-guard:] == sentinel).all() and np.array_equal(back[guard:-guard], a.ravel())
    assert np.array_equal(got[guard:-guard].reshape(batch, n << rb).T, O.lde_leaves(a, rb))


# ---- commitment ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,w", [(4, 3), (10, 9)])
@pytest.mark.parametrize("rb", [0, 1, 2, 4, 6])
def test_commit_every_rate_and_cap(ctx, mp2, rb, log_n, w):
    n, lg = 1 << log_n, log_n + rb
    N = n << rb
    vals = O.rand_field((w, n), 0xC0FFEE01 + log_n * 100 + w + rb)
    coeffs = O.fft(vals, inverse=True)
    leaves = O.lde_leaves(coeffs, rb)
    for cap_h in (0, 1, lg):
        for variant in (0, 1):
            b = mp2.PolynomialBatch.from_values(ctx, vals, rb, cap_h, variant)
            assert np.array_equal(b.coeffs, coeffs)
            levels = O.merkle_build(leaves, cap_h, variant)
            cap = O.merkle_cap(levels, cap_h)
            assert np.array_equal(b.cap, cap), (cap_h, variant)
            idx = [0, 1, N - 1, N // 3]
            got_leaves, sib = b.open(idx)
            assert sib.shape == (4, lg - cap_h, 4)  # a cap as tall as the tree: paths of depth 0
            for k, i in enumerate(idx):
                assert np.array_equal(got_leaves[k], leaves[i])
                assert np.array_equal(sib[k], O.merkle_prove(levels, lg, cap_h, i))
                assert O.merkle_verify(got_leaves[k], i, sib[k], cap, variant)
            b.free()


# ---- coset shifts ----------------------------------------------------------------------------------------
ROOT_2_32 = 7277203076849721926  # the 2^32-th root of unity
SHIFTS = [1, 2, P - 1, ROOT_2_32, 0x9E3779B97F4A7C15 % P]


@pytest.mark.parametrize("log_n", [3, 10, 13, 14, 16])
def test_ntt_coset_shifts(ctx, log_n):
    a = O.rand_field((2, 1 << log_n), 4100 + log_n)
    for s in SHIFTS:
        assert np.array_equal(ctx.ntt(a, coset_shift=s), O.fft(a, coset_shift=s)), s
        assert np.array_equal(ctx.ntt(a, inverse=True, coset_shift=s), O.fft(a, inverse=True, coset_shift=s)), s


def test_ntt_coset_table_cache_keeps_shifts_apart(ctx):
    """the tables are cached under a hash of the shift: s1, s2, s1 again at one size, each against the oracle"""
    a = O.rand_field((1, 1 << 13), 4200)
    s1, s2 = SHIFTS[4], SHIFTS[3]
    for s in (s1, s2, s1, O.MULT_GEN, s2):
        assert np.array_equal(ctx.ntt(a, coset_shift=s), O.fft(a, coset_shift=s)), s


# ---- host checks: the layer-count rule and the refusals (the loaded library, no launch) ---------------------
def test_reduction_arity_bits_is_plonky2s_rule(mp2):
    """mp2g_reduction_arity_bits against ConstantArityBits over everything params_check takes: equal where plonky2 neither
    asserts nor gives more than 8 layers; where its assert fires, the layers pushed before it ("stop instead of wrapping");
    never more than 8"""
    f = mp2.load().mp2g_reduction_arity_bits
    out = (ctypes.c_uint32 * 9)()
    agree = asserts = over = 0
    for d, r, c, a, fin in FC.reduction_grid():
        out[8] = 0xDEAD
        n = f(d, r, c, a, fin, out)
        assert n <= 8 and out[8] == 0xDEAD and all(out[i] == a for i in range(n)), (d, r, c, a, fin)
        want = FC.constant_arity_bits(d, r, c, a, fin)
        if want is None:
            asserts += 1
            dd, k = d, 0
            while dd > fin and dd + r - a >= c and dd >= a:
                dd, k = dd - a, k + 1
            assert n == min(k, 8), (d, r, c, a, fin)
        elif len(want) > 8:
            over += 1
            assert n == 8, (d, r, c, a, fin)
        else:
            agree += 1
            assert n == len(want), (d, r, c, a, fin)
    assert (agree, asserts, over) == (51520, 1124, 4956)


def test_params_check_refuses_what_it_documents(ctx, mp2):
    def refused(match, **change):
        fp = mp2.standard_recursion_params(7, FC.WS, pow_bits=4, num_queries=3)
        assert fp.n_layers == 1 and fp.arity_bits[0] == 4
        for k, v in change.items():
            if k == "arity_bits":
                for i, x in enumerate(v):
                    fp.arity_bits[i] = x
            else:
                setattr(fp, k, v)
        with pytest.raises(mp2.Mp2gError, match=match):
            mp2.BatchedProver(ctx, fp, 1)

    refused("rate_bits", rate_bits=7)
    refused("arity_bits in 1..4", arity_bits=[5])
    refused("cap_height", cap_height=11)
    refused("layer smaller than cap", cap_height=7)  # 2^10 / 2^4 = 2^6 leaves under a cap of 2^7
    refused("n_layers", n_layers=9)
    refused("num_queries", num_queries=65)
    refused("arity exceeds degree", n_layers=2, arity_bits=[4, 4])  # plonky2's own assert: degree 2^7 after one layer is 2^3
    mp2.BatchedProver(ctx, mp2.standard_recursion_params(7, FC.WS, pow_bits=4, num_queries=3), 1).free()  # the unchanged one is taken
