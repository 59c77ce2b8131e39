"""FRI parameter sets away from standard_recursion_config (rate 3, cap 4, ConstantArityBits(4, 5), four oracles), shared by the
CPU-only test of the list (test_fri_param_cases.py) and the device tests (test_gpu_fri_parameters.py): the PCS cases, the circuit
cases, the oracle's proof of each (made once per process and shared; treat the arrays as read-only) and the catalogue of single-word
mutations of a proof. A helper module: nothing here touches the device."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

import circuits as C
import oracle as O

WS = (5, 9, 4, 3)

# kw: keywords of O.standard_params; layers: arity_bits set by hand after it (None: what ConstantArityBits gives); batched: also
# proved three at a time by the device tests
PcsCase = namedtuple("PcsCase", "name log_n ws variant kw layers batched")


def _pcs(name, log_n, ws=WS, variants=(0,), layers=None, batched=False, **kw):
    kw.setdefault("pow_bits", 4)
    kw.setdefault("num_queries", 3)
    return [PcsCase(f"{name}-v{v}", log_n, tuple(ws), v, tuple(sorted(kw.items())), layers, batched) for v in variants]


PCS_CASES = (
    [c for rb in (1, 2, 4, 5, 6) for c in _pcs(f"rate{rb}", 7, rate_bits=rb)]
    # the tree tops take another kernel under Poseidon2 (variant 0): caps and arities under both hashers
    + [c for ch in (0, 1, 2, 7, 10) for c in _pcs(f"cap{ch}", 7, variants=(0, 1), cap_height=ch, batched=ch == 0)]
    + [c for a in (1, 2, 3) for c in _pcs(f"arity{a}", 9, variants=(0, 1), arity=a)]
    + [c for f in (0, 2, 7) for c in _pcs(f"final{f}", 9, final_poly_bits=f)]
    + _pcs("eight_layers", 9, arity=1, final_poly_bits=1, cap_height=1, batched=True)
    + _pcs("mixed", 10, cap_height=2, layers=(4, 3, 2, 1), batched=True)
    + _pcs("one_query_no_pow", 7, pow_bits=0, num_queries=1)
    + _pcs("queries64", 7, num_queries=64)
    + _pcs("queries0", 7, num_queries=0)
    + _pcs("one_oracle", 6, ws=(3,), zs_oracle=0, zs_count=0)
    + _pcs("eight_oracles", 6, ws=(3, 2, 4, 2, 1, 5, 2, 9), batched=True)
    + _pcs("tiny1", 1, rate_bits=1, cap_height=0)
    + _pcs("tiny2", 2, cap_height=5)
    + _pcs("two_pass14", 14, ws=(3, 4, 2, 2), batched=True)  # batched: the two-pass transforms over batch * w polynomials
    + _pcs("two_pass14_rate1", 14, ws=(3, 4, 2, 2), rate_bits=1, arity=3, cap_height=0)
    + _pcs("two_pass16_rate1", 16, ws=(2, 2, 2, 1), rate_bits=1, num_queries=2)
)

# kw: keywords of C.oracle_params (O.standard_params' names); rate_bits stays 3: the quotient's degree factor is 8
CircuitCase = namedtuple("CircuitCase", "name log_n kinds kw")
CIRCUIT_CASES = [
    CircuitCase("all6_arity2", 6, "ALL_KINDS", (("arity", 2), ("cap_height", 1), ("final_poly_bits", 2), ("num_queries", 5), ("pow_bits", 3))),
    CircuitCase("all6_arity1", 6, "ALL_KINDS", (("arity", 1), ("cap_height", 0), ("final_poly_bits", 3), ("num_queries", 1), ("pow_bits", 0))),
    CircuitCase("all7_arity3", 7, "ALL_KINDS", (("arity", 3), ("cap_height", 6), ("final_poly_bits", 1), ("num_queries", 40), ("pow_bits", 5))),
    CircuitCase("all5_cap_is_tree", 5, "ALL_KINDS", (("cap_height", 8), ("num_queries", 2), ("pow_bits", 2))),
    CircuitCase("lookup7_arity2", 7, "LOOKUP", (("arity", 2), ("cap_height", 2), ("final_poly_bits", 4), ("num_queries", 7), ("pow_bits", 3))),
]


def device_kw(kw):
    """the keywords under mp2.standard_recursion_params' names (`arity` is `arity_bits` there)"""
    return {("arity_bits" if k == "arity" else k): v for k, v in dict(kw).items()}


def pcs_params(case):
    fp = O.standard_params(case.log_n, case.ws, variant=case.variant, **dict(case.kw))
    if case.layers is not None:
        fp.n_layers = len(case.layers)
        for i in range(8):
            fp.arity_bits[i] = case.layers[i] if i < len(case.layers) else 0
    return fp


def pcs_inputs(case, seed=0xC0FFEE01):
    """(values per oracle [w][n], circuit digest, public-inputs hash)"""
    n = 1 << case.log_n
    return [O.rand_field((w, n), seed + i) for i, w in enumerate(case.ws)], O.rand_field(4, seed ^ 1), O.rand_field(4, seed ^ 2)


@functools.lru_cache(maxsize=None)
def pcs_oracle(case):
    """(params, values, digest, pi hash, caps, openings, proof) with the oracle's proof, made once"""
    fp = pcs_params(case)
    vals, cd, ph = pcs_inputs(case)
    return (fp, vals, cd, ph) + tuple(O.pcs_prove(fp, vals, cd, ph))


def n_siblings(fp):
    """Merkle path lengths of one query round: the initial trees', then each layer's"""
    lg = fp.log_n + fp.rate_bits
    out = [lg - fp.cap_height]
    for i in range(fp.n_layers):
        lg -= fp.arity_bits[i]
        out.append(lg - fp.cap_height)
    return out


def proof_sizes(fp):
    """(FRI proof words, openings) by the oracle's own size functions"""
    return int(O.lib().orc_fri_proof_words(ctypes.byref(fp))), int(O.lib().orc_n_openings(ctypes.byref(fp)))


_built = {}


def circuit(log_n, kinds_name, seed=3):
    key = (log_n, kinds_name, seed)
    if key not in _built:
        if kinds_name == "LOOKUP":
            _built[key] = C.build(log_n, C.ALL_KINDS + C.LOOKUP_KINDS, seed, luts=[(t, 100) for t in C.bits_lookup_tables()])
        else:
            _built[key] = C.build(log_n, getattr(C, kinds_name), seed)
    return _built[key]


def bump(a, idx):
    """v -> v + 1 mod p at flat index idx of array a (in place)"""
    flat = a.reshape(-1)
    flat[idx] = np.uint64((int(flat[idx]) + 1) % O.P)


def catalogue(fp, n_openings, proof_words, cap_stride=5):
    """[(part, flat index)]: every 5th word of the caps after cap 0 (cap 0 is the verifier's own and is bound through the circuit
    digest only), every 7th opening (alternating limb), every 97th FRI word and the last three (final polynomial tail, PoW witness)"""
    capw = 4 << fp.cap_height
    out = [("caps", o * capw + j) for o in range(1, fp.n_oracles) for j in range(0, capw, cap_stride)]
    out += [("openings", 2 * i + (i & 1)) for i in range(0, n_openings, 7)]
    out += [("fri", i) for i in sorted(set(range(0, proof_words, 97)) | {proof_words - 3, proof_words - 2, proof_words - 1})]
    return out


def mutated(caps, openings, proof, part, idx):
    """copies of the three arrays with the catalogue entry applied"""
    arrays = {"caps": caps.copy(), "openings": openings.copy(), "fri": proof.copy()}
    bump(arrays[part], idx)
    return arrays["caps"], arrays["openings"], arrays["fri"]


def constant_arity_bits(d, r, c, a, f):
    """plonky2 fri/reduction_strategies.rs ConstantArityBits(a, f) for degree 2^d, rate r, cap height c; None where its assert fires"""
    out = []
    while d > f and d + r - a >= c:
        if d < a:
            return None
        out.append(a)
        d -= a
    return out


def reduction_grid():
    """(log_n, rate_bits, cap_height, arity_bits, final_poly_bits) over everything params_check takes: 57 600 points"""
    return [(n, r, c, a, f) for n in range(1, 21) for r in range(1, 7) for c in range(0, n + r + 1) for a in range(1, 5) for f in range(0, 8)]
