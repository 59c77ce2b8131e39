"""Oracle-side companions of the synthetic circuits (mapreduce-plonky2_amd/circuits.py): the CPU oracle's
prove(), PLONK identity check and constraint evaluation for a built circuit. Test infrastructure.
"""
import ctypes
import importlib

import numpy as np

import oracle as O

_pc = importlib.import_module("mapreduce-plonky2_amd.circuits")
globals().update({k: v for k, v in vars(_pc).items() if not k.startswith("__")})


def eval_on_points(ckt, consts, wires):
    """C_j at the given points: consts [num_constants][npts], wires [135][npts] -> [maxc][npts]"""
    consts, wires = O.arr(consts), O.arr(wires)
    npts = wires.shape[1]
    maxc = max(gate_num_constraints(g) for g in ckt.gates)
    out = np.zeros((maxc, npts), dtype=np.uint64)
    ph = O.arr(ckt.pi_hash)
    O.lib().orc_gates_eval_points(ckt.gate_array, len(ckt.gates), ckt.num_selectors, consts.shape[0], O.p(consts), wires.shape[0],
                                  O.p(wires), O.sz(npts), O.p(ph), O.p(out))
    return out


class OrcLookup(ctypes.Structure):
    _fields_ = [("last_lu_row", ctypes.c_uint32), ("last_lut_row", ctypes.c_uint32), ("first_lut_row", ctypes.c_uint32),
                ("table_len", ctypes.c_uint32), ("table", ctypes.c_void_p)]


class OrcCircuit(ctypes.Structure):
    """orc_circuit (oracle/fri.c): permutation geometry, gate table, lookup tables"""
    _fields_ = [("num_routed", ctypes.c_uint32), ("degree", ctypes.c_uint32), ("gates", ctypes.c_void_p), ("n_gates", ctypes.c_uint32),
                ("num_selectors", ctypes.c_uint32), ("luts", ctypes.c_void_p), ("n_luts", ctypes.c_uint32)]


def orc_circuit(ckt):
    """(OrcCircuit, keep-alive list) of a built circuit"""
    luts = ckt.luts or []  # bench.py's CPU farm hands over a stand-in with luts = None
    tabs = [np.ascontiguousarray(t["table"], dtype=np.uint16) for t in luts]
    arr = (OrcLookup * max(1, len(luts)))()
    for i, (t, tab) in enumerate(zip(luts, tabs)):
        arr[i] = OrcLookup(t["last_lu_row"], t["last_lut_row"], t["first_lut_row"], tab.shape[0], tab.ctypes.data)
    ck = OrcCircuit(NUM_ROUTED, 8, ctypes.cast(ckt.gate_array, ctypes.c_void_p), len(ckt.gates), ckt.num_selectors,
                    ctypes.cast(arr, ctypes.c_void_p) if luts else None, len(luts))
    return ck, (arr, tabs)


def oracle_params(ckt, variant=0, **kw):
    """standard_recursion_config FRI / oracle shape of a built circuit (with the lookup polynomials, if any)"""
    return O.standard_params(ckt.log_n, ckt.oracle_widths(), variant=variant, num_lookup_polys=ckt.num_lookup_polys, **kw)


def prove_witness(ckt, fp, circuit_digest, wires, pi_hash):
    """oracle prove() of the circuit for the given witness and public-inputs hash; returns (caps, openings, proof, chal)
    with chal = betas[2], gammas[2], alphas[2], zeta[2] (+ the 8 lookup challenges)"""
    n = 1 << ckt.log_n
    vals = [O.arr(ckt.pre), O.arr(wires), np.zeros((fp.oracle_w[2], n), dtype=np.uint64), np.zeros((fp.oracle_w[3], n), dtype=np.uint64)]
    ptrs = (ctypes.c_void_p * 4)(*[v.ctypes.data for v in vals])
    capw = 4 << fp.cap_height
    caps = np.zeros((fp.n_oracles, capw), dtype=np.uint64)
    openings = np.zeros((O.lib().orc_n_openings(ctypes.byref(fp)), 2), dtype=np.uint64)
    proof = np.zeros(O.lib().orc_fri_proof_words(ctypes.byref(fp)), dtype=np.uint64)
    cd, ph, chal = O.arr(circuit_digest), O.arr(pi_hash), np.zeros(16, dtype=np.uint64)
    ck, keep = orc_circuit(ckt)
    O.lib().orc_prove_circuit(ctypes.byref(fp), ptrs, O.p(cd), O.p(ph), ctypes.byref(ck), O.p(chal), O.p(caps), O.p(openings), O.p(proof))
    return caps, openings, proof, chal


def prove(ckt, fp, circuit_digest):
    """oracle prove() of the circuit with its own witness; returns (caps, openings, proof, chal)"""
    return prove_witness(ckt, fp, circuit_digest, ckt.wires, ckt.pi_hash)


def verify(ckt, fp, circuit_digest, pi_hash, caps, openings, proof):
    """oracle verify(): challenges from the transcript, PLONK identity with the lookup and gate terms, FRI. 0 = accept."""
    cd, ph = O.arr(circuit_digest), O.arr(pi_hash)
    caps, openings, proof = O.arr(caps), O.arr(openings), O.arr(proof)
    ck, keep = orc_circuit(ckt)
    return O.lib().orc_verify_circuit(ctypes.byref(fp), O.p(cd), O.p(ph), ctypes.byref(ck), O.p(caps), O.p(openings), O.p(proof))


def identity_check(ckt, fp, openings, chal):
    class G2(ctypes.Structure):
        _fields_ = [("c", ctypes.c_uint64 * 2)]
    z = G2()
    z.c[0], z.c[1] = int(chal[6]), int(chal[7])
    o, b, g, a, ph = O.arr(openings), O.arr(chal[0:2]), O.arr(chal[2:4]), O.arr(chal[4:6]), O.arr(ckt.pi_hash)
    d = O.arr(chal[8:16]) if len(chal) >= 16 else np.zeros(8, dtype=np.uint64)
    ck, keep = orc_circuit(ckt)
    return O.lib().orc_identity_check_circuit(ctypes.byref(fp), ctypes.byref(ck), O.p(o), z, O.p(b), O.p(g), O.p(a), O.p(d), O.p(ph))
