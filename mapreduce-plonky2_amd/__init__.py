"""Host-side (Python) mirror of the prover interface of Lagrange-Labs/mapreduce-plonky2's hot
path, over the C ABI of libmp2gpu (include/mp2g.h).

The reference is Rust: the Python layer here is only the test / bench harness. The names follow
plonky2's as used behind `prove()` (recursion-framework/src/circuit_builder.rs:308):
PolynomialBatch.from_values / from_coeffs, MerkleTree.new / prove, Hasher.hash_no_pad.
There is no CPU fallback: loading fails loudly when the HIP library is missing, and
Context() fails when no GPU is visible.
"""
import ctypes
import time
import os
import weakref

import numpy as np

from ._abi import prototypes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MP2G_LIB", os.path.join(_HERE, "libmp2gpu.so"))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mp2g.h")

P = 0xFFFFFFFF00000001
MULT_GEN = 14293326489335486720
POSEIDON2, POSEIDON = 0, 1

_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_lib = None


class Mp2gError(RuntimeError):
    pass


def load():
    """dlopen libmp2gpu.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Mp2gError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`; "
                            "there is no CPU fallback for the product path")
        if not os.path.exists(HEADER_PATH):
            raise Mp2gError(f"{HEADER_PATH} is missing: the prototype of every library call is read from it")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in prototypes(HEADER_PATH).items():
            if not hasattr(lib, name):
                raise Mp2gError(f"{LIB_PATH} does not export {name}, which include/mp2g.h declares")
            f = getattr(lib, name)
            f.restype, f.argtypes = restype, argtypes
        _lib = lib
    return _lib


def _ck(rc):
    if rc != 0:
        raise Mp2gError(load().mp2g_last_error().decode())


def _arr(a, dtype=np.uint64):
    return np.ascontiguousarray(a, dtype=dtype)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class DeviceBuffer:
    _as_parameter_ = property(lambda self: self.ptr)  # passed to a library call, a buffer is its device address

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        ptr = ctypes.c_void_p()
        _ck(load().mp2g_dev_alloc(ctx.h, nbytes, ctypes.byref(ptr)))
        self.ptr = ptr
        ctx._adopt(self)

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        _ck(load().mp2g_h2d(self.ctx.h, self, _p(a), a.nbytes))
        return self

    def upload_at(self, a, offset):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        _ck(load().mp2g_h2d(self.ctx.h, self.ptr.value + offset, _p(a), a.nbytes))
        return self

    def download(self, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _ck(load().mp2g_d2h(self.ctx.h, _p(out), self, out.nbytes))
        return out

    def free(self):
        if self.ptr and self.ctx.h:
            load().mp2g_dev_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One per GPU (mp2g_ctx)."""
    _as_parameter_ = property(lambda self: self.h)  # a library call takes a Context, or None where it needs no device

    def __init__(self, device=0):
        self.h = ctypes.c_void_p()
        self._children = weakref.WeakSet()
        _ck(load().mp2g_ctx_create(int(device), ctypes.byref(self.h)))

    def _adopt(self, obj):
        self._children.add(obj)
        return obj

    def close(self):
        """Free every handle that lives on this context, then the context itself (handles keep
        a raw pointer to their context, so they must never outlive it)."""
        if self.h:
            for obj in list(self._children):
                obj.free()
            load().mp2g_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def make_current(self):
        """select this context's device for the calling thread (HIP's current device is per thread; call at the start of a worker thread)"""
        _ck(load().mp2g_ctx_make_current(self.h))

    def mem_info(self):
        """(free, total) bytes of the context's device"""
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        _ck(load().mp2g_ctx_mem_info(self.h, ctypes.byref(free), ctypes.byref(total)))
        return int(free.value), int(total.value)

    def sync(self):
        _ck(load().mp2g_ctx_sync(self.h))

    def stream(self):
        return load().mp2g_ctx_stream(self.h)

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        return DeviceBuffer(self, a.nbytes).upload(a)

    def host_alloc(self, nbytes):
        """Pinned host buffer as a numpy uint8 view (freed with host_free)."""
        ptr = ctypes.c_void_p()
        _ck(load().mp2g_host_alloc(self.h, nbytes, ctypes.byref(ptr)))
        buf = (ctypes.c_uint8 * nbytes).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.uint8), ptr

    def host_free(self, ptr):
        _ck(load().mp2g_host_free(self.h, ptr))

    def h2d_async(self, d_dst, host_ptr, nbytes, dst_offset=0):
        _ck(load().mp2g_h2d_async(self.h, d_dst.ptr.value + dst_offset, host_ptr, nbytes))

    def d2d_2d(self, d_dst, dst_offset, dst_pitch, d_src, src_offset, src_pitch, width, rows):
        """stream-ordered strided device copy (all sizes in bytes): `rows` pieces of `width` bytes"""
        _ck(load().mp2g_d2d_2d(self.h, d_dst.ptr.value + dst_offset, dst_pitch, d_src.ptr.value + src_offset, src_pitch, width, rows))

    def d2h_raw(self, src_ptr, shape, dtype=np.uint64):
        """download from a raw device address"""
        out = np.empty(shape, dtype=dtype)
        _ck(load().mp2g_d2h(self.h, _p(out), int(src_ptr), out.nbytes))
        return out

    def d2d_raw(self, d_dst, dst_offset, src_ptr, nbytes):
        """stream-ordered device copy of nbytes from a raw device address into a DeviceBuffer"""
        _ck(load().mp2g_d2d_2d(self.h, d_dst.ptr.value + dst_offset, nbytes, int(src_ptr), nbytes, nbytes, 1))

    def wires_from_rows_dev(self, d_rows, d_wires, log_n, batch, num_wires=135):
        """[batch][n][num_wires] (the witness executor's row layout) -> [batch][num_wires][n] (the prover's), on the device"""
        _ck(load().mp2g_wires_from_rows_dev(self.h, d_rows.ptr, d_wires.ptr, log_n, num_wires, batch))

    def timer_start(self):
        _ck(load().mp2g_timer_start(self.h))

    def timer_stop(self):
        ms = ctypes.c_float()
        _ck(load().mp2g_timer_stop(self.h, ctypes.byref(ms)))
        return ms.value

    # ---- plonky2_field fft.rs ---------------------------------------------------------------
    def ntt(self, data, inverse=False, coset_shift=0, bitrev_out=False):
        a = _arr(data).copy()
        batch, n = (1, a.shape[0]) if a.ndim == 1 else a.shape
        log_n = int(n).bit_length() - 1
        assert 1 << log_n == n
        _ck(load().mp2g_ntt(self.h, _p(a), log_n, batch, int(inverse), coset_shift, int(bitrev_out)))
        return a

    def ntt_dev(self, d_in, d_out, log_n, batch, inverse=False, coset_shift=0, bitrev_out=False):
        _ck(load().mp2g_ntt_dev(self.h, d_in.ptr, d_out.ptr, log_n, batch, int(inverse), coset_shift, int(bitrev_out)))

    def lde_leaves(self, coeffs, rate_bits):
        c = _arr(coeffs)
        w, n = c.shape
        log_n = int(n).bit_length() - 1
        out = np.empty((n << rate_bits, w), dtype=np.uint64)
        _ck(load().mp2g_lde_leaves(self.h, _p(c), log_n, w, rate_bits, _p(out)))
        return out

    def lde_dev(self, d_coeffs, log_n, w, rate_bits, d_values):
        _ck(load().mp2g_lde_dev(self.h, d_coeffs.ptr, log_n, w, rate_bits, d_values.ptr))

    # ---- Hasher -------------------------------------------------------------------------------
    def hash_no_pad_batch(self, inputs, out_len=4, variant=POSEIDON2):
        a = _arr(inputs)
        count, in_len = a.shape
        out = np.empty((count, out_len), dtype=np.uint64)
        _ck(load().mp2g_hash_no_pad_batch(self.h, variant, _p(a), in_len, count, out_len, _p(out)))
        return out

    def hash_no_pad(self, values, variant=POSEIDON2):
        return self.hash_no_pad_batch(_arr(values).reshape(1, -1), 4, variant)[0]


class MerkleTree:
    """plonky2 hash/merkle_tree.rs MerkleTree."""

    def __init__(self, ctx, leaves, cap_height, variant=POSEIDON2):
        a = _arr(leaves)
        L, leaf_len = a.shape
        self.log_leaves = int(L).bit_length() - 1
        assert 1 << self.log_leaves == L
        self.ctx, self.cap_height, self.leaf_len = ctx, cap_height, leaf_len
        self.h = ctypes.c_void_p()
        _ck(load().mp2g_merkle_build(ctx.h, variant, _p(a), leaf_len, self.log_leaves, cap_height, ctypes.byref(self.h)))
        ctx._adopt(self)

    @property
    def cap(self):
        out = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        _ck(load().mp2g_merkle_cap(self.h, _p(out)))
        return out

    def prove(self, indices):
        idx = _arr(indices, np.uint32)
        depth = self.log_leaves - self.cap_height
        leaves = np.empty((len(idx), self.leaf_len), dtype=np.uint64)
        sib = np.empty((len(idx), depth, 4), dtype=np.uint64)
        _ck(load().mp2g_merkle_open(self.h, _p(idx), len(idx), _p(leaves), _p(sib)))
        return leaves, sib

    def free(self):
        if self.h and self.ctx.h:
            load().mp2g_merkle_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PolynomialBatch:
    """plonky2 fri/oracle.rs PolynomialBatch: coefficients + LDE Merkle tree."""

    def __init__(self, ctx, handle, log_n, w, rate_bits, cap_height):
        self.ctx, self.h = ctx, handle
        self.log_n, self.w, self.rate_bits, self.cap_height = log_n, w, rate_bits, cap_height
        ctx._adopt(self)

    @classmethod
    def from_values(cls, ctx, values, rate_bits=3, cap_height=4, variant=POSEIDON2):
        v = _arr(values)
        w, n = v.shape
        log_n = int(n).bit_length() - 1
        h = ctypes.c_void_p()
        _ck(load().mp2g_commit_from_values(ctx.h, variant, _p(v), log_n, w, rate_bits, cap_height, ctypes.byref(h)))
        return cls(ctx, h, log_n, w, rate_bits, cap_height)

    @classmethod
    def from_values_dev(cls, ctx, d_values, log_n, w, rate_bits=3, cap_height=4, variant=POSEIDON2):
        h = ctypes.c_void_p()
        _ck(load().mp2g_commit_from_values_dev(ctx.h, variant, d_values.ptr, log_n, w, rate_bits, cap_height, ctypes.byref(h)))
        return cls(ctx, h, log_n, w, rate_bits, cap_height)

    @classmethod
    def from_coeffs_dev(cls, ctx, d_coeffs, log_n, w, rate_bits=3, cap_height=4, variant=POSEIDON2):
        h = ctypes.c_void_p()
        _ck(load().mp2g_commit_from_coeffs_dev(ctx.h, variant, d_coeffs.ptr, log_n, w, rate_bits, cap_height, ctypes.byref(h)))
        return cls(ctx, h, log_n, w, rate_bits, cap_height)

    def recommit_from_values_dev(self, d_values):
        _ck(load().mp2g_recommit_from_values_dev(self.ctx.h, self.h, d_values.ptr))

    def rehash_dev(self, parts=3):
        """MerkleTree::new over the LDE values the batch holds: parts 1 = leaf sponges, 2 = tree levels, 3 = both"""
        _ck(load().mp2g_batch_rehash_dev(self.ctx.h, self.h, parts))

    @property
    def cap(self):
        out = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        _ck(load().mp2g_batch_cap(self.h, _p(out)))
        return out

    @property
    def coeffs(self):
        out = np.empty((self.w, 1 << self.log_n), dtype=np.uint64)
        _ck(load().mp2g_batch_coeffs(self.h, _p(out)))
        return out

    def eval_ext(self, point):
        """Evaluate every polynomial of the batch at an extension-field point (the openings)."""
        pt = _arr(point)
        out = np.empty((self.w, 2), dtype=np.uint64)
        _ck(load().mp2g_batch_eval_ext(self.h, _p(pt), _p(out)))
        return out

    def open(self, indices):
        idx = _arr(indices, np.uint32)
        depth = self.log_n + self.rate_bits - self.cap_height
        leaves = np.empty((len(idx), self.w), dtype=np.uint64)
        sib = np.empty((len(idx), depth, 4), dtype=np.uint64)
        _ck(load().mp2g_batch_open(self.h, _p(idx), len(idx), _p(leaves), _p(sib)))
        return leaves, sib

    def free(self):
        if self.h and self.ctx.h:
            load().mp2g_batch_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FriParams(ctypes.Structure):
    """mp2g_fri_params (include/mp2g.h)."""
    _fields_ = [("variant", ctypes.c_uint32), ("log_n", ctypes.c_uint32), ("rate_bits", ctypes.c_uint32),
                ("cap_height", ctypes.c_uint32), ("pow_bits", ctypes.c_uint32), ("num_queries", ctypes.c_uint32),
                ("n_layers", ctypes.c_uint32), ("arity_bits", ctypes.c_uint32 * 8), ("n_oracles", ctypes.c_uint32),
                ("oracle_w", ctypes.c_uint32 * 8), ("zs_oracle", ctypes.c_uint32), ("zs_count", ctypes.c_uint32),
                ("num_lookup_polys", ctypes.c_uint32)]

    @property
    def proof_words(self):
        return load().mp2g_fri_proof_words(ctypes.byref(self))

    @property
    def n_openings(self):
        return load().mp2g_fri_n_openings(ctypes.byref(self))

    @property
    def cap_words(self):
        return 4 << self.cap_height


def standard_recursion_params(log_n, oracle_w=(84, 135, 20, 16), variant=POSEIDON2, rate_bits=3, cap_height=4,
                              pow_bits=16, num_queries=28, zs_oracle=2, zs_count=2, arity_bits=4, final_poly_bits=5,
                              num_lookup_polys=0):
    """FRI parameters of standard_recursion_config (mp2-common/src/lib.rs:45-47) for 2^log_n rows:
    135 wires, 2 challenges (=> 20 Z/partial-product and 16 quotient-chunk polynomials),
    ConstantArityBits(4, 5). 84 = constants + 80 sigma polynomials of a typical circuit."""
    fp = FriParams()
    fp.variant, fp.log_n, fp.rate_bits, fp.cap_height = variant, log_n, rate_bits, cap_height
    fp.pow_bits, fp.num_queries = pow_bits, num_queries
    ab = (ctypes.c_uint32 * 8)()
    fp.n_layers = load().mp2g_reduction_arity_bits(log_n, rate_bits, cap_height, arity_bits, final_poly_bits, ab)
    fp.arity_bits = ab
    fp.n_oracles = len(oracle_w)
    for i, w in enumerate(oracle_w):
        fp.oracle_w[i] = w
    fp.zs_oracle, fp.zs_count, fp.num_lookup_polys = zs_oracle, zs_count, num_lookup_polys
    return fp


class Challenger:
    """plonky2 iop/challenger.rs Challenger; `count` transcripts in lockstep on the device."""

    def __init__(self, ctx, variant=POSEIDON2, count=1):
        self.ctx, self.count = ctx, count
        self.h = ctypes.c_void_p()
        _ck(load().mp2g_challenger_create(ctx.h, variant, count, ctypes.byref(self.h)))
        ctx._adopt(self)

    def observe_elements(self, elems):
        a = _arr(elems).reshape(self.count, -1)
        _ck(load().mp2g_challenger_observe(self.h, _p(a), a.shape[1]))

    def get_n_challenges(self, n):
        out = np.empty((self.count, n), dtype=np.uint64)
        _ck(load().mp2g_challenger_get(self.h, n, _p(out)))
        return out

    def free(self):
        if self.h and self.ctx.h:
            load().mp2g_challenger_free(self.h)
        self.h = None


def fri_fold(ctx, evals, arity_bits, beta, shift):
    a = _arr(evals)
    m = a.shape[0]
    log_m = int(m).bit_length() - 1
    out = np.empty((m >> arity_bits, 2), dtype=np.uint64)
    b = _arr(beta)
    _ck(load().mp2g_fri_fold(ctx.h, _p(a), log_m, arity_bits, _p(b), shift, _p(out)))
    return out


def fri_pow(ctx, state, pos, bits, variant=POSEIDON2):
    s = _arr(state)
    w = ctypes.c_uint64()
    _ck(load().mp2g_fri_pow(ctx.h, variant, _p(s), pos, bits, ctypes.byref(w)))
    return w.value


def pcs_prove(ctx, fp, values, circuit_digest, pi_hash):
    """Single proof, host arrays: the PCS skeleton of prove(). Returns (caps, openings, proof)."""
    vals = [_arr(v) for v in values]
    ptrs = (ctypes.c_void_p * len(vals))(*[v.ctypes.data for v in vals])
    caps = np.empty((fp.n_oracles, fp.cap_words), dtype=np.uint64)
    openings = np.empty((fp.n_openings, 2), dtype=np.uint64)
    proof = np.empty(fp.proof_words, dtype=np.uint64)
    cd, ph = _arr(circuit_digest), _arr(pi_hash)
    _ck(load().mp2g_pcs_prove(ctx.h, ctypes.byref(fp), ptrs, _p(cd), _p(ph), _p(caps), _p(openings), _p(proof)))
    return caps, openings, proof


class Gate(ctypes.Structure):
    """mp2g_gate: one entry of CommonCircuitData::gates with its selector group."""
    _fields_ = [("kind", ctypes.c_uint32), ("p0", ctypes.c_uint32), ("p1", ctypes.c_uint32), ("p2", ctypes.c_uint32),
                ("selector_index", ctypes.c_uint32), ("group_start", ctypes.c_uint32), ("group_end", ctypes.c_uint32)]

    @property
    def num_constraints(self):
        return load().mp2g_gate_num_constraints(ctypes.byref(self))

    @property
    def degree(self):
        return load().mp2g_gate_degree(ctypes.byref(self))


(GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC, GATE_BASE_SUM, GATE_ARITHMETIC_EXT, GATE_MUL_EXT, GATE_POSEIDON2,
 GATE_EXPONENTIATION, GATE_REDUCING, GATE_REDUCING_EXT, GATE_RANDOM_ACCESS, GATE_POSEIDON, GATE_POSEIDON_MDS,
 GATE_COSET_INTERPOLATION, GATE_U32_ARITHMETIC, GATE_U32_RANGE_CHECK, GATE_U32_SUBTRACTION, GATE_U32_ADD_MANY,
 GATE_COMPARISON, GATE_LOOKUP, GATE_LOOKUP_TABLE, GATE_U32_INTERLEAVE, GATE_UNINTERLEAVE_TO_B32, GATE_UNINTERLEAVE_TO_U32) = range(25)


class Lookup(ctypes.Structure):
    """mp2g_lookup: one lookup table and its rows (plonky2's LookupWire + the table of CommonCircuitData::luts)."""
    _fields_ = [("last_lu_row", ctypes.c_uint32), ("last_lut_row", ctypes.c_uint32), ("first_lut_row", ctypes.c_uint32),
                ("table_len", ctypes.c_uint32), ("table", ctypes.c_void_p)]


def lookup_array(luts):
    """(Lookup * n) from the builder's lookup descriptions (dicts with the row fields and a uint16 [len][2] table);
    the second value keeps the table arrays alive"""
    tabs = [np.ascontiguousarray(t["table"], dtype=np.uint16) for t in luts]
    arr = (Lookup * max(1, len(luts)))()
    for i, (t, tab) in enumerate(zip(luts, tabs)):
        arr[i] = Lookup(t["last_lu_row"], t["last_lut_row"], t["first_lut_row"], tab.shape[0], tab.ctypes.data)
    return arr, tabs


def gate_array(gates):
    """(Gate * n) from the builder's gates or from Gates (anything with the seven fields of mp2g_gate)"""
    return (Gate * max(1, len(gates)))(*[Gate(g.kind, g.p0, g.p1, g.p2, g.selector_index, g.group_start, g.group_end) for g in gates])


def eval_gate_constraints(ctx, gates, num_selectors, consts, wires, pi_hash):
    """Filtered gate constraints C_j at arbitrary points: consts [num_constants][npts], wires [w][npts]
    -> [max_j][npts]. All zero on H for a satisfied witness (plonky2's prove() panics otherwise)."""
    c, w, ph = _arr(consts), _arr(wires), _arr(pi_hash)
    arr = gate_array(gates)
    max_j = max(arr[i].num_constraints for i in range(len(gates)))
    out = np.zeros((max_j, w.shape[1]), dtype=np.uint64)
    _ck(load().mp2g_eval_gate_constraints(ctx.h, arr, len(gates), num_selectors, _p(c), c.shape[0], _p(w), w.shape[0],
                                          w.shape[1], _p(ph), _p(out)))
    return out


def eval_gate_constraints_lde(ctx, gates, num_selectors, consts, wires, alphas, pi_hash, num_lookup_selectors=0, out=None):
    """The gate term of the quotient, sum_j alpha^j C_j, by the launchers prove() runs on the LDE: consts [num_constants][N]
    (selectors, num_lookup_selectors unread rows, gate constants), wires [B][w][N], alphas [B][nc], pi_hash [B][4]
    -> [B][nc][N], N a power of two. Column p of the inputs is memory column p of the bit-reversed LDE; its result is at
    [b][a][bitrev(p)]. Words >= p are refused. out: an array to fill instead of a new one."""
    c, w, al, ph = _arr(consts), _arr(wires), _arr(alphas), _arr(pi_hash)
    B, N, nc = w.shape[0], w.shape[-1], al.shape[-1]
    if w.ndim != 3 or al.shape != (B, nc) or ph.shape != (B, 4) or c.ndim != 2 or c.shape[1] != N or N < 2 or N & (N - 1):
        raise ValueError("consts [.][N], wires [B][.][N], alphas [B][nc], pi_hash [B][4] with N = 2^k >= 2")
    if out is None:
        out = np.zeros((B, nc, N), dtype=np.uint64)
    if out.dtype != np.uint64 or not out.flags.c_contiguous or out.size < B * nc * N:
        raise ValueError("out: a contiguous uint64 array of at least B * nc * N words")
    _ck(load().mp2g_eval_gate_constraints_lde(ctx.h, gate_array(gates), len(gates), num_selectors, num_lookup_selectors, _p(c), c.shape[0],
                                              _p(w), w.shape[1], N.bit_length() - 1, B, _p(al), nc, _p(ph), _p(out)))
    return out


class BatchedProver:
    """mp2g_prover: `batch` same-shape proofs per call, device resident."""

    def __init__(self, ctx, fp, batch):
        self.ctx, self.fp, self.batch = ctx, fp, batch
        self.h = ctypes.c_void_p()
        _ck(load().mp2g_prover_create(ctx.h, ctypes.byref(fp), batch, ctypes.byref(self.h)))
        ctx._adopt(self)
        self.d_caps = ctx.alloc(batch * fp.n_oracles * fp.cap_words * 8)
        self.d_openings = ctx.alloc(batch * fp.n_openings * 2 * 8)
        self.d_proof = ctx.alloc(batch * fp.proof_words * 8)

    def set_preprocessed(self, d_values):
        _ck(load().mp2g_prover_set_preprocessed_dev(self.h, d_values.ptr))

    def enable_permutation(self, num_routed=80, degree=8):
        """Compute the Z / partial-product oracle on the device from the wires and the sigma
        polynomials (prove()'s permutation argument); d_values[1] may then be None."""
        _ck(load().mp2g_prover_enable_permutation(self.h, num_routed, degree))

    def enable_quotient(self):
        """Also compute the quotient chunks on the device: permutation terms, plus the gate constraints
        once set_gates() has given the gate table; d_values[2] may then be None."""
        _ck(load().mp2g_prover_enable_quotient(self.h))

    def set_gates(self, gates, num_selectors):
        """Gate table of the circuit (CommonCircuitData::gates + SelectorsInfo): the quotient then
        includes the gate constraint terms -- prove() of a circuit built from the supported gates."""
        _ck(load().mp2g_prover_set_gates(self.h, gate_array(gates), len(gates), num_selectors))

    def lookup_wires_dev(self, n_lookups, d_wires, batch):
        """prove()'s set_lookup_wires on the device, in place on d_wires [batch][wires_w][n] (needs set_lookups): n_lookups[t] =
        the looked-up slots of table t; the padding, the table rows and the multiplicities are written"""
        nl = np.ascontiguousarray(n_lookups, dtype=np.uint32)
        _ck(load().mp2g_prover_lookup_wires_dev(self.h, _p(nl), d_wires.ptr, int(batch)))

    def set_lookups(self, luts):
        """Lookup tables of the circuit (CommonCircuitData::luts + ProverOnlyCircuitData::lookup_rows): prove() then
        draws the lookup challenges, computes the RE / Sum / LDC polynomials into the Z oracle and adds the lookup
        terms to the quotient. Needs set_gates() with the lookup gates in the table."""
        arr, keep = lookup_array(luts)
        _ck(load().mp2g_prover_set_lookups(self.h, arr, len(luts)))

    def bind_public_inputs(self, row):
        """PublicInputGate's generator on the device: wires 0..3 of `row` of every proof's wire matrix are
        overwritten (in place) with that proof's public-inputs hash before the commitment."""
        _ck(load().mp2g_prover_bind_public_inputs(self.h, -1 if row is None else int(row)))

    def enable_witness_check(self, on=True):
        """Check gate and copy constraints of every witness on the device (plonky2 panics on a bad one)."""
        _ck(load().mp2g_prover_enable_witness_check(self.h, int(on)))

    def set_active(self, n):
        """prove only the first n <= batch witnesses from the next prove() on (no reallocation: every buffer is proof-major)"""
        _ck(load().mp2g_prover_set_active(self.h, int(n)))
        self.active = int(n)

    def witness_status(self):
        """Per-proof flags of the last prove() (bit 0 copy constraint, bit 1 gate constraint); raises
        Mp2gError naming the first bad proof, like prove()'s panic in the reference."""
        flags = np.zeros(self.batch, dtype=np.uint32)
        rc = load().mp2g_prover_witness_status(self.h, _p(flags))
        if rc:
            err = Mp2gError(load().mp2g_last_error().decode())
            err.flags = flags
            raise err
        return flags

    def enable_graph(self, on=True):
        """Replay the launch sequence as a hipGraph from the third prove() with the same buffers on."""
        _ck(load().mp2g_prover_enable_graph(self.h, int(on)))

    STAGES = ("wires_commit", "z_partial_products", "quotient", "openings", "fri_commit_phase", "proof_of_work", "fri_queries")

    def enable_timing(self, on=True):
        _ck(load().mp2g_prover_enable_timing(self.h, int(on)))

    def stage_ms(self):
        """{stage: milliseconds} of the last prove() (HIP events on the prover's stream); synchronises."""
        out = (ctypes.c_float * len(self.STAGES))()
        _ck(load().mp2g_prover_stage_ms(self.h, out))
        return dict(zip(self.STAGES, [float(x) for x in out]))

    def prove(self, d_values, d_circuit_digest, d_pi_hash):
        """d_values: device buffers [batch][w_o][n] for oracles 1..; asynchronous."""
        ptrs = (ctypes.c_void_p * len(d_values))(*[(d.ptr.value if d is not None else None) for d in d_values])
        _ck(load().mp2g_prover_prove_dev(self.h, ptrs, d_circuit_digest.ptr, d_pi_hash.ptr, self.d_caps.ptr,
                                         self.d_openings.ptr, self.d_proof.ptr))

    def results(self):
        fp, B = self.fp, getattr(self, "active", self.batch)
        return (self.d_caps.download((B, fp.n_oracles, fp.cap_words)), self.d_openings.download((B, fp.n_openings, 2)),
                self.d_proof.download((B, fp.proof_words)))

    def free(self):
        if self.h and self.ctx.h:
            load().mp2g_prover_free(self.h)
        self.h = None


PI_HASH_GIVEN = 0xFFFFFFFF


def gate_table_line_points(gates, num_selectors):
    """mp2g_gate_table_line_points: the number of base-field points the verifier evaluates the gate constraints at (1 + the
    largest filtered constraint degree of the table). Host arithmetic: needs no GPU."""
    return int(load().mp2g_gate_table_line_points(gate_array(gates), len(gates), int(num_selectors)))


def verifier_part_words(fp, n_public_inputs):
    """the lengths of a proof's four parts in a parent's input order: public inputs (4 for PI_HASH_GIVEN: the hash), caps of
    oracles 1.., openings, FRI words. Host arithmetic (the layout mp2g_verifier_proof_words reports)."""
    n_pi = 4 if n_public_inputs == PI_HASH_GIVEN else int(n_public_inputs)
    return [n_pi, (fp.n_oracles - 1) * fp.cap_words, 2 * fp.n_openings, fp.proof_words]


class Verifier:
    """mp2g_verifier: VerifierCircuitData::verify for batches of proofs of one circuit, on the device. Status per proof: 0 accept,
    10 + a PLONK identity of challenge a, 1 proof of work, 2 initial Merkle path, 3 FRI layer consistency, 4 FRI layer Merkle path,
    5 final polynomial (2..5: the first failing check of the lowest failing query), 20 a non-canonical word."""

    def __init__(self, ctx, fp, constants_sigmas_cap, circuit_digest, gates, num_selectors, luts=None, num_routed=80, degree=8,
                 n_public_inputs=PI_HASH_GIVEN, capacity=1):
        self.ctx, self.fp, self.capacity, self.n_public_inputs = ctx, fp, int(capacity), n_public_inputs
        cap, dig = _arr(constants_sigmas_cap).ravel(), _arr(circuit_digest)
        assert cap.size == fp.cap_words and dig.size == 4
        arr = gate_array(gates)
        larr, keep = lookup_array(luts or [])
        self.h = ctypes.c_void_p()
        _ck(load().mp2g_verifier_create(ctx.h, ctypes.byref(fp), _p(cap), _p(dig), int(num_routed), int(degree), arr, len(gates),
                                        int(num_selectors), larr if luts else None, len(luts or []), n_public_inputs,
                                        self.capacity, ctypes.byref(self.h)))
        ctx._adopt(self)
        parts = (ctypes.c_uint32 * 4)()
        self.proof_words = load().mp2g_verifier_proof_words(self.h, parts)
        self.part_words = [int(x) for x in parts]

    def verify_dev(self, d_parts, strides, count):
        """d_parts: four device addresses (ints or DeviceBuffers), strides: words between consecutive proofs of each part"""
        ptrs = (ctypes.c_void_p * 4)(*[(d.ptr.value if isinstance(d, DeviceBuffer) else (int(d) if d else None)) for d in d_parts])
        st = (ctypes.c_uint64 * 4)(*[int(x) for x in strides])
        status = np.full(int(count), 0xFFFFFFFF, dtype=np.uint32)
        _ck(load().mp2g_verifier_verify_dev(self.h, ptrs, st, int(count), _p(status)))
        return status

    def verify(self, words):
        """words [count][proof_words] (host): contiguous proofs in a parent's input order"""
        w = _arr(words).reshape(-1, self.proof_words)
        status = np.full(w.shape[0], 0xFFFFFFFF, dtype=np.uint32)
        _ck(load().mp2g_verifier_verify(self.h, _p(w), w.shape[0], _p(status)))
        return status

    def challenges(self, count):
        """[count][words]: betas[2], gammas[2], alphas[2], zeta[2], the 8 lookup challenges, FRI alpha[2], FRI betas[n_layers][2],
        the PoW response, the query indices -- of the last verify call"""
        n = ctypes.c_size_t()
        _ck(load().mp2g_verifier_challenges(self.h, None, ctypes.byref(n)))
        out = np.zeros((int(count), n.value), dtype=np.uint64)
        _ck(load().mp2g_verifier_challenges(self.h, _p(out), ctypes.byref(n)))
        return out

    def free(self):
        if self.h and self.ctx.h:
            load().mp2g_verifier_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class WitnessProgram:
    """mp2g_witness_program: the witness generator of one circuit built by recursion.Builder (its recorded tape),
    replayed on the host for batches of input vectors. No GPU involved."""

    def __init__(self, ckt):
        tape, ins, cs = _arr(ckt.tape), _arr(ckt.input_sids, np.uint32), _arr(ckt.const_slots).reshape(-1, 2)
        self.log_n, self.n_inputs = ckt.log_n, int(ins.size)
        self.probe = _arr(np.concatenate([ckt.pi_hash_sids, ckt.public_input_sids]), np.uint32)
        self.n_public_inputs = int(ckt.public_input_sids.size)
        self.h = ctypes.c_void_p()
        _ck(load().mp2g_witness_program_create(_p(tape), tape.size, int(ckt.n_slots), int(ckt.log_n), _p(ins), int(ins.size),
                                               _p(cs), int(cs.shape[0]), ctypes.byref(self.h)))
        if getattr(ckt, "luts", None):
            self.set_lookups(ckt.luts)
        _ck(load().mp2g_witness_program_set_probe(self.h, _p(self.probe), int(self.probe.size)))
        self.n_levels = int(load().mp2g_witness_program_num_levels(self.h))

    def set_lookups(self, luts):
        """the circuit's lookup tables (the dicts a built circuit keeps in ckt.luts): a tape with MP2G_OP_LOOKUP needs them, and
        every replay then also fills the padding, the table rows and the multiplicities (prove()'s set_lookup_wires)"""
        arr, keep = lookup_array(luts)
        _ck(load().mp2g_witness_program_set_lookups(self.h, arr, len(luts)))

    def run_dev(self, ctx, d_inputs, batch, d_wires, d_probe):
        """the same replay on the device, stream ordered on ctx's stream: d_inputs [batch][n_inputs] -> d_wires [batch][135][n] (the
        prover's layout) and d_probe [batch][4 + n_public_inputs] (public-inputs hash, then the public inputs); asynchronous"""
        _ck(load().mp2g_witness_program_run_dev(self.h, ctx.h, d_inputs.ptr, int(batch), d_wires.ptr, d_probe.ptr))

    def run(self, inputs, threads=0, out=None, rows=False):
        """inputs [batch][n_inputs] -> (wires [batch][135][n], pi_hash [batch][4], public_inputs [batch][n_pi]);
        rows=True: the wires as [batch][n][135] (one contiguous row per gate row: faster to fill; Context.wires_from_rows_dev
        gives the prover's layout on the device)"""
        a = _arr(inputs).reshape(-1, self.n_inputs)
        B = a.shape[0]
        shape = (B, 1 << self.log_n, 135) if rows else (B, 135, 1 << self.log_n)
        wires = out if out is not None else np.empty(shape, dtype=np.uint64)
        assert wires.shape == shape
        probe = np.empty((B, self.probe.size), dtype=np.uint64)
        fn = load().mp2g_witness_program_run_rows if rows else load().mp2g_witness_program_run
        _ck(fn(self.h, _p(a), B, int(threads), _p(wires), _p(self.probe), int(self.probe.size), _p(probe)))
        return wires, probe[:, :4], probe[:, 4:]

    def free(self):
        if self.h:
            load().mp2g_witness_program_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ChainPatch(ctypes.Structure):
    _fields_ = [("job", ctypes.c_uint32), ("offset", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("pad_", ctypes.c_uint32), ("d_src", ctypes.c_void_p)]


class ProofChain:
    """mp2g_chain: generate_proof (base prove() + wrap chain) for batches of nodes of one framework circuit, on the device.
    provers: BatchedProver per step (set up for its circuit), programs: WitnessProgram per step, d_digests: DeviceBuffer per step."""

    def __init__(self, ctx, provers, programs, d_digests, capacity):
        n = len(provers)
        self.ctx, self.n_steps, self.capacity = ctx, n, capacity
        self.seconds_in_run = 0.0
        self.provers, self.programs, self.d_digests = list(provers), list(programs), list(d_digests)  # keep the handles alive
        self.fps = [p.fp for p in provers]
        pr = (ctypes.c_void_p * n)(*[p.h for p in provers])
        pg = (ctypes.c_void_p * n)(*[p.h for p in programs])
        fp = (FriParams * n)(*self.fps)
        dg = (ctypes.c_void_p * n)(*[d.ptr for d in d_digests])
        self.h = ctypes.c_void_p()
        _ck(load().mp2g_chain_create(ctx.h, n, pr, pg, fp, dg, int(capacity), ctypes.byref(self.h)))
        ctx._adopt(self)

    def run(self, inputs, patches=()):
        """inputs [B][n_inputs] (host); patches [(job, word offset, device address, n words)] -> (caps [B][4][cap words], openings
        [B][n][2], FRI proofs [B][words], public inputs [B][n_pi]) of the last step; raises on an unsatisfied witness"""
        a = _arr(inputs)
        B = a.shape[0]
        fp, prog = self.fps[-1], self.programs[-1]
        caps = np.empty((B, fp.n_oracles, fp.cap_words), dtype=np.uint64)
        openings = np.empty((B, fp.n_openings, 2), dtype=np.uint64)
        proofs = np.empty((B, fp.proof_words), dtype=np.uint64)
        pis = np.empty((B, prog.n_public_inputs), dtype=np.uint64)
        arr = (ChainPatch * max(1, len(patches)))(*[ChainPatch(int(j), int(off), int(n), 0, int(ptr)) for j, off, ptr, n in patches])
        t0 = time.perf_counter()
        _ck(load().mp2g_chain_run(self.h, _p(a), B, arr, len(patches), _p(caps), _p(openings), _p(proofs), _p(pis)))
        self.seconds_in_run += time.perf_counter() - t0  # inside the library (the GIL is released): what is left of a worker's time is host glue
        self.last_batch = B
        return caps, openings, proofs, pis

    def step_buffers(self, step):
        """raw device addresses of a step's (wires, probe, caps, openings, proof) after a run"""
        ptrs = [ctypes.c_void_p() for _ in range(5)]
        _ck(load().mp2g_chain_step_buffers(self.h, int(step), *[ctypes.byref(p) for p in ptrs]))
        return [p.value for p in ptrs]

    def device_proof(self, b=0):
        """[(device address, words)] x 4 of proof b of the last run: public inputs, the three caps, openings, FRI proof"""
        parts, words = (ctypes.c_void_p * 4)(), (ctypes.c_uint32 * 4)()
        _ck(load().mp2g_chain_device_proof(self.h, int(b), parts, words))
        return [(int(parts[i]), int(words[i])) for i in range(4)]

    def free(self):
        if self.h and self.ctx.h:
            load().mp2g_chain_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def forest_staging_words():
    """mp2g_forest_staging_words: the most words Forest.put_proofs / Forest.proofs move per chunk (one kernel and one synchronisation each)"""
    return int(load().mp2g_forest_staging_words())


class ForestCircuit(ctypes.Structure):
    _fields_ = [("n_inputs", ctypes.c_uint32), ("n_children", ctypes.c_uint32), ("child_offset", ctypes.c_uint32 * 4), ("n_const", ctypes.c_uint32)]


class Forest:
    """mp2g_forest: the native scheduler of a tree build (csrc/forest.hip). ctxs: one Context per worker; descriptors: [(n_inputs,
    [child offsets], n_const)] per circuit; chains[w][c]: the ProofChain of circuit c on worker w's context (None = never used there)."""

    def __init__(self, ctxs, descriptors, chains, slot_words, pool_slots):
        self.ctxs, self.chains = list(ctxs), [list(row) for row in chains]  # keep the handles alive
        nw, nc = len(ctxs), len(descriptors)
        d = (ForestCircuit * nc)()
        for i, (n_in, offs, n_const) in enumerate(descriptors):
            d[i].n_inputs, d[i].n_children, d[i].n_const = int(n_in), len(offs), int(n_const)
            for k, o in enumerate(offs):
                d[i].child_offset[k] = int(o)
        cx = (ctypes.c_void_p * nw)(*[c.h for c in ctxs])
        ch = (ctypes.c_void_p * (nw * nc))(*[(self.chains[w][c].h if self.chains[w][c] is not None else None) for w in range(nw) for c in range(nc)])
        self.h = ctypes.c_void_p()
        _ck(load().mp2g_forest_create(nw, cx, nc, d, ch, int(slot_words), int(pool_slots), ctypes.byref(self.h)))
        for c in self.ctxs:  # the forest holds raw pointers to every worker's context and chains: whichever closes first frees it
            c._adopt(self)
        self.n_const = [int(x[2]) for x in descriptors]
        self.n_children = [len(x[1]) for x in descriptors]

    def add_nodes(self, circuit, ids, child_ids, consts, keep=None):
        ids = _arr(ids)
        n = ids.size
        kids = _arr(child_ids).reshape(n, self.n_children[circuit]) if self.n_children[circuit] else None
        cs = _arr(consts).reshape(n, self.n_const[circuit])
        kp = np.ascontiguousarray(keep, dtype=np.uint8) if keep is not None else None
        _ck(load().mp2g_forest_add_nodes(self.h, int(circuit), int(n), _p(ids), _p(kids) if kids is not None else None, _p(cs), _p(kp) if kp is not None else None))

    def prove(self, units):
        """units: lists of node ids, independent of each other; the workers take them from a queue (the call releases the GIL)"""
        flat = _arr([i for u in units for i in u])
        offs = _arr(np.cumsum([0] + [len(u) for u in units]), np.uint32)
        _ck(load().mp2g_forest_prove(self.h, _p(flat), _p(offs), len(units)))

    def prove_plan(self, plan, group_nodes, n_satellites=0, satellite_shift=40):
        """drain an UpdatePlan (workplan.py) inside the library: the Ready items of every wave grouped into units of ~group_nodes plan
        nodes, proved, marked done, until the plan is finished. A plan node k = forest node k + its satellites ((j + 1) << shift) | k.
        Returns the items of every wave."""
        waves, per = ctypes.c_uint32(), (ctypes.c_uint32 * 64)()
        _ck(load().mp2g_forest_prove_plan(self.h, plan.h, int(group_nodes), int(n_satellites), int(satellite_shift), ctypes.byref(waves), per, 64))
        return [int(per[i]) for i in range(min(64, waves.value))]

    def proof_words(self, node_id):
        n = ctypes.c_uint32()
        _ck(load().mp2g_forest_proof(self.h, int(node_id), None, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.uint64)
        _ck(load().mp2g_forest_proof(self.h, int(node_id), _p(out), ctypes.byref(n)))
        return out

    def device_proof(self, node_id):
        """(device address, words) of a proved node's proof in the pool: public inputs, caps of oracles 1..3, openings, FRI words"""
        ptr, n = ctypes.c_void_p(), ctypes.c_uint32()
        _ck(load().mp2g_forest_device_proof(self.h, int(node_id), ctypes.byref(ptr), ctypes.byref(n)))
        return int(ptr.value), int(n.value)

    def verify(self, ids, verifier):
        """mp2g_forest_verify: the published nodes `ids` of ONE circuit verified where they lie in the device pool; `verifier` = the
        Verifier (or framework.CircuitVerifier) of that circuit's last chain step. Raises when an id is unknown or released."""
        ids = _arr(ids)
        status = np.full(ids.size, 0xFFFFFFFF, dtype=np.uint32)
        _ck(load().mp2g_forest_verify(self.h, getattr(verifier, "v", verifier).h, _p(ids), int(ids.size), _p(status)))
        return status

    def release(self, node_id):
        _ck(load().mp2g_forest_release(self.h, int(node_id)))

    def put_proofs(self, ids, proofs, keep=None):
        """mp2g_forest_put_proofs: register the external nodes `ids` with their proofs -- word arrays in a parent's input order (what
        proof_words returns), one per id or one [count][words] array -- in pool slots of their own; published on return. Raises, with
        nothing registered, on a known id, an empty or oversized proof, a full pool, a non-canonical word or a running prove()."""
        ids = _arr(ids).ravel()
        rows = [_arr(p).ravel() for p in proofs]
        if len(rows) != ids.size:
            raise Mp2gError(f"put_proofs: {ids.size} ids, {len(rows)} proofs")
        n_words = _arr([r.size for r in rows], np.uint32)
        stride = max([r.size for r in rows] + [1])
        words = np.zeros((ids.size, stride), dtype=np.uint64)
        for i, r in enumerate(rows):
            words[i, :r.size] = r
        kp = np.ascontiguousarray(keep, dtype=np.uint8) if keep is not None else None
        if kp is not None and kp.size != ids.size:
            raise Mp2gError(f"put_proofs: {ids.size} ids, {kp.size} keep flags")
        _ck(load().mp2g_forest_put_proofs(self.h, int(ids.size), _p(ids), _p(words), stride, _p(n_words), _p(kp) if kp is not None else None))

    def proofs(self, ids):
        """mp2g_forest_proofs: [proof_words(i) for i in ids] in one call (a gather kernel, a copy and a synchronisation per staging chunk
        instead of one of each per proof). Raises before anything is downloaded when an id is unknown, unproved or released."""
        ids = _arr(ids).ravel()
        if not ids.size:
            return []
        n_words = np.zeros(ids.size, dtype=np.uint32)
        _ck(load().mp2g_forest_proofs(self.h, _p(ids), int(ids.size), None, 0, _p(n_words)))
        stride = int(n_words.max())
        words = np.empty((ids.size, stride), dtype=np.uint64)
        _ck(load().mp2g_forest_proofs(self.h, _p(ids), int(ids.size), _p(words), stride, _p(n_words)))
        return [words[i, :int(n)].copy() for i, n in enumerate(n_words)]

    @property
    def free_slots(self):
        return int(load().mp2g_forest_free_slots(self.h))

    @property
    def proved(self):
        return load().mp2g_forest_proved(self.h)

    def free(self):
        if self.h and all(c.h for c in self.ctxs):
            load().mp2g_forest_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- Ecgfp5 multiset digest (mp2-common/src/group_hashing) ---------------------------------
def map_to_curve_batch(ctx, inputs, variant=POSEIDON2, weierstrass=False):
    """map_to_curve_point for each row of `inputs`; returns encodings [count][5] (and the 11-limb
    Weierstrass form when asked)."""
    a = _arr(inputs)
    count, in_len = a.shape
    w = np.empty((count, 5), dtype=np.uint64)
    wei = np.empty((count, 11), dtype=np.uint64) if weierstrass else None
    _ck(load().mp2g_map_to_curve_batch(ctx.h, variant, _p(a), in_len, count, _p(w), _p(wei) if weierstrass else None))
    return (w, wei) if weierstrass else w


def swu_batch(ctx, u, weierstrass=False):
    """simple_swu (sswu_value.rs:31-77) of each row of u [count][5] (GF(p^5) elements, coefficient i of z^i; limbs are any u64, read
    mod p), without map_to_curve_point's sponge; returns encodings [count][5] (and the 11-limb Weierstrass form when asked)."""
    a = _arr(u).reshape(-1, 5)
    count = a.shape[0]
    w = np.empty((count, 5), dtype=np.uint64)
    wei = np.empty((count, 11), dtype=np.uint64) if weierstrass else None
    _ck(load().mp2g_swu_batch(ctx.h, _p(a), count, _p(w), _p(wei) if weierstrass else None))
    return (w, wei) if weierstrass else w


def curve_sum(ctx, pts_w, weierstrass=False):
    a = _arr(pts_w).reshape(-1, 5)
    w = np.empty(5, dtype=np.uint64)
    wei = np.empty(11, dtype=np.uint64)
    _ck(load().mp2g_curve_sum(ctx.h, _p(a), a.shape[0], _p(w), _p(wei)))
    return (w, wei) if weierstrass else w


def curve_sum_ranges(ctx, pts_w, ranges):
    """the sum of pts_w[start:end] for every (start, end) of `ranges` in one call: the accumulated digest of every node of a
    tree laid out in order. Returns (encodings [n][5], Weierstrass forms [n][11])."""
    a = _arr(pts_w).reshape(-1, 5)
    r = _arr(ranges, np.uint32).reshape(-1, 2)
    w = np.empty((r.shape[0], 5), dtype=np.uint64)
    wei = np.empty((r.shape[0], 11), dtype=np.uint64)
    _ck(load().mp2g_curve_sum_ranges(ctx.h, _p(a), a.shape[0], _p(r), r.shape[0], _p(w), _p(wei)))
    return w, wei


def scalar_mul_batch(ctx, pts_w, scalars, weierstrass=False):
    """scalars: python ints < 2^128 (hash_to_int_value range). Returns the encodings [count][5] (and the 11-limb Weierstrass
    forms = Point::to_fields when asked)."""
    a = _arr(pts_w).reshape(-1, 5)
    k = _arr([[(int(s) >> (32 * i)) & 0xFFFFFFFF for i in range(4)] for s in scalars], np.uint32).reshape(-1, 4)
    out = np.empty((a.shape[0], 5), dtype=np.uint64)
    wei = np.empty((a.shape[0], 11), dtype=np.uint64) if weierstrass else None
    _ck(load().mp2g_scalar_mul_batch(ctx.h, _p(a), _p(k), a.shape[0], _p(out), _p(wei) if weierstrass else None))
    return (out, wei) if weierstrass else out


def field_hashed_scalar_mul(ctx, inputs, base_w, variant=POSEIDON2):
    a, b = _arr(inputs), _arr(base_w)
    w = np.empty(5, dtype=np.uint64)
    wei = np.empty(11, dtype=np.uint64)
    _ck(load().mp2g_field_hashed_scalar_mul(ctx.h, variant, _p(a), a.size, _p(b), _p(w), _p(wei)))
    return w, wei


def u256_to_limbs(values):
    """U256 -> 8 big-endian u32 words, most significant first (mp2-common/src/u256.rs:870-877)."""
    out = np.empty((len(values), 8), dtype=np.uint32)
    for i, v in enumerate(values):
        v = int(v)
        for j in range(8):
            out[i, j] = (v >> (32 * (7 - j))) & 0xFFFFFFFF
    return out


def compute_table_row_digest(ctx, col_ids, values, unique, variant=POSEIDON2):
    """compute_table_row_digest (mp2-v1/src/values_extraction/mod.rs:527-571).
    values: uint32 [rows][n_cols][8]; unique: uint32 [rows][n_unique][8]."""
    ids = _arr(col_ids)
    v = _arr(values, np.uint32)
    u = _arr(unique, np.uint32)
    rows, n_cols = v.shape[0], ids.size
    n_unique = u.shape[1] if u.ndim == 3 else 0
    w = np.empty(5, dtype=np.uint64)
    wei = np.empty(11, dtype=np.uint64)
    _ck(load().mp2g_row_digest_batch(ctx.h, variant, _p(ids), n_cols, _p(v), _p(u), n_unique, rows, _p(w), _p(wei)))
    return w, wei


def row_digests(ctx, col_ids, values, unique, variant=POSEIDON2):
    """the per-row terms of compute_table_row_digest, row_id * sum_c D(id_c || value_c): (encodings [rows][5], Weierstrass [rows][11])"""
    ids = _arr(col_ids)
    v = _arr(values, np.uint32)
    u = _arr(unique, np.uint32)
    rows, n_cols = v.shape[0], ids.size
    n_unique = u.shape[1] if u.ndim == 3 else 0
    w = np.empty((rows, 5), dtype=np.uint64)
    wei = np.empty((rows, 11), dtype=np.uint64)
    _ck(load().mp2g_row_digests(ctx.h, variant, _p(ids), n_cols, _p(v), _p(u), n_unique, rows, _p(w), _p(wei)))
    return w, wei


# ---- tables in contract storage (csrc/extraction.hip; the reference's names and orderings: extraction.py) -------------------------
def _bytes32(a, inner=None):
    """uint8 [count][32] (or [count][inner][32]) of words / keys given as arrays or as a list of 32-byte strings"""
    if isinstance(a, (list, tuple)) and a and isinstance(a[0], (bytes, bytearray)):
        a = np.frombuffer(b"".join(a), dtype=np.uint8)
    a = _arr(a, np.uint8)
    return a.reshape(-1, 32) if inner is None else a.reshape(-1, inner, 32)


def extract_values(ctx, words, layout):
    """mp2g_extract_values: extract_value (column_gadget.rs:326-368) of every word [count][32] under every layout row (byte offset,
    bit offset, length in bits); uint32 [count][n_cols][8], the cell format of row_digests and the cells-tree calls"""
    w, lay = _bytes32(words), _arr(layout, np.uint32).reshape(-1, 3)
    out = np.zeros((w.shape[0], lay.shape[0], 8), dtype=np.uint32)
    _ck(load().mp2g_extract_values(ctx, _p(w), _p(lay), lay.shape[0], w.shape[0], _p(out)))
    return out


def extract_values_dev(ctx, d_words, layout, count, d_out):
    """mp2g_extract_values_dev: the same from d_words [count][32] (16-byte aligned) into d_out [count][n_cols][8]; stream ordered;
    layout is a host array"""
    lay = _arr(layout, np.uint32).reshape(-1, 3)
    _ck(load().mp2g_extract_values_dev(ctx, d_words, _p(lay), lay.shape[0], int(count), d_out))


def leaf_values_digests(ctx, col_ids, layout, n_table_columns, words, keys=None, key_ids=(), evm_word=0, variant=POSEIDON2):
    """mp2g_leaf_values_digests: the values digest of every storage leaf (mod.rs:327-341, :374-406, :450-496). col_ids / layout: the
    extracted columns; words [count][32]; keys [count][n_keys][32] with n_keys = len(key_ids). Returns (encodings [count][5],
    Weierstrass [count][11], (encoding, Weierstrass) of the sum of all leaves)."""
    ids, lay, kid = _arr(col_ids).ravel(), _arr(layout, np.uint32).reshape(-1, 3), _arr(key_ids).ravel()
    w = _bytes32(words)
    count = w.shape[0]
    k = _bytes32(keys, kid.size) if kid.size else np.zeros((count, 0, 32), dtype=np.uint8)
    if lay.shape[0] != ids.size or k.shape[0] != count:
        raise ValueError("one layout row per extracted column and one key set per word are needed")
    out_w, out_wei = np.zeros((count, 5), dtype=np.uint64), np.zeros((count, 11), dtype=np.uint64)
    sum_w, sum_wei = np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    _ck(load().mp2g_leaf_values_digests(ctx, int(variant), _p(ids), _p(lay), ids.size, int(n_table_columns), _p(w), _p(k), _p(kid), kid.size,
                                        int(evm_word), count, _p(out_w), _p(out_wei), _p(sum_w), _p(sum_wei)))
    return out_w, out_wei, (sum_w, sum_wei)


def leaf_values_digests_dev(ctx, variant, col_ids, layout, n_table_columns, d_words, d_keys, key_ids, evm_word, count, d_frac_out=None,
                            each=False, total=True):
    """mp2g_leaf_values_digests_dev: the same from d_words [count][32] and d_keys [count][n_keys][32] (16-byte aligned); the leaves'
    points go to d_frac_out [count][20] when given. Returns (encodings, Weierstrass forms, (encoding, Weierstrass) of the sum): the
    first two None without `each`, the last None without `total`; with neither the call is stream ordered."""
    ids, lay, kid = _arr(col_ids).ravel(), _arr(layout, np.uint32).reshape(-1, 3), _arr(key_ids).ravel()
    count = int(count)
    out_w, out_wei = (np.zeros((count, 5), dtype=np.uint64), np.zeros((count, 11), dtype=np.uint64)) if each else (None, None)
    sum_w, sum_wei = (np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)) if total else (None, None)
    _ck(load().mp2g_leaf_values_digests_dev(ctx, int(variant), _p(ids), _p(lay), ids.size, int(n_table_columns), d_words, d_keys, _p(kid),
                                            kid.size, int(evm_word), count, d_frac_out, None if out_w is None else _p(out_w),
                                            None if out_wei is None else _p(out_wei), None if sum_w is None else _p(sum_w),
                                            None if sum_wei is None else _p(sum_wei)))
    return out_w, out_wei, ((sum_w, sum_wei) if total else None)


# ---- Keccak-256: storage slot keys and MPT leaf words (csrc/storage.hip; the reference's names: extraction.py) ---------------------
MPT_LEAF_OK, MPT_LEAF_MALFORMED, MPT_LEAF_NOT_A_LEAF, MPT_LEAF_BAD_VALUE, MPT_LEAF_KEY_MISMATCH = range(5)


def rows_at_stride(msgs, stride=None, fill=0):
    """(uint8 [count][stride], uint32 lens [count]) of a list of byte strings of unequal length (or of a uint8 [count][len] array):
    one row per message at a stride that is a multiple of 8, the bytes past a message's end set to `fill`"""
    if isinstance(msgs, np.ndarray):
        msgs = [bytes(r) for r in np.ascontiguousarray(msgs, dtype=np.uint8).reshape(len(msgs), -1)]
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    if stride is None:
        stride = max(8, (int(lens.max(initial=0)) + 7) // 8 * 8)
    rows = np.full((len(msgs), stride), fill, dtype=np.uint8)
    for r, m in zip(rows, msgs):
        r[:min(len(m), stride)] = np.frombuffer(bytes(m)[:stride], dtype=np.uint8)
    return rows, lens


def _opt(a):
    return None if a is None else _p(a)


def keccak256_batch(ctx, msgs, stride=None):
    """mp2g_keccak256_batch: keccak256 of every message (a list of byte strings of unequal length); uint8 [count][32]. Read as eight
    little-endian u32 words a digest is pack(Endianness::Little), the H public input."""
    rows, lens = rows_at_stride(msgs, stride)
    out = np.zeros((len(lens), 32), dtype=np.uint8)
    _ck(load().mp2g_keccak256_batch(ctx, _p(rows), rows.shape[1], _p(lens), 0, len(lens), _p(out)))
    return out


def keccak256_batch_dev(ctx, d_msgs, stride, d_lens, length, count, d_out):
    """mp2g_keccak256_batch_dev: d_msgs [count][stride] (8-byte aligned, stride a multiple of 8), d_lens [count] uint32 or None (every
    message has `length` bytes) into d_out [count][32]; a device length above stride is clamped; stream ordered"""
    _ck(load().mp2g_keccak256_batch_dev(ctx, d_msgs, int(stride), d_lens, int(length), int(count), d_out))


def storage_slot_keys(ctx, slot, keys=None, n_keys=0, evm_offset=0, parents=None, count=None):
    """mp2g_storage_slot_keys: StorageSlot::location / mpt_key / mpt_nibbles (eth.rs:233-276) of `count` leaves under `slot` (or under
    parents [count][32]), keys [count][n_keys][32] left-padded, the outer key first. Returns (locations [count][32], mpt_keys
    [count][32], nibbles [count][64], number of leaves whose location + evm_offset overflowed and were zeroed)."""
    n_keys = int(n_keys)
    k = _bytes32(keys, n_keys) if n_keys else None
    par = _bytes32(parents) if parents is not None else None
    if count is None:
        count = k.shape[0] if k is not None else (par.shape[0] if par is not None else 1)
    if (k is not None and k.shape[0] != count) or (par is not None and par.shape[0] != count):
        raise ValueError("one key set and one parent per leaf are needed")
    loc, key, nib = (np.zeros((count, w), dtype=np.uint8) for w in (32, 32, 64))
    over = ctypes.c_uint32(0)
    _ck(load().mp2g_storage_slot_keys(ctx, int(slot), _opt(par), _opt(k), n_keys, int(evm_offset), count, _p(loc), _p(key), _p(nib),
                                      ctypes.byref(over)))
    return loc, key, nib, over.value


def storage_slot_keys_dev(ctx, slot, d_parents, d_keys, n_keys, evm_offset, count, d_locations=None, d_mpt_keys=None, d_nibbles=None,
                          overflow=True):
    """mp2g_storage_slot_keys_dev: the same between device buffers (8-byte aligned; each output may be None). Returns the number of
    overflowed leaves, or None without `overflow`: then the call is stream ordered."""
    over = ctypes.c_uint32(0)
    _ck(load().mp2g_storage_slot_keys_dev(ctx, int(slot), d_parents, d_keys, int(n_keys), int(evm_offset), int(count), d_locations,
                                          d_mpt_keys, d_nibbles, ctypes.byref(over) if overflow else None))
    return over.value if overflow else None


def mpt_storage_leaves(ctx, nodes, mpt_keys=None, stride=None):
    """mp2g_mpt_storage_leaves: every MPT storage leaf node (a list of byte strings of unequal length) hashed and opened. Returns
    (hashes [count][32], words [count][32] = left_pad32(value), n_nibbles [count], status [count] of MPT_LEAF_*); with mpt_keys
    [count][32] the path must be the key's tail."""
    rows, lens = rows_at_stride(nodes, stride)
    count = len(lens)
    k = _bytes32(mpt_keys) if mpt_keys is not None else None
    if k is not None and k.shape[0] != count:
        raise ValueError("one MPT key per node is needed")
    hashes, words = np.zeros((count, 32), dtype=np.uint8), np.zeros((count, 32), dtype=np.uint8)
    nib, status = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    _ck(load().mp2g_mpt_storage_leaves(ctx, _p(rows), rows.shape[1], _p(lens), _opt(k), count, _p(hashes), _p(words), _p(nib), _p(status)))
    return hashes, words, nib, status


def mpt_storage_leaves_dev(ctx, d_nodes, stride, d_lens, d_mpt_keys, count, d_hashes=None, d_words=None, d_n_nibbles=None, d_status=None):
    """mp2g_mpt_storage_leaves_dev: the same between device buffers (d_nodes, d_hashes, d_words 8-byte aligned; each output may be
    None); stream ordered"""
    _ck(load().mp2g_mpt_storage_leaves_dev(ctx, d_nodes, int(stride), d_lens, d_mpt_keys, int(count), d_hashes, d_words, d_n_nibbles,
                                           d_status))


# ---- MPT inclusion proofs: nodes opened once, paths walked to the root (csrc/mpt.hip; the proof sets: extraction.py) ----------------
MPT_MAX_DEPTH = 65
MPT_NODE_INVALID, MPT_NODE_BRANCH, MPT_NODE_EXTENSION, MPT_NODE_LEAF = range(4)
MPT_NODE_MALFORMED, MPT_NODE_ITEM_COUNT, MPT_NODE_EMBEDDED_CHILD, MPT_NODE_BRANCH_VALUE, MPT_NODE_BAD_PREFIX = range(1, 6)
MPT_VALUE_WORD, MPT_VALUE_ACCOUNT, MPT_VALUE_RAW = range(3)
(MPT_PATH_OK, MPT_PATH_BAD_PATH, MPT_PATH_ROOT_MISMATCH, MPT_PATH_HASH_MISMATCH, MPT_PATH_BAD_NODE, MPT_PATH_LEAF_ABOVE, MPT_PATH_NO_LEAF,
 MPT_PATH_KEY_LENGTH, MPT_PATH_EMPTY_CHILD, MPT_PATH_KEY_MISMATCH, MPT_PATH_BAD_VALUE) = range(11)
MPT_PATH_OUTPUTS = ("status", "fail_level", "words", "val_off", "val_len", "consumed")


def mpt_open_nodes(ctx, nodes, stride=None):
    """mp2g_mpt_open_nodes: every node (a list of byte strings of unequal length) hashed and opened. Returns (hashes [n_nodes][32],
    info [n_nodes] uint32: kind, reason, header length, branch mask or nibble count and item 1's offset, as include/mp2g.h packs
    them)."""
    rows, lens = rows_at_stride(nodes, stride)
    hashes, info = np.zeros((len(lens), 32), dtype=np.uint8), np.zeros(len(lens), dtype=np.uint32)
    _ck(load().mp2g_mpt_open_nodes(ctx, _p(rows), rows.shape[1], _p(lens), len(lens), _p(hashes), _p(info)))
    return hashes, info


def mpt_open_nodes_dev(ctx, d_nodes, stride, d_lens, n_nodes, d_hashes=None, d_info=None):
    """mp2g_mpt_open_nodes_dev: the same between device buffers (d_nodes, d_hashes 8-byte aligned; each output may be None); stream
    ordered"""
    _ck(load().mp2g_mpt_open_nodes_dev(ctx, d_nodes, int(stride), d_lens, int(n_nodes), d_hashes, d_info))


def mpt_verify_paths(ctx, nodes, paths, depths, mpt_keys, roots=None, mode=MPT_VALUE_WORD, stride=None):
    """mp2g_mpt_verify_paths: the proofs paths [count][max_depth] (indices into `nodes`, a list of byte strings; the root first) of
    depths [count] walked under mpt_keys [count][32]. roots: None (not checked), 32 bytes (one root for all) or [count][32]. Returns
    a dict of MPT_PATH_OUTPUTS: status (MPT_PATH_*), fail_level, words [count][32], val_off, val_len, consumed [count][max_depth]."""
    rows, lens = rows_at_stride(nodes, stride)
    paths, depths, k = _arr(paths, np.uint32), _arr(depths, np.uint32).ravel(), _bytes32(mpt_keys)
    count = depths.size
    paths = paths.reshape(count, -1) if count else paths.reshape(0, 1)
    if k.shape[0] != count:
        raise ValueError("one MPT key per path is needed")
    r = None if roots is None else _bytes32([roots] if isinstance(roots, (bytes, bytearray)) else roots)
    if r is not None and r.shape[0] not in (1, count):
        raise ValueError("one root, or one root per path, is needed")
    out = {"status": np.zeros(count, dtype=np.uint32), "fail_level": np.zeros(count, dtype=np.uint32),
           "words": np.zeros((count, 32), dtype=np.uint8), "val_off": np.zeros(count, dtype=np.uint32),
           "val_len": np.zeros(count, dtype=np.uint32), "consumed": np.zeros(paths.shape, dtype=np.uint8)}
    root_stride = 32 if r is not None and r.shape[0] == count else 0
    _ck(load().mp2g_mpt_verify_paths(ctx, _p(rows), rows.shape[1], _p(lens), len(lens), _p(paths), _p(depths), paths.shape[1], _p(k), count,
                                     _opt(r), root_stride, int(mode), *(_p(out[name]) for name in MPT_PATH_OUTPUTS)))
    return out


def mpt_verify_paths_dev(ctx, d_nodes, stride, d_lens, d_hashes, d_info, n_nodes, d_paths, d_depths, max_depth, d_mpt_keys, count,
                         d_roots=None, root_stride=0, mode=MPT_VALUE_WORD, d_status=None, d_fail_level=None, d_words=None, d_val_off=None,
                         d_val_len=None, d_consumed=None):
    """mp2g_mpt_verify_paths_dev: the same between device buffers, over the hashes and info words mpt_open_nodes_dev left (d_nodes,
    d_hashes, d_roots, d_words 8-byte aligned; d_roots and each output may be None); stream ordered"""
    _ck(load().mp2g_mpt_verify_paths_dev(ctx, d_nodes, int(stride), d_lens, d_hashes, d_info, int(n_nodes), d_paths, d_depths, int(max_depth),
                                         d_mpt_keys, int(count), d_roots, int(root_stride), int(mode), d_status, d_fail_level, d_words,
                                         d_val_off, d_val_len, d_consumed))


# ---- MPT subtree digests: DV and N of every trie node (csrc/mpt_digest.hip; the public-input rows: extraction.py) ------------------
MPT_NO_NODE = 0xFFFFFFFF
MPT_SUBTREE_UNREACHED, MPT_SUBTREE_OK, MPT_SUBTREE_CONFLICT = range(3)
MPT_SUBTREE_OUTPUTS = ("n_leaves", "state", "via", "parent", "entered")


def mpt_subtree_digests(ctx, nodes, paths, depths, mpt_keys, leaf_w, roots=None, mode=MPT_VALUE_WORD, stride=None, points=True):
    """mp2g_mpt_subtree_digests: the proofs as mpt_verify_paths takes them, and the leaves' digests as encodings leaf_w [count][5] by
    proof. Returns a dict: status [count] (MPT_PATH_*), w [n_nodes][5] and weierstrass [n_nodes][11] (every node's sum; None without
    `points`, and leaf_w may then be None), n_leaves, state (MPT_SUBTREE_*), via, parent [n_nodes] uint32, entered [n_nodes] uint8,
    totals (rejected proofs, conflict nodes, levels)."""
    rows, lens = rows_at_stride(nodes, stride)
    n = len(lens)
    paths, depths, k = _arr(paths, np.uint32), _arr(depths, np.uint32).ravel(), _bytes32(mpt_keys)
    count = depths.size
    paths = paths.reshape(count, -1) if count else paths.reshape(0, 1)
    if k.shape[0] != count:
        raise ValueError("one MPT key per path is needed")
    r = None if roots is None else _bytes32([roots] if isinstance(roots, (bytes, bytearray)) else roots)
    if r is not None and r.shape[0] not in (1, count):
        raise ValueError("one root, or one root per path, is needed")
    lw = None if leaf_w is None else _arr(leaf_w).reshape(-1, 5)
    if points and (lw is None or lw.shape[0] != count):
        raise ValueError("one leaf digest per path is needed")
    out = {"status": np.zeros(count, dtype=np.uint32), "w": np.zeros((n, 5), dtype=np.uint64) if points else None,
           "weierstrass": np.zeros((n, 11), dtype=np.uint64) if points else None, "n_leaves": np.zeros(n, dtype=np.uint32),
           "state": np.zeros(n, dtype=np.uint32), "via": np.zeros(n, dtype=np.uint32), "parent": np.zeros(n, dtype=np.uint32),
           "entered": np.zeros(n, dtype=np.uint8), "totals": np.zeros(3, dtype=np.uint32)}
    root_stride = 32 if r is not None and r.shape[0] == count else 0
    _ck(load().mp2g_mpt_subtree_digests(ctx, _p(rows), rows.shape[1], _p(lens), n, _p(paths), _p(depths), paths.shape[1], _p(k), count, _opt(r),
                                        root_stride, int(mode), _opt(lw if points else None), _p(out["status"]), _opt(out["w"]),
                                        _opt(out["weierstrass"]), *(_p(out[name]) for name in MPT_SUBTREE_OUTPUTS), _p(out["totals"])))
    return out


def mpt_subtree_digests_dev(ctx, d_info, n_nodes, d_paths, d_depths, max_depth, d_mpt_keys, d_status, count, d_leaf_frac, d_acc_frac=None,
                            d_n_leaves=None, d_state=None, d_via=None, d_parent=None, d_entered=None):
    """mp2g_mpt_subtree_digests_dev: the same between device buffers, over the info words mpt_open_nodes_dev left and the statuses
    mpt_verify_paths_dev left (d_status None: every proof counts as OK); d_leaf_frac [count][20] as leaf_values_digests_dev leaves
    its d_frac_out; each output may be None. One synchronisation. Returns (rejected proofs, conflict nodes, levels)."""
    totals = np.zeros(3, dtype=np.uint32)
    _ck(load().mp2g_mpt_subtree_digests_dev(ctx, d_info, int(n_nodes), d_paths, d_depths, int(max_depth), d_mpt_keys, d_status, int(count),
                                            d_leaf_frac, d_acc_frac, d_n_leaves, d_state, d_via, d_parent, d_entered, _p(totals)))
    return tuple(int(t) for t in totals)


# ---- node hashes of a table's trees (csrc/index_hash.hip) ------------------------------------
class TreeShape:
    """mp2g_tree_shape: a binary tree or forest over nodes 0..n-1 by its children arrays (-1 = no child), checked and levelled on
    the host (csrc/tree_shape.h); needs no GPU. A malformed forest raises Mp2gError with the fault's name."""

    def __init__(self, handle):
        self.h = handle
        lib = load()
        self.size, self.num_levels, self.num_roots = (int(f(self.h)) for f in (lib.mp2g_tree_shape_size, lib.mp2g_tree_shape_num_levels,
                                                                                 lib.mp2g_tree_shape_num_roots))

    @classmethod
    def from_children(cls, left, right):
        l, r = _arr(left, np.int32).ravel(), _arr(right, np.int32).ravel()
        if l.size != r.size:
            raise ValueError("left and right differ in length")
        h = ctypes.c_void_p()
        _ck(load().mp2g_tree_shape_create(_p(l), _p(r), l.size, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def sbbst(cls, n):
        """ryhope's sbbst over positions 1..n (position k = node k - 1)"""
        h = ctypes.c_void_p()
        _ck(load().mp2g_tree_shape_sbbst(int(n), ctypes.byref(h)))
        return cls(h)

    def describe(self):
        """{left, right (int32), height, min_idx, max_idx (uint32): [n]; roots: [num_roots] ascending}"""
        n = self.size
        out = {k: np.empty(n, dtype=np.int32) for k in ("left", "right")}
        out.update({k: np.empty(n, dtype=np.uint32) for k in ("height", "min_idx", "max_idx")})
        out["roots"] = np.empty(self.num_roots, dtype=np.uint32)
        _ck(load().mp2g_tree_shape_describe(self.h, *(_p(out[k]) for k in ("left", "right", "height", "min_idx", "max_idx", "roots"))))
        return out

    def touched(self, nodes):
        """mp2g_tree_shape_touched: the given nodes and all their ancestors (ryhope's touched(), ryhope/src/lib.rs:216-222), uint32,
        grouped by height (ascending height, ascending node index inside a height); duplicates collapse. Needs no GPU."""
        t = _arr(nodes, np.uint32).ravel()
        n = ctypes.c_uint32()
        _ck(load().mp2g_tree_shape_touched(self.h, _p(t), t.size, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        _ck(load().mp2g_tree_shape_touched(self.h, _p(t), t.size, _p(out), n.value, ctypes.byref(n)))
        return out

    def free(self):
        if self.h:
            load().mp2g_tree_shape_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def cells_tree_hashes_dev(ctx, variant, col_ids, d_values, rows, d_roots, d_nodes=None):
    """mp2g_cells_tree_hashes_dev: stream ordered, no synchronisation; col_ids is a host array"""
    ids = _arr(col_ids).ravel()
    _ck(load().mp2g_cells_tree_hashes_dev(ctx, int(variant), _p(ids), ids.size, d_values, rows, d_roots, d_nodes))


def row_tree_hashes_dev(ctx, variant, shape, ident, d_values, value_stride, d_payload, d_hashes):
    """mp2g_row_tree_hashes_dev: stream ordered, no synchronisation. The shape joins the context's handles: closing the context
    frees it (a shape is freed before the context it was used with)."""
    if ctx is not None:
        ctx._adopt(shape)
    _ck(load().mp2g_row_tree_hashes_dev(ctx, int(variant), shape.h, int(ident), d_values, int(value_stride), d_payload, d_hashes))


def row_tree_update_fused_width():
    """mp2g_row_tree_update_fused_width: the widest level of a touched closure that mp2g_row_tree_hashes_update still hashes in one launch"""
    return int(load().mp2g_row_tree_update_fused_width())


def cells_tree_hashes_rows_dev(ctx, variant, col_ids, d_values, rows, row_idx, d_roots, d_nodes=None):
    """mp2g_cells_tree_hashes_rows_dev: the cells trees of the listed rows only; stream ordered; col_ids and row_idx are host arrays"""
    ids, idx = _arr(col_ids).ravel(), _arr(row_idx, np.uint32).ravel()
    _ck(load().mp2g_cells_tree_hashes_rows_dev(ctx, int(variant), _p(ids), ids.size, d_values, rows, _p(idx), idx.size, d_roots, d_nodes))


def row_tree_hashes_update_dev(ctx, variant, shape, ident, d_values, value_stride, d_payload, touched, d_hashes):
    """mp2g_row_tree_hashes_update_dev: the touched nodes and their ancestors only; stream ordered; touched is a host array. The
    shape joins the context's handles as in row_tree_hashes_dev."""
    if ctx is not None:
        ctx._adopt(shape)
    t = _arr(touched, np.uint32).ravel()
    _ck(load().mp2g_row_tree_hashes_update_dev(ctx, int(variant), shape.h, int(ident), d_values, int(value_stride), d_payload,
                                               _p(t), t.size, d_hashes))


# ---- accumulated digests of a table's trees (csrc/tree_digest.hip): points stay on the device as 20 words each --------------------
FRAC_BYTES = 160  # one point in fractional coordinates (X:Z:U:T, 5 limbs each): a representative, not a canonical form


def curve_decode_dev(ctx, pts_w, d_frac):
    """mp2g_curve_decode_dev: the encodings pts_w [count][5] decoded into d_frac [count][20]; refuses a limb >= p and an invalid
    encoding. One synchronisation."""
    a = _arr(pts_w).reshape(-1, 5)
    _ck(load().mp2g_curve_decode_dev(ctx, _p(a), a.shape[0], d_frac))


def curve_emit_dev(ctx, d_frac, count, idx=None):
    """mp2g_curve_emit_dev: (encodings [k][5], Weierstrass forms [k][11]) of the points idx (a host list whose entries the caller
    keeps inside d_frac) or, without one, of the points 0..count-1. One synchronisation."""
    i = None if idx is None else _arr(idx, np.uint32).ravel()
    k = int(count) if i is None else i.size
    w, wei = np.zeros((k, 5), dtype=np.uint64), np.zeros((k, 11), dtype=np.uint64)
    _ck(load().mp2g_curve_emit_dev(ctx, d_frac, None if i is None else _p(i), k, _p(w), _p(wei)))
    return w, wei


def tree_digests_dev(ctx, shape, d_own, d_acc):
    """mp2g_tree_digests_dev: acc[i] = own[i] + acc[left[i]] + acc[right[i]] for every node of the shape, one launch per level;
    stream ordered. The shape joins the context's handles as in row_tree_hashes_dev."""
    if ctx is not None:
        ctx._adopt(shape)
    _ck(load().mp2g_tree_digests_dev(ctx, shape.h, d_own, d_acc))


def tree_digests(ctx, shape, own_w):
    """mp2g_tree_digests: the same from encodings own_w [n][5] in host memory; returns (encodings [n][5], Weierstrass [n][11])"""
    a = _arr(own_w).reshape(-1, 5)
    if a.shape[0] != shape.size:
        raise ValueError("own_w has not one encoding per node of the shape")
    if ctx is not None:
        ctx._adopt(shape)
    w, wei = np.zeros((shape.size, 5), dtype=np.uint64), np.zeros((shape.size, 11), dtype=np.uint64)
    _ck(load().mp2g_tree_digests(ctx, shape.h, _p(a), _p(w), _p(wei)))
    return w, wei


def tree_digests_update_fused_width():
    """mp2g_tree_digests_update_fused_width: the widest level of a touched closure that mp2g_tree_digests_update_dev still sums in one launch"""
    return int(load().mp2g_tree_digests_update_fused_width())


def tree_digests_update_dev(ctx, shape, d_own, touched, d_acc):
    """mp2g_tree_digests_update_dev: the touched nodes and their ancestors only; stream ordered; touched is a host array"""
    if ctx is not None:
        ctx._adopt(shape)
    t = _arr(touched, np.uint32).ravel()
    _ck(load().mp2g_tree_digests_update_dev(ctx, shape.h, d_own, _p(t), t.size, d_acc))


def cells_tree_digests_dev(ctx, variant, col_ids, d_values, rows, d_nodes, row_idx=None):
    """mp2g_cells_tree_digests_dev: every node of every row's cells tree (row_idx None), or of the listed rows only, into d_nodes
    [rows][n_cols-1][20]; stream ordered; col_ids and row_idx are host arrays"""
    ids = _arr(col_ids).ravel()
    idx = None if row_idx is None else _arr(row_idx, np.uint32).ravel()
    _ck(load().mp2g_cells_tree_digests_dev(ctx, int(variant), _p(ids), ids.size, d_values, int(rows), None if idx is None else _p(idx),
                                           0 if idx is None else idx.size, d_nodes))


def row_digests_dev(ctx, variant, col_ids, d_values, d_unique, unique_stride, n_unique, rows, d_own, d_cells_nodes=None, row_idx=None):
    """mp2g_row_digests_dev: the rows' own digests row_id * sum_c D(id_c || value_c) into d_own [rows][20]; with d_cells_nodes (what
    cells_tree_digests_dev wrote) the cells' part of the sum is taken from the cells tree's root. Stream ordered."""
    ids = _arr(col_ids).ravel()
    idx = None if row_idx is None else _arr(row_idx, np.uint32).ravel()
    _ck(load().mp2g_row_digests_dev(ctx, int(variant), _p(ids), ids.size, d_values, d_unique, int(unique_stride), int(n_unique), int(rows),
                                    d_cells_nodes, None if idx is None else _p(idx), 0 if idx is None else idx.size, d_own))


def leaf_permutations_queued():
    """permutations the Merkle leaf sponge has queued since the library was loaded (mp2g_stat_leaf_permutations)"""
    return int(load().mp2g_stat_leaf_permutations())


# ---- proof wire format (mp2-common/src/proof.rs) ---------------------------------------------
def serialize_proof(fp, num_constants, caps, openings, fri_proof, public_inputs):
    """bincode bytes of ProofWithPublicInputs (mp2-common/src/proof.rs:84-98 serialize_proof)."""
    caps, openings, fri_proof = _arr(caps), _arr(openings), _arr(fri_proof)
    pis = _arr(public_inputs)
    n = ctypes.c_size_t()
    _ck(load().mp2g_proof_serialize(ctypes.byref(fp), num_constants, _p(caps), _p(openings), _p(fri_proof), _p(pis), pis.size, None, ctypes.byref(n)))
    out = np.empty(n.value, dtype=np.uint8)
    _ck(load().mp2g_proof_serialize(ctypes.byref(fp), num_constants, _p(caps), _p(openings), _p(fri_proof), _p(pis), pis.size, _p(out), ctypes.byref(n)))
    return out.tobytes()


def deserialize_proof(fp, num_constants, data, n_public_inputs):
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    caps = np.zeros((fp.n_oracles, fp.cap_words), dtype=np.uint64)
    openings = np.zeros((fp.n_openings, 2), dtype=np.uint64)
    fri = np.zeros(fp.proof_words, dtype=np.uint64)
    pis = np.zeros(n_public_inputs, dtype=np.uint64)
    _ck(load().mp2g_proof_deserialize(ctypes.byref(fp), num_constants, _p(buf), buf.size, _p(caps), _p(openings),
                                      _p(fri), _p(pis), n_public_inputs))
    return caps, openings, fri, pis


def serialize_proof_with_vk(proof_bytes, vk_cap, vk_circuit_digest):
    """ProofWithVK::serialize (mp2-common/src/proof.rs:42-52)."""
    pb = np.frombuffer(proof_bytes, dtype=np.uint8).copy()
    cap, dig = _arr(vk_cap).reshape(-1, 4), _arr(vk_circuit_digest)
    n = ctypes.c_size_t()
    _ck(load().mp2g_proof_with_vk_serialize(_p(pb), pb.size, _p(cap), cap.shape[0], _p(dig), None, ctypes.byref(n)))
    out = np.empty(n.value, dtype=np.uint8)
    _ck(load().mp2g_proof_with_vk_serialize(_p(pb), pb.size, _p(cap), cap.shape[0], _p(dig), _p(out), ctypes.byref(n)))
    return out.tobytes()


def deserialize_proof_with_vk(fp, num_constants, data, n_public_inputs, vk_cap_len=None):
    """ProofWithVK::deserialize (mp2-common/src/proof.rs:54-57): (caps, openings, fri words, public inputs) with caps[0] = the
    verifier key's constants_sigmas cap (what the prover hands out for a proof it made), and the key's circuit digest."""
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    n_cap = (1 << fp.cap_height) if vk_cap_len is None else int(vk_cap_len)
    caps = np.zeros((fp.n_oracles, fp.cap_words), dtype=np.uint64)
    openings = np.zeros((fp.n_openings, 2), dtype=np.uint64)
    fri = np.zeros(fp.proof_words, dtype=np.uint64)
    pis = np.zeros(n_public_inputs, dtype=np.uint64)
    vk_cap = np.zeros((n_cap, 4), dtype=np.uint64)
    dig = np.zeros(4, dtype=np.uint64)
    _ck(load().mp2g_proof_with_vk_deserialize(ctypes.byref(fp), num_constants, _p(buf), buf.size, _p(caps), _p(openings),
                                              _p(fri), _p(pis), n_public_inputs, _p(vk_cap), n_cap, _p(dig)))
    if vk_cap.size == caps[0].size:
        caps[0] = vk_cap.ravel()
    return (caps, openings, fri, pis), vk_cap, dig


# ---- recursion-framework pieces that sit on the path ------------------------------------------
# recursion-framework/src/universal_verifier_gadget/mod.rs:27-40, circuit_builder.rs:26
CIRCUIT_SET_CAP_HEIGHT = 0
RECURSION_THRESHOLD = 12
SHRINK_LIMIT = 15
MIN_CIRCUIT_SIZE = 64
NUM_HASH_OUT_ELTS = 4


def hash_pad_input(values):
    """plonky2 Hasher::hash_pad padding: append 1, zeros to rate-1 (mod 8), append 1."""
    v = [int(x) for x in values] + [1]
    while (len(v) + 1) % 8:
        v.append(0)
    return v + [1]


def circuit_digest(ctx, constants_sigmas_cap, degree_bits, variant=POSEIDON2, domain_separator=()):
    """recursion-framework/src/universal_verifier_gadget/circuit_set.rs:136-158:
    H(flatten(constants_sigmas_cap) || H_pad(domain separator) || degree_bits); the framework's circuits have no domain
    separator, a base circuit may (CircuitBuilder::set_domain_separator, wrap_circuit.rs:327-358)."""
    cap = [int(x) for x in _arr(constants_sigmas_cap).reshape(-1)]
    domain_sep = [int(x) for x in ctx.hash_no_pad(hash_pad_input(domain_separator), variant)]
    return ctx.hash_no_pad(cap + domain_sep + [degree_bits], variant)


class CircuitSet:
    """Merkle set of circuit digests (circuit_set.rs:173-237): leaves in insertion order, padded
    to a power of two with [0] leaves, cap height 0; the root is the 4 extra public inputs of
    every framework proof (circuit_builder.rs:169-171)."""

    def __init__(self, ctx, digests, variant=POSEIDON2):
        d = _arr(digests).reshape(-1, 4)
        self.digests = d
        n = max(1, d.shape[0])
        size = 1 << (n - 1).bit_length()
        leaves = np.zeros((size, 4), dtype=np.uint64)
        leaves[:d.shape[0]] = d
        self.tree = MerkleTree(ctx, leaves, CIRCUIT_SET_CAP_HEIGHT, variant)

    def circuit_set_digest(self):
        return self.tree.cap[0]

    def membership_proof(self, digest):
        """(leaf index little-endian bits, siblings) as set_circuit_membership_target assigns them
        (circuit_set.rs:205-237)."""
        digest = _arr(digest)
        hits = [i for i in range(self.digests.shape[0]) if np.array_equal(self.digests[i], digest)]
        if not hits:
            raise KeyError("circuit digest not found")  # circuit_set.rs:212 "circuit digest not found"
        idx = hits[0]
        _, sib = self.tree.prove([idx])
        bits = [(idx >> i) & 1 for i in range(self.tree.log_leaves)]
        return bits, sib[0]


def compute_table_row_digest_dev(ctx, d_col_ids, n_cols, d_values, d_unique, n_unique, rows, variant=POSEIDON2):
    """Device-resident form of compute_table_row_digest; returns the encoded digest."""
    w = np.empty(5, dtype=np.uint64)
    _ck(load().mp2g_row_digest_batch_dev(ctx.h, variant, d_col_ids.ptr, n_cols, d_values.ptr, d_unique.ptr, n_unique, rows,
                                         None, _p(w), None))
    return w


def partial_products_and_zs(ctx, wires, sigmas, betas, gammas, degree=8):
    """plonk/prover.rs all_wires_permutation_partial_products in prove()'s commit order."""
    wv, sg, b, g = _arr(wires), _arr(sigmas), _arr(betas), _arr(gammas)
    num_routed, n = sg.shape
    out = np.empty((b.size * (num_routed // degree), n), dtype=np.uint64)
    _ck(load().mp2g_partial_products_and_zs(ctx.h, _p(wv), wv.shape[0], _p(sg), int(n).bit_length() - 1, num_routed, degree,
                                            _p(b), _p(g), b.size, _p(out)))
    return out


def fri_prove(ctx, fp, oracles, zeta, challenger):
    """PolynomialBatch::prove_openings over committed batches (granular path for hosts that compute
    the quotient polynomials themselves). Returns the flat FriProof."""
    hs = (ctypes.c_void_p * len(oracles))(*[o.h.value for o in oracles])
    z = _arr(zeta)
    proof = np.empty(fp.proof_words, dtype=np.uint64)
    _ck(load().mp2g_fri_prove(ctx.h, ctypes.byref(fp), hs, _p(z), challenger.h, _p(proof)))
    return proof
