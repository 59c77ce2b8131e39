"""csrc/gate_shape.h -- the one table of what a gate kind is -- and gate_table_make (csrc/gates.h), compiled for the host under
-fsanitize=undefined (tools/hosttest/gate_shape_test.cpp, a stand-alone program) and held against
  * circuits.py's gate_num_constraints / gate_degree (Python integers: no overflow) over the gate sets the GPU tests prove;
  * the parameter ranges of include/mp2g.h, written out below;
  * descriptors whose counts overflow 32 bits or whose parameters would be shifted or divided by unchecked: all refused, with a
    clean exit;
  * tests/golden/gate_shape_parent.json: the table verdict and the four counts that the five separate definitions this header
    replaced (gate_num_constraints, gate_degree, gate_footprint, the per-kind rules of gate_table_check) gave for the descriptors
    of the first two checks -- recorded from that text by a throw-away host program, not recomputed here.
The public queries (mp2g_gate_num_constraints, mp2g_gate_degree, mp2g_gate_table_line_points) need the library and no GPU."""
import json
import os
import subprocess

import pytest

import circuits as C
import hosttest

U32 = 0xFFFFFFFF
# the CosetInterpolationGate parameters tests/test_gpu_gates_extension.py sweeps, restated (a host test does not import a GPU test):
# every subgroup size with the smallest degree whose wires fit and the largest the quotient allows
COSET = [(C.COSET_INTERPOLATION, b, d, 0) for b in range(2, 6)
         for d in (next(d for d in range(2, (1 << b) + 1) if 1 + 2 * (1 << b) + 6 + 4 * (((1 << b) - 2) // (d - 1)) <= C.NUM_WIRES),
                   min(1 << b, C.MAX_DEGREE))]
LIGHT = {C.CONSTANT, C.PUBLIC_INPUT, C.ARITHMETIC, C.BASE_SUM, C.ARITHMETIC_EXT, C.MUL_EXT}

# (kind, a well-formed (p0, p1, p2), then per documented range: (index of the parameter, lowest, highest or None)). From the comments
# of include/mp2g.h: RandomAccess bits <= 6, CosetInterpolation subgroup_bits 2..5 with degree 2..2^bits, U32AddMany addends <= 16,
# Comparison chunks of at most 4 bits (num_chunks <= num_bits <= 4 num_chunks), BaseSum base >= 2; and a count of 0 is refused where
# the gate needs an operation, slot, limb, coefficient, power bit or copy. Constant, Arithmetic, ArithmeticExtension and MulExtension
# take any count (0 gives a gate without constraints), RandomAccess any number of extra constants.
RANGES = [
    (C.NOOP, (0, 0, 0)), (C.PUBLIC_INPUT, (0, 0, 0)), (C.POSEIDON2, (0, 0, 0)), (C.POSEIDON, (0, 0, 0)), (C.POSEIDON_MDS, (0, 0, 0)),
    (C.CONSTANT, (2, 0, 0), (0, 0, None)), (C.ARITHMETIC, (20, 0, 0), (0, 0, None)), (C.ARITHMETIC_EXT, (10, 0, 0), (0, 0, None)),
    (C.MUL_EXT, (13, 0, 0), (0, 0, None)),
    (C.BASE_SUM, (20, 4, 0), (0, 1, None), (1, 2, None)),
    (C.EXPONENTIATION, (66, 0, 0), (0, 1, None)), (C.REDUCING, (43, 0, 0), (0, 1, None)), (C.REDUCING_EXT, (32, 0, 0), (0, 1, None)),
    (C.RANDOM_ACCESS, (4, 4, 2), (0, 1, 6), (1, 1, None), (2, 0, None)),
    (C.RANDOM_ACCESS, (6, 1, 0), (0, 1, 6)),
    (C.COSET_INTERPOLATION, (2, 2, 0), (0, 2, 5), (1, 2, 4)), (C.COSET_INTERPOLATION, (3, 2, 0), (1, 2, 8)),
    (C.COSET_INTERPOLATION, (4, 2, 0), (1, 2, 16)), (C.COSET_INTERPOLATION, (5, 32, 0), (0, 5, 5), (1, 2, 32)),
    (C.U32_ARITHMETIC, (3, 0, 0), (0, 1, None)), (C.U32_RANGE_CHECK, (7, 0, 0), (0, 1, None)), (C.U32_SUBTRACTION, (6, 0, 0), (0, 1, None)),
    (C.U32_ADD_MANY, (3, 5, 0), (0, 1, 16), (1, 1, None)),
    (C.COMPARISON, (32, 16, 0), (0, 16, 64), (1, 8, 32)), (C.COMPARISON, (4, 1, 0), (0, 1, 4), (1, 1, 4)),
    (C.LOOKUP, (40, 0, 0), (0, 1, None)), (C.LOOKUP_TABLE, (26, 0, 0), (0, 1, None)),
    (C.U32_INTERLEAVE, (3, 0, 0), (0, 1, None)), (C.UNINTERLEAVE_TO_B32, (2, 0, 0), (0, 1, None)), (C.UNINTERLEAVE_TO_U32, (2, 0, 0), (0, 1, None)),
]
# counts that wrap in 32 bits, shifts and divisions by unchecked parameters, unknown kinds: (kind, p0, p1, p2)
MALFORMED = [(C.U32_RANGE_CHECK, 0xF0F0F0F1, 0, 0), (C.U32_ARITHMETIC, 0x80000000, 0, 0), (C.U32_INTERLEAVE, 0x80000000, 0, 0),
             (C.LOOKUP, 0x80000000, 0, 0), (C.COSET_INTERPOLATION, 3, 1, 0), (C.COSET_INTERPOLATION, 40, 0, 0), (C.COMPARISON, 200, 1, 0),
             (C.U32_ADD_MANY, 11, 0x08000000, 0), (25, 0, 0, 0), (U32, 0, 0, 0), (C.COSET_INTERPOLATION, 3, 0, 0)]


def circuit_descriptors():
    """the gate sets the GPU tests prove, each descriptor once"""
    return list(dict.fromkeys(C.ALL_KINDS + C.LEAF_KINDS + C.VERIFIER_KINDS + C.LOOKUP_KINDS + COSET))


def range_descriptors():
    """[(descriptor, inside its ranges)]: each end of each range of RANGES and one step outside it"""
    out = {}
    for kind, base, *ranges in RANGES:
        out[(kind,) + base] = True
        for idx, lo, hi in ranges:
            for v in sorted({lo, lo - 1, hi, None if hi is None else hi + 1} - {None, -1}):
                p = list(base)
                p[idx] = v
                out[(kind,) + tuple(p)] = lo <= v and (hi is None or v <= hi)
    return list(out.items())


def recorded_descriptors():
    """what tests/golden/gate_shape_parent.json holds: the first two checks' descriptors, without CosetInterpolation of degree 1,
    where the earlier definitions divided by zero"""
    ds = list(dict.fromkeys(circuit_descriptors() + [d for d, _ in range_descriptors()]))
    return [d for d in ds if not (d[0] == C.COSET_INTERPOLATION and d[2] == 1)]


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    exe = hosttest.build(tmp_path_factory.mktemp("gate_shape"), "gate_shape_test",
                         flags=("-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"))

    def run(descriptors):
        """[(shape = (constraints, degree, wires, consts, light) or None, table accepted)]"""
        r = subprocess.run([exe], input="\n".join(" ".join(str(x) for x in d) for d in descriptors), capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-300:] + r.stderr
        out = []
        for line in r.stdout.splitlines():
            t = line.split("#")[0].split()
            assert t[0] == "shape" and t[-2] == "table" and t[-1] in ("ok", "refused") and len(t) in (4, 8), line
            out.append((None if t[1] == "refused" else tuple(int(x) for x in t[1:6]), t[-1] == "ok"))
        assert len(out) == len(descriptors)
        return out
    return run


def test_counts_are_the_python_builders(shapes):
    ds = circuit_descriptors()
    for d, (shape, table_ok) in zip(ds, shapes(ds)):
        g = C.Gate(*d, 0, 0, 1)
        assert shape is not None and table_ok, d
        assert shape[:2] == (C.gate_num_constraints(g), C.gate_degree(g)), d
        assert shape[4] == (d[0] in LIGHT), d
    assert {d[0] for d in ds} == set(range(25))


def test_parameter_ranges(shapes):
    cases = range_descriptors()
    assert {d[0] for d, _ in cases} == set(range(25))
    got = shapes([d for d, _ in cases])
    for (d, inside), (shape, table_ok) in zip(cases, got):
        assert (shape is not None) == inside, d
        assert not table_ok or inside, d  # a table never takes what the shape refuses


def test_overflowing_and_malformed_descriptors_are_refused(shapes):
    for d, (shape, table_ok) in zip(MALFORMED, shapes(MALFORMED)):  # shapes() itself asserts exit status 0 and an empty stderr
        assert shape is None and not table_ok, d


def test_nothing_else_moved(shapes):
    golden = json.load(open(os.path.join(hosttest.ROOT, "tests", "golden", "gate_shape_parent.json")))["cases"]
    ds = recorded_descriptors()
    assert [tuple(c[:4]) for c in golden] == ds  # the file holds exactly the descriptors of the two checks above
    for c, (shape, table_ok) in zip(golden, shapes(ds)):
        assert table_ok == bool(c[4]), c
        if shape is not None:  # a refused descriptor has no counts; an accepted one has the counts it always had
            assert list(shape[:4]) == c[5:9], c
        assert shape is not None or not c[4], c


def test_gate_descriptor_queries(mp2):
    for k in C.ALL_KINDS:
        og = C.Gate(*k, 0, 0, 0)
        g = mp2.Gate(*k, 0, 0, 0)
        assert g.num_constraints == C.gate_num_constraints(og) and g.degree == C.gate_degree(og)
    for d in MALFORMED:
        g = mp2.Gate(*d, 0, 0, 1)
        assert g.num_constraints == 0 and g.degree == 0 and mp2.gate_table_line_points([g], 1) == 0, d
