"""csrc/coset_constants.h (subgroup points and barycentric weights of CosetInterpolationGate) against the host field code of
csrc/gl.cuh -- gl_root_of_unity, gl_inv, gl_mul, compiled for the host -- and against an independent computation: the barycentric
weights from their definition 1 / prod_{j != i} (x_i - x_j), and every entry as a signed power of two."""
import os
import re
import subprocess

import hosttest
import oracle as O

P = O.P
CSRC = os.path.join(O.ROOT, "mapreduce-plonky2_amd", "csrc")


def header_tables():
    out = {}
    for m in re.finditer(r"uint64_t (\w+)\[(\d+)\] = \{(.*?)\};", open(os.path.join(CSRC, "coset_constants.h")).read(), re.S):
        out[m.group(1)] = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", m.group(3))]
        assert len(out[m.group(1)]) == int(m.group(2))
    return out


def test_tables_from_the_definition():
    t = header_tables()
    assert set(t) == {"COSET_POINTS", "COSET_WEIGHTS"} and len(t["COSET_POINTS"]) == len(t["COSET_WEIGHTS"]) == 4 + 8 + 16 + 32
    for k in range(2, 6):
        n, off = 1 << k, (1 << k) - 4
        xs, ws = t["COSET_POINTS"][off:off + n], t["COSET_WEIGHTS"][off:off + n]
        w = pow(7277203076849721926, 1 << (32 - k), P)
        assert pow(w, n, P) == 1 and pow(w, n // 2, P) == P - 1
        assert xs == [pow(w, i, P) for i in range(n)]
        for i in range(n):
            d = 1
            for j in range(n):
                if j != i:
                    d = d * (xs[i] - xs[j]) % P
            assert ws[i] == pow(d, P - 2, P)  # coset_interpolation.rs barycentric_weights
            # a power of two up to sign: 2 has order 192, w = 2^(192 / n), 1 / n = 2^(192 - k)
            assert xs[i] == pow(2, i * 192 // n, P) and ws[i] == pow(2, (i * 192 // n + 192 - k) % 192, P)


def test_tables_against_the_host_field_code(tmp_path):
    exe = hosttest.build(tmp_path, "coset_constants_test", flags=("-O2", "-DMP2G_DEVCONST=static const"), mp2g_h=False)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["checked", "60", "bad", "0"], r.stdout + r.stderr
