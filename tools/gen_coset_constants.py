"""Writes mapreduce-plonky2_amd/csrc/coset_constants.h: for the 2^k-point subgroups, k = 2..5, of CosetInterpolationGate the points
x_i = w^i (w = POWER_OF_TWO_GENERATOR^(2^(32-k))) and the barycentric weights x_i / 2^k.   usage: python tools/gen_coset_constants.py"""
import os

P = 2**64 - 2**32 + 1
TWO_GEN = 7277203076849721926

HEAD = '''// CosetInterpolationGate: the points of the 2^k-point subgroup, x_i = w^i with w = gl_root_of_unity(k), and the barycentric weights
// x_i / 2^k, for k = 2..5; the table of size 2^k starts at entry 2^k - 4. Every entry is a power of two up to sign (w_64 = 2^3,
// 1/2 = 2^191). Written by tools/gen_coset_constants.py; checked against the host field code and an independent computation by
// tests/test_coset_constants.py.
#ifndef MP2G_COSET_CONSTANTS_H
#define MP2G_COSET_CONSTANTS_H
#include <stdint.h>
#ifndef MP2G_DEVCONST
#define MP2G_DEVCONST static __device__ __constant__
#endif
#define MP2G_COSET_TABLE(bits) ((1u << (bits)) - 4)
'''


def table(name, f):
    vals = []
    for k in range(2, 6):
        n = 1 << k
        w = pow(TWO_GEN, 1 << (32 - k), P)
        vals += [f(pow(w, i, P), n) for i in range(n)]
    s = f"MP2G_DEVCONST uint64_t {name}[{len(vals)}] = {{\n"
    for i in range(0, len(vals), 4):
        s += "  " + " ".join(f"0x{v:016x}ULL," for v in vals[i:i + 4]) + "\n"
    return s + "};\n"


if __name__ == "__main__":
    out = HEAD + table("COSET_POINTS", lambda x, n: x) + table("COSET_WEIGHTS", lambda x, n: x * pow(n, P - 2, P) % P) + "#endif\n"
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapreduce-plonky2_amd", "csrc", "coset_constants.h")
    with open(path, "w") as f:
        f.write(out)
