"""Compiles a host-side test program of tools/hosttest/ for the tests that run one: the csrc/ headers under test compiled for the
host alone (hipcc -x hip --cuda-host-only), no GPU and no library needed unless the caller links one. A plain helper module."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapreduce-plonky2_amd", "csrc")


def build(out_dir, program, flags=("-O2",), link=(), mp2g_h=True):
    """tools/hosttest/<program>.cpp -> <out_dir>/<program>; `flags` go before the source, `link` (objects, linker options) after it;
    mp2g_h: the program reads include/mp2g.h"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(str(out_dir), program)
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", *flags, "-std=c++17", "-I" + CSRC, *(["-I" + os.path.join(ROOT, "include")] if mp2g_h else []),
                           os.path.join(ROOT, "tools", "hosttest", program + ".cpp"), *link, "-o", exe])
    return exe
