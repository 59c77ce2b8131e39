"""time the replay of a program of the wide opcode block (tests/test_gpu_witness_tape_wide.py's circuit: 600 interleaves on one
level, a chain of xors, div_u256, two BigUintDivRem hints, PoseidonMds) on the device and on the host:
    python tools/dbg/wide_ops_timing.py [repetitions]
device: mp2g_witness_program_run_dev between device events, one warm-up, then the repetitions and their median, at batch 1 and 48;
host: mp2g_witness_program_run_rows on 16 threads by tools/dbg/witness_host_timing.py's method (wall clock around the call, median)."""
import importlib, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_witness_tape_wide import wide_circuit, wide_input_vector, wide_inputs
mp2 = importlib.import_module("mapreduce-plonky2_amd")
R = importlib.import_module("mapreduce-plonky2_amd.recursion")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ck = wide_circuit(wide_inputs(0x6D0), independent=600)
prog = mp2.WitnessProgram(ck)
n = 1 << ck.log_n
wide = sum(1 for _, op in R.tape_instructions(ck.tape) if op >= 48)
print(f"log_n {ck.log_n}, {len(ck.tape)} tape words, {wide} wide instructions, {prog.n_levels} levels, {prog.n_inputs} inputs")
ctx = mp2.Context(0)
for B in (1, 48):
    inp = np.array([wide_input_vector(wide_inputs(0x6D0 + k)) for k in range(B)], dtype=np.uint64)
    d_in, d_w, d_pr = ctx.to_device(inp), ctx.alloc(B * 135 * n * 8), ctx.alloc(B * prog.probe.size * 8)
    prog.run_dev(ctx, d_in, B, d_w, d_pr); ctx.sync()
    out = np.empty((B, n, 135), dtype=np.uint64)
    assert np.array_equal(d_w.download((B, 135, n)), np.ascontiguousarray(prog.run(inp, 16, out=out, rows=True)[0].transpose(0, 2, 1)))
    dev, host = [], []
    for _ in range(reps):
        ctx.timer_start()
        prog.run_dev(ctx, d_in, B, d_w, d_pr)
        dev.append(ctx.timer_stop())
    for _ in range(reps):
        t0 = time.perf_counter()
        prog.run(inp, 16, out=out, rows=True)
        host.append((time.perf_counter() - t0) * 1e3)
    print(f"B={B}: device {' '.join(f'{x:.3f}' for x in dev)} ms, median {statistics.median(dev):.3f} ms; "
          f"host (16 threads) {' '.join(f'{x:.2f}' for x in host)} ms, median {statistics.median(host):.2f} ms")
    d_in.free(); d_w.free(); d_pr.free()
ctx.close()
