"""time the HOST replay of the wrap circuit's witness program (mp2g_witness_program_run_rows; no GPU):
    MP2G_LIB=OLD/libmp2gpu.so python tools/dbg/witness_host_timing.py [threads [batch [repetitions]]]
prints the repetitions' times and their median. To compare two builds run it for each in turn, several times over (the library is
chosen by MP2G_LIB), and hold the difference of the medians against the spread of one build's own runs."""
import importlib, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle as O
from test_recursion import verifier_data
mp2 = importlib.import_module("mapreduce-plonky2_amd")
R = importlib.import_module("mapreduce-plonky2_amd.recursion")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
threads, batch, reps = (int(a) for a in (sys.argv[1:] + ["1", "8", "7"][len(sys.argv) - 1:])[:3])
base = R.map_circuit(O.rand_field(4, 77))
cap, cd = verifier_data(base)
inner = R.InnerCircuit(base, FW.circuit_fri_params(base), cap, cd, len(base.public_inputs))
w = R.wrap_circuit(inner, *R.dummy_proof(inner), strict=False)  # the replay's work does not depend on the proof's values
prog = mp2.WitnessProgram(w)
inp = np.tile(np.asarray(w.input_values, dtype=np.uint64), (batch, 1))
out = np.empty((batch, 1 << w.log_n, 135), dtype=np.uint64)
assert np.array_equal(prog.run(inp, threads, out=out, rows=True)[0][0].T, w.wires)
ms = []
for _ in range(reps):
    t0 = time.perf_counter()
    prog.run(inp, threads, out=out, rows=True)
    ms.append((time.perf_counter() - t0) * 1e3)
print(f"{os.path.basename(os.path.dirname(os.path.abspath(mp2.LIB_PATH)))}: {len(w.tape)} tape words, batch {batch}, {threads} threads: "
      f"{' '.join(f'{x:.1f}' for x in ms)} ms, median {statistics.median(ms):.1f} ms")
