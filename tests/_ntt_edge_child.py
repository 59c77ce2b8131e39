"""Child process of tests/test_gpu_edge_operands.py: the edge-operand NTT cases of tests/edge_inputs.py through whichever kernel
family the environment selects (MP2G_NTT_V1), one line `log_n label sha256` per case. argv[1]: the repository root."""
import importlib
import sys

sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import edge_inputs as X  # noqa: E402

mp2 = importlib.import_module("mapreduce-plonky2_amd")
ctx = mp2.Context(0)
for log_n in X.NTT_LOG_N:
    for label, a, mode, _ in X.ntt_cases(log_n):
        print(log_n, label, X.digest(ctx.ntt(a, **mode)))
ctx.close()
