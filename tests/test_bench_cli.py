"""bench.py's command line on a box without GPUs: `--gpus N` starts its own ranks only when N devices are visible, and says so
otherwise (before anything touches a GPU)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_devices_is_refused_with_a_message():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MP2G_BENCH_BACKEND")}
    env["HIP_VISIBLE_DEVICES"] = ""  # also on a GPU box: no device visible to this child
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0
    assert "--gpus 2 needs 2 visible GPUs" in r.stderr + r.stdout


def test_default_workload_is_the_table_build():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "table (default, the headline)" in " ".join(r.stdout.split())


def test_resume_dir_is_a_single_gpu_mode(tmp_path):
    """`--resume-dir` builds the table's blocks one after another on one GPU; asked for together with several GPUs it says so before
    any rank is started or any GPU touched"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MP2G_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--resume-dir", str(tmp_path / "s")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "--resume-dir builds the blocks one after another on ONE GPU" in r.stderr + r.stdout
    assert not (tmp_path / "s").exists()


def test_block_plan_rows_per_rank():
    """the rows of a rank's block: --steps x the rows of a step (1024 without --rows), so that the timed work grows with --steps and
    --steps 128 gives every rank a 2^17-row block -- 8 ranks build the metric's 2^20-row table (+ 7 separator rows); the warm-up block
    is --warmup steps and never exceeds 5120 rows"""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.block_plan(None, 20, 5) == (20 * 1024, 1024, 5120)
    assert [bench.block_plan(None, k, 1)[0] for k in (1, 2, 5)] == [1024, 2048, 5120]
    n, per_step, warm = bench.block_plan(None, 128, 1)
    assert n == 1 << 17 and per_step == 1024 and warm == 1024
    assert 8 * n == 1 << 20 and 8 * n + 7 == 1048583
    assert bench.block_plan(None, 5, 0)[2] == 0 and bench.block_plan(None, 5, 9)[2] == 5120
    assert bench.block_plan(1024, 20, 5) == (20480, 1024, 5120) and bench.block_plan(1024, 20, 9)[2] == 5120
    assert bench.block_plan(8, 2, 1) == (16, 8, 8)
    assert bench.block_plan(None, 4, 1, default_step_rows=16) == (64, 16, 16)
    os.environ["MP2G_BENCH_STEP_ROWS"] = "24"
    try:
        assert bench.block_plan(None, 5, 2) == (120, 24, 48)
        assert bench.block_plan(8, 5, 2) == (40, 8, 16)  # --rows wins over the default
    finally:
        del os.environ["MP2G_BENCH_STEP_ROWS"]


def test_full_and_dump_outputs_options():
    """`--full` (everything beyond the headline) and `--dump-outputs DIR` are on the command line; the dump belongs to the table
    workload and is refused elsewhere before any GPU is touched"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MP2G_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "ntt", "--dump-outputs", "x"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0 and "--dump-outputs writes the root proof of the timed table block" in r.stderr + r.stdout


def test_dump_outputs_is_exact(tmp_path):
    """dump_outputs writes a root proof's four parts as float64 [low, high] 32-bit halves: every u64 word comes back exactly"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    rng = np.random.default_rng(7)
    P = (1 << 64) - (1 << 32) + 1
    proof = tuple(rng.integers(0, P, size=s, dtype=np.uint64) for s in ((3, 16, 4), (90, 2), (4000,), (38,)))
    proof[2][:3] = [0, P - 1, (1 << 53) + 1]  # words a float64 of the whole word would round
    names = bench.dump_outputs(str(tmp_path / "d"), proof)
    assert names == ["root_caps", "root_fri_proof", "root_openings", "root_public_inputs"]
    for name, want in zip(("root_caps", "root_openings", "root_fri_proof", "root_public_inputs"), proof):
        a = np.load(str(tmp_path / "d" / (name + ".npy")))
        assert a.dtype == np.float64 and a.shape == want.shape + (2,)
        got = a[..., 0].astype(np.uint64) | (a[..., 1].astype(np.uint64) << np.uint64(32))
        assert np.array_equal(got, want)


def test_cpu_throughput_sweep_reports_the_best_mode():
    """bench.py's cpu_baseline as THROUGHPUT: the sampled framework proofs proved P side by side x T OpenMP threads each by the oracle;
    the value reported is the best mode's. Here on a small circuit (the GPU run hands it the timed block's captured witnesses)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import bench
    import circuits as C
    import oracle as O
    ckt = C.build(5, C.ALL_KINDS, 1)
    ofp = O.standard_params(5, (ckt.num_constants + C.NUM_ROUTED, C.NUM_WIRES, 20, 16), pow_bits=4, num_queries=2)
    cd = O.rand_field(4, 2)
    chain = lambda name: [(f"{name} step {i}", ckt, ofp, cd, (lambda: ckt.wires), ckt.pi_hash) for i in range(2)]
    samples = [chain("cells_leaf"), chain("cells_full"), chain("row_leaf"), chain("row_full")]
    best, sweep = bench.cpu_throughput(samples, seconds_per_mode=0.3, modes=[(2, 1), (1, 2)])
    assert len(sweep["modes"]) == 2 and all(m["framework_proofs"] >= m["concurrent_proofs"] and m["proofs_per_s"] > 0 for m in sweep["modes"])
    assert best["proofs_per_s"] == max(m["proofs_per_s"] for m in sweep["modes"]) and sweep["memory_cap"]["max_concurrent"] >= 1
    # the default modes: P x T = the host's threads, capped by memory
    _, sweep = bench.cpu_throughput(samples, seconds_per_mode=0.05)
    cores = os.cpu_count()
    assert [(m["concurrent_proofs"], m["threads_per_proof"]) for m in sweep["modes"]][0] == (cores, 1)


def test_cpu_farm_runs_the_throughput_modes_as_processes():
    """the farm behind cpu_baseline's throughput modes: a helper process (started before the GPU is touched in a real run) spawns P
    worker processes per mode, each maps the spooled samples and proves framework proofs with T OpenMP threads; here two modes on a
    small circuit, and the fallback to threads when no farm is there"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    import circuits as C
    import oracle as O
    ckt = C.build(5, C.ALL_KINDS, 1)
    ofp = O.standard_params(5, (ckt.num_constants + C.NUM_ROUTED, C.NUM_WIRES, 20, 16), pow_bits=4, num_queries=2)
    cd = O.rand_field(4, 2)
    chain = lambda name: [(f"{name} step {i}", ckt, ofp, cd, (lambda: ckt.wires), ckt.pi_hash) for i in range(2)]
    samples = [chain("cells_leaf"), chain("cells_full"), chain("row_leaf"), chain("row_full")]
    farm = bench.CpuFarm()
    try:
        assert farm.p is not None
        best, sweep = bench.cpu_throughput_modes(samples, farm, 0.3)
        assert "separate processes" in sweep["how"] and len(sweep["modes"]) >= 1
        cores = os.cpu_count()
        assert sweep["modes"][0]["threads_per_proof"] in (1, 4) and sweep["modes"][0]["concurrent_proofs"] * sweep["modes"][0]["threads_per_proof"] <= cores
        assert all(m["workers_failed"] == 0 and m["framework_proofs"] >= m["concurrent_proofs"] and m["proofs_per_s"] > 0 for m in sweep["modes"])
        assert best["proofs_per_s"] == max(m["proofs_per_s"] for m in sweep["modes"])
    finally:
        farm.close()
    best, sweep = bench.cpu_throughput_modes(samples, None, 0.1)
    assert "threads of one process" in sweep["how"] and best["proofs_per_s"] > 0
