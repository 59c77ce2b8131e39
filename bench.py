#!/usr/bin/env python3
"""bench.py -- BASELINE.json metric ("leaf proofs/sec (whole node) + NTT GB/s vs HBM peak, 2^20-row table build") on MI355X.

    python bench.py --gpus N --steps K --warmup W            (N > 1 without a launcher: starts its own N ranks)
    python bench.py --gpus N --steps K --warmup W --full     (the same headline, then every check and side leg below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Default workload (`--workload table`, run_table below): BASELINE configs[3] as ONE contiguous block of `--steps` x `--rows` table rows
per rank. A step is `--rows` rows, 1024 when `--rows` is not given, so that the timed work grows with `--steps`: `--steps 128` gives
every rank a 2^17-row block and `--gpus 8 --steps 128` builds the metric's whole 2^20-row table (8 blocks + 7 separator rows, three
join levels). The warm-up block is `--warmup` steps, at most 5120 rows. One work plan per block.

A plain run does what the headline needs and nothing else: set-up, warm-up, the timed block, `--dump-outputs DIR` if given (the
block root proof as .npy files, see dump_outputs), the JSON line. The self-check, the CPU baseline, the side legs and the kernel legs
described below run with `--full` only.
Per row the reference proves 4 cells-tree nodes and 1 row-tree node, each a framework proof (witness generation, base prove(),
wrap chain to 2^12 rows: recursion-framework/src/circuit_builder.rs:286-311, wrap_circuit.rs:122-148); here they are REAL
circuits with the reference's tree logic (mapreduce-plonky2_amd/table.py), their witnesses replayed on the device
(mp2g_witness_program_run_dev), the row tree scheduled by ryhope's batched work plan (mp2g_update_plan_*), the rows' multiset
digests computed inside the timed region. value = framework proofs per second (5 per row). With `--full` at N = 1 the same JSON line carries BASELINE's other single-GPU configurations:
`config2` = configs[2] at full size (1024 real leaf proofs aggregated 2-to-1: 2047 framework proofs), `by_base_degree` = the table
rate with every base circuit padded to 2^k rows, k = 12..15, and carrying the reference's leaf gate set (the
reference's real base degrees lie there), `leaves_prove_only` = round 2's headline (`--workload leaves`: prove() only, synthetic
circuits, resident witnesses), `roofline` = configs[1].

Self-check (`--full`). After the timed region: the block root's public inputs = the off-circuit tree hash / multiset digest / min / max and the
root passes the oracle's verifier; one framework proof of every circuit kind of the timed block is re-proved from its captured
witness by the CPU oracle -- caps, openings and FRI proof bit for bit, and accepted by its verifier (transcript, PLONK identity with
the gate terms, FRI). "verified": k counts those prove() calls; any mismatch makes the run fail. The oracle proofs of that leg are
the `cpu_baseline` sample at N=1 (plus 1-thread / all-thread medians of 5 on one fixed prove() call, CPU model printed).

Rows shard across ranks as blocks with no data-path collective ("scaling": "weak"); log2(N) join levels above the block roots
move one final proof each, device to device over RCCL. Before anything is timed every join pair moves a small libmp2gpu-allocated
buffer the same way (sharding.probe_handoff); if that fails anywhere, all levels use the staged hand-off (download + torch tensor)
and `config.sharding` says so.

The NTT half of the metric is the `roofline` object (`--full`): BASELINE configs[1]'s 2^22-point forward NTT, timed with HIP events on
the context's stream in this same run, algorithmic 16 B/point.

Other workloads: leaves (above), tree (synthetic circuits + aggregation levels), recursion (map-reduce trees of real proofs + the
final Poseidon wrap), ntt (the roofline leg alone, for rocprof).
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# the CPU oracle runs several OpenMP teams side by side (one per sampled leaf proof): idle team members must sleep,
# not spin, or the teams starve each other on a fully subscribed host. Read by libgomp when it is first loaded.
os.environ.setdefault("OMP_WAIT_POLICY", "passive")
os.environ.setdefault("GOMP_SPINCOUNT", "0")

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
LOG_NTT = 22
SEED = 0xC0FFEE03


_CLOCK_HELPER = r"""
import subprocess, sys
for line in sys.stdin:
    try:
        r = subprocess.run(["rocm-smi", "-d", line.strip(), "--showclocks", "--json"], capture_output=True, text=True, timeout=20)
        out = " ".join(r.stdout.split())
    except Exception as e:
        out = "error: " + str(e)[:80]
    print(out, flush=True)
"""


class ClockReader:
    """rocm-smi's current clocks of a device (state the measured clocks with every report). rocm-smi is run by a
    helper process started before this one touches the GPU: a process that has initialised the GPU must not fork + exec."""

    def __init__(self):
        import subprocess
        # under a counter-collecting profiler the preloaded library has initialised the GPU before this program's first line: no child
        # process may be started then (the pool's boxes refuse an exec after GPU initialisation)
        if "rocprofiler" in os.environ.get("LD_PRELOAD", "").lower() and os.environ.get("ROCPROF_COUNTER_COLLECTION", "0") not in ("", "0"):
            self.p = None
            return
        try:
            self.p = subprocess.Popen([sys.executable, "-c", _CLOCK_HELPER], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        except Exception:
            self.p = None

    def read(self, device):
        if self.p is None:
            return {"error": "no helper process"}
        try:
            self.p.stdin.write(f"{device}\n")
            self.p.stdin.flush()
            line = self.p.stdout.readline()
            card = next(iter(json.loads(line).values()))
            return {k.strip(): v for k, v in card.items() if "clock" in k.lower() and ("sclk" in k.lower() or "mclk" in k.lower() or "fclk" in k.lower())}
        except Exception as e:  # no rocm-smi / no permission: say so instead of guessing
            return {"error": str(e)[:80]}

    def close(self):
        if self.p is not None:
            try:
                self.p.stdin.close()
                self.p.wait(timeout=5)
            except Exception:
                self.p.kill()
            self.p = None


class NoClocks:
    """a plain run of the table workload reads no clocks: ClockReader's helper process is started for `--full` and the other workloads"""

    def read(self, device):
        return None

    def close(self):
        pass


class CpuFarm:
    """The CPU baseline's THROUGHPUT modes run as separate PROCESSES: one address space per proof, so that nothing the proofs share
    inside one process (the memory map, the allocator, the OpenMP runtime) can be what limits them. (It is not: 256 oracle proofs
    side by side do 1.5 proofs/s as threads and as processes -- profiles/r06/cpu_throughput_modes.json: the host's memory system.)
    A process that has initialised the GPU must not fork + exec, so the farm's parent is a helper started before this process
    touches the GPU (like ClockReader); it gets its jobs over a pipe and starts the workers itself."""

    def __init__(self):
        import subprocess
        if "rocprofiler" in os.environ.get("LD_PRELOAD", "").lower():
            self.p = None
            return
        try:
            self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-farm"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        except Exception:
            self.p = None

    def run(self, spool, modes, seconds):
        """modes [(P processes, T threads each)] over the spooled samples; returns the farm's list of mode dicts (or raises)"""
        self.p.stdin.write(json.dumps({"spool": spool, "modes": modes, "seconds": seconds, "orc_lib": os.environ.get("ORC_LIB", "")}) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the CPU farm's helper process ended")
        return json.loads(line)

    def close(self):
        if self.p is not None:
            try:
                self.p.stdin.close()
                self.p.wait(timeout=10)
            except Exception:
                self.p.kill()
            self.p = None


def spool_samples(samples, path):
    """the captured prove() calls of the sampled framework proofs as files a worker process maps: per prove() its preprocessed
    polynomials and wires (.npy), in meta.json its shape, gate table, oracle parameters, digest, public-inputs hash; `cycle` = the
    order in which framework proofs are pulled (the table's proportion: per two rows 2 x 4 cells proofs, a row leaf, a row full node)"""
    os.makedirs(path, exist_ok=True)
    kind = lambda chain: chain[0][0].rsplit(" step", 1)[0]
    cells = [i for i, c in enumerate(samples) if kind(c).startswith("cells")]
    leaf = [i for i, c in enumerate(samples) if kind(c) == "row_leaf"] or [i for i, c in enumerate(samples) if kind(c).startswith("row")][:1]
    full = [i for i, c in enumerate(samples) if kind(c) == "row_full"] or leaf
    cycle = (cells + leaf[:1] + cells + full[:1]) if cells else list(range(len(samples)))
    meta, k = {"cycle": cycle, "proofs": []}, 0
    for chain in samples:
        steps = []
        for label, ckt, ofp, cd, make_wires, ph, *_ in chain:
            np.save(os.path.join(path, f"p{k}_pre.npy"), np.ascontiguousarray(ckt.pre, dtype=np.uint64))
            np.save(os.path.join(path, f"p{k}_wires.npy"), np.ascontiguousarray(make_wires(), dtype=np.uint64))
            steps.append({"k": k, "label": label, "log_n": int(ckt.log_n), "num_selectors": int(ckt.num_selectors), "num_constants": int(ckt.num_constants),
                          "gates": [[int(g.kind), int(g.p0), int(g.p1), int(g.p2), int(g.selector_index), int(g.group_start), int(g.group_end)] for g in ckt.gates],
                          "fp": bytes(ofp).hex(), "cd": [int(x) for x in cd], "ph": [int(x) for x in ph]})
            k += 1
        meta["proofs"].append(steps)
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump(meta, f)
    return path


def cpu_farm_worker(argv):
    """bench.py --cpu-farm-worker SPOOL IDX P SECONDS: one slot of a throughput mode (OMP_NUM_THREADS is set by the farm). Loads the
    oracle and the spooled samples, says `ready`, waits for `go`, proves framework proofs IDX, IDX + P, ... of the cycle until SECONDS
    have passed (at least one), prints how many and how long."""
    spool, idx, P_, seconds = argv[0], int(argv[1]), int(argv[2]), float(argv[3])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits as OC
    import oracle as O
    mp2 = importlib.import_module("mapreduce-plonky2_amd")  # the ctypes structure of a gate descriptor; the GPU library is never loaded here
    with open(os.path.join(spool, "meta.json")) as f:
        meta = json.load(f)

    class Ckt:
        pass
    proofs = []
    for steps in meta["proofs"]:
        chain = []
        for st in steps:
            c = Ckt()
            c.pre = np.load(os.path.join(spool, f"p{st['k']}_pre.npy"), mmap_mode="c")
            c.log_n, c.num_selectors, c.num_constants, c.luts = st["log_n"], st["num_selectors"], st["num_constants"], None
            c.gates = [mp2.Gate(*g) for g in st["gates"]]
            c.gate_array = (mp2.Gate * len(c.gates))(*c.gates)
            fp = O.FriParams.from_buffer_copy(bytes.fromhex(st["fp"]))
            chain.append((c, fp, np.array(st["cd"], dtype=np.uint64), np.load(os.path.join(spool, f"p{st['k']}_wires.npy"), mmap_mode="c"), np.array(st["ph"], dtype=np.uint64)))
        proofs.append(chain)
    O.lib()
    cycle = meta["cycle"]
    print("ready", flush=True)
    sys.stdin.readline()
    t0, done, j = time.perf_counter(), 0, idx
    while True:
        for c, fp, cd, wires, ph in proofs[cycle[j % len(cycle)]]:
            OC.prove_witness(c, fp, cd, wires, ph)
        done += 1
        j += P_
        if time.perf_counter() - t0 > seconds:
            break
    print(json.dumps({"done": done, "seconds": time.perf_counter() - t0}), flush=True)
    return 0


def cpu_farm_main():
    """bench.py --cpu-farm: the helper behind CpuFarm. One JSON job per input line; per mode (P, T): P worker processes with
    OMP_NUM_THREADS = T, released together once all are ready; value = framework proofs completed / time from the release to the last
    worker's end. Answers one JSON line per job."""
    import subprocess
    for line in sys.stdin:
        try:
            job = json.loads(line)
            out = []
            for P_, T_ in job["modes"]:
                env = dict(os.environ, OMP_NUM_THREADS=str(T_), OMP_WAIT_POLICY="passive", GOMP_SPINCOUNT="0")
                if job.get("orc_lib"):
                    env["ORC_LIB"] = job["orc_lib"]
                ws = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-farm-worker", job["spool"], str(i), str(P_), str(job["seconds"])],
                                       stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env) for i in range(P_)]
                ok = [w.stdout.readline().strip() == "ready" for w in ws]
                t0 = time.perf_counter()
                for w in ws:
                    try:
                        w.stdin.write("go\n")
                        w.stdin.flush()
                    except Exception:
                        pass
                done, failed = 0, ok.count(False)
                for w in ws:
                    res = w.stdout.readline()
                    try:
                        done += json.loads(res)["done"]
                    except Exception:
                        failed += 1
                    w.wait()
                wall = time.perf_counter() - t0
                out.append({"mode": f"{P_} processes x {T_} thread(s) each", "concurrent_proofs": P_, "threads_per_proof": T_, "framework_proofs": done,
                            "wall_s": round(wall, 2), "proofs_per_s": done / wall, "workers_failed": failed})
            print(json.dumps(out), flush=True)
        except Exception as e:
            print(json.dumps({"error": f"{type(e).__name__}: {e}"[:300]}), flush=True)
    return 0


def check_against_oracle(samples, budget_s, timed, ranks_on_host=1):
    """The checker leg (and, at N=1, the `cpu_baseline` sample): the CPU oracle proves the witnesses of the sampled
    GPU proofs -- leaf proof = one base + one wrap prove() -- `groups` leaf proofs at a time with cores/groups
    OpenMP threads each, until every mandatory sample is done and, when `timed`, ~budget_s seconds are spent.
    samples: list of leaf proofs, each a list of (label, ckt, ofp, circuit_digest, make_wires, pi_hash, gpu_caps,
    gpu_openings, gpu_proof, mandatory), mandatory ones first. Returns (n_verified, baseline dict or None); raises on any mismatch."""
    import threading
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits as OC  # oracle-side prove / verify of a built circuit (tests/circuits.py)
    import oracle as O
    cores = max(1, (os.cpu_count() or 1) // max(1, ranks_on_host))  # every rank of the node checks its own proofs at the same time
    groups = max(1, min(len(samples), cores // 32))
    per_group = max(1, cores // groups)
    omp = ctypes.CDLL("libgomp.so.1")
    errors, verified = [], [0]
    lock = threading.Lock()

    def one_leaf(parts):
        omp.omp_set_num_threads(per_group)  # per-thread ICV: the parallel regions this thread opens
        for label, ckt, ofp, cd, make_wires, ph, g_caps, g_open, g_proof, _ in parts:
            caps, openings, proof, _ = OC.prove_witness(ckt, ofp, cd, make_wires(), ph)
            ok = np.array_equal(caps, g_caps) and np.array_equal(openings, g_open) and np.array_equal(proof, g_proof)
            rc = OC.verify(ckt, ofp, cd, ph, g_caps, g_open, g_proof)
            with lock:
                if not ok:
                    errors.append(f"{label}: GPU proof differs from the oracle's proof of the same witness")
                elif rc:
                    errors.append(f"{label}: the oracle's verifier rejects the GPU proof (code {rc})")
                else:
                    verified[0] += 1

    t_total, n_leaf, i = 0.0, 0, 0
    n_mand = sum(1 for s in samples if s[0][-1])
    while i < len(samples):
        if i >= n_mand and (not timed or t_total * (n_leaf + groups) / max(n_leaf, 1) > budget_s):
            break
        part = samples[i:i + groups]
        ts = [threading.Thread(target=one_leaf, args=(s,)) for s in part]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        t_total += time.perf_counter() - t0
        n_leaf += len(part)
        i += len(part)
    if errors:
        raise SystemExit("bench.py self-check FAILED:\n  " + "\n  ".join(errors))
    base = None
    if timed and n_leaf:
        base = {"value": n_leaf / t_total, "unit": "leaf proofs/s", "cores": cores, "kind": "port",
                "single_leaf_latency_s": t_total / ((n_leaf + groups - 1) // groups),
                "sample": f"{n_leaf} leaf proof(s) = base + wrap prove() of the sampled GPU witnesses by oracle/ (our C restatement, not the "
                          f"Rust prover), {groups} at a time with {per_group} OpenMP threads each; every one compared bit for bit with the GPU's"}
    return verified[0], base


def run_tree(args, rank, local_rank, world, dist, torch, VARIANT):
    """--workload tree: BASELINE configs[2]/[3] shaped map-reduce. Per step every rank proves the subtree over its
    `--batch` leaves bottom-up (framework.MapReduce: base 2^13 + wrap 2^12 per node, public-input chain of
    recursion-framework/tests/integration.rs:108-127), then the log2(world) levels above the shard boundary: the rank
    that owns a parent (sharding.tree_handoff_plan: the owner of its first leaf) receives the other child's final proof
    -- caps, openings, FRI proof and public inputs as device tensors over RCCL, no host copy -- and proves the parent
    from the two children's public inputs. value = leaf proofs per second with all aggregation proving inside the timed
    region. (The circuits are the synthetic gate-level ones of the headline workload: a parent's witness depends on its
    children through the public-input chain only; recursion.py holds the real verifier circuits.)"""
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    sharding = importlib.import_module("mapreduce-plonky2_amd.sharding")
    FW = importlib.import_module("mapreduce-plonky2_amd.framework")
    assert world & (world - 1) == 0 and args.batch & (args.batch - 1) == 0, "powers of two"
    ctx0, ctx1 = mp2.Context(local_rank), mp2.Context(local_rank)
    B = args.batch
    mr = FW.MapReduce(ctx0, ctx1, B, chunk=min(128, B), variant=VARIANT, seed=SEED, base_bits=args.base_bits, data_seed=SEED + 977 * rank)
    top = FW.FrameworkProver(ctx0, ctx1, 1, variant=VARIANT, seed=SEED, circuits=(mr.fw.base_ckt, mr.fw.wrap_ckt))
    nccl = dist is not None and dist.get_backend() == "nccl"
    dev = torch.device("cuda", local_rank) if nccl else None
    wp = top.wrap
    fp = wp.fp
    sizes = [fp.n_oracles * fp.cap_words, fp.n_openings * 2, fp.proof_words, FW.NUM_PUBLIC_INPUTS + 4]
    n_levels = world.bit_length() - 1
    moved = [0]

    def step():
        root = mr.run(keep=lambda level, index: False)  # the subtree of this rank; its root node was proved by a 2-wide or wider prover
        pv = mr.prover_for(1)
        pis = root
        holder = pv.wrap  # the CircuitProver whose device outputs hold this rank's current root proof (slot 0)
        for lvl in range(n_levels):
            bit = 1 << lvl
            if rank & (bit - 1):
                break  # handed its subtree over at a lower level
            if rank & bit:
                dst = rank - bit
                d_pis = ctx1.to_device(pis)
                bufs = (holder.pr.d_caps, holder.pr.d_openings, holder.pr.d_proof, d_pis)
                if nccl:
                    ctx1.sync()
                    parts = [sharding.device_words(b, 0, n, dev) for b, n in zip(bufs, sizes)]
                else:
                    parts = [torch.from_numpy(b.download((n,)).view(np.int64)) for b, n in zip(bufs, sizes)]
                sharding.send_proof_words(dist, parts, dst, dev)
                moved[0] += sum(sizes) * 8
                break
            got = sharding.recv_proof_words(dist, sizes, rank + bit, dev)
            child = got[3].cpu().numpy().view(np.uint64)
            # the parent's public inputs (ReduceCircuitWires): sum of the sums, hash of the hashes; same circuit set
            assert np.array_equal(child[FW.NUM_PUBLIC_INPUTS:], pis[FW.NUM_PUBLIC_INPUTS:]), "children of different circuit sets"
            own = FW.MapReduce.reduce_public_inputs(ctx0, np.stack([pis[:FW.NUM_PUBLIC_INPUTS], child[:FW.NUM_PUBLIC_INPUTS]]), VARIANT)[0]
            pis = np.concatenate([own, pis[FW.NUM_PUBLIC_INPUTS:]])
            top.generate_proofs(ctx0.hash_no_pad_batch(pis[None], 4, VARIANT))
            holder = top.wrap
        ctx0.sync(); ctx1.sync()
        return pis

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        ctx0.sync(); ctx1.sync()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        root_pis = step()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device="cuda" if nccl else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    out = None
    if rank == 0:
        # the root's public inputs are the whole dataset's: sum of the even elements of every rank's data, hash chain of the hashes
        total_even, hs = 0, []
        for r in range(world):
            data = importlib.import_module("mapreduce-plonky2_amd.circuits").rand_field(B * FW.INPUT_CHUNK_SIZE, SEED + 977 * r)
            total_even = (total_even + sum(int(x) for x in data if int(x) % 2 == 0)) % ((1 << 64) - (1 << 32) + 1)
        assert int(root_pis[0]) == total_even, "root sum != sum of the even elements of the dataset"
        n_nodes = world * (2 * B - 1) + (world - 1)
        out = {"metric": "leaf proofs/sec (whole node) + NTT GB/s vs HBM peak, 2^20-row table build, 1/2/4/8 GPU",
               "value": world * B * args.steps / dt, "unit": "leaf proofs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "u64 (Goldilocks field)", "data": "synthetic",
               "framework_proofs_per_s": n_nodes * args.steps / dt,
               "config": {"workload": f"tree: {world} x {B} leaf proofs and the {n_nodes - world * B} aggregation nodes above them per step (each node = base "
                                      f"2^{args.base_bits} + wrap 2^12 prove()); {n_levels} level(s) cross ranks by send/recv of the child's final proof "
                                      f"({sum(sizes) * 8} B, {'device tensors over RCCL' if nccl else 'host tensors over gloo'})",
                          "batch_per_rank": B, "hasher": "Poseidon2" if VARIANT == 0 else "Poseidon", "root_public_inputs": [int(x) for x in root_pis]}}
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()
    mr.free(); top.free()
    ctx1.close(); ctx0.close()
    return out


def run_recursion(args, rank, local_rank, world, dist, torch, VARIANT):
    """--workload recursion: a map-reduce tree of REAL framework proofs per step and rank (recursion.py): `--batch` map
    proofs (MapCircuit of integration.rs:65-93: base 2^6 rows + wrap to the shared 2^12-row shape, RECURSION_THRESHOLD) and the
    batch - 1 reduce proofs above them (two universal verifiers + the reduce logic: base 2^13 rows + wrap 2^12), level by level. Everything
    generate_proof does is inside the timed region: witness generation (mp2g_witness_program_run on the host's threads),
    upload, prove() with the device-side witness check, download of the proofs the next level verifies. With several
    ranks the tree continues above the shard boundary: log2(world) levels in which the owner of a parent receives the
    other child's final proof -- the word ranges of the sender's prover outputs as device tensors over RCCL, copied on the
    device into the parent's witness inputs (recursion.DeviceProof; host tensors over gloo) -- and proves the reduce node
    whose universal verifiers check both children in-circuit."""
    assert VARIANT == 0, "the recursive verifier circuit of recursion.py hashes with Poseidon2 gates (the reference's default config)"
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    R = importlib.import_module("mapreduce-plonky2_amd.recursion")
    FW = importlib.import_module("mapreduce-plonky2_amd.framework")
    C = importlib.import_module("mapreduce-plonky2_amd.circuits")
    import threading
    ctx = mp2.Context(local_rank)
    prover = FW.GpuProver(ctx, VARIANT, witness_check=True, device_witness=not args.host_witness)
    fw = R.RecursiveCircuits([R.FrameworkCircuit("map", 0, R.map_logic, 5), R.FrameworkCircuit("reduce", 2, R.reduce_logic, 5)], prover,
                             lambda ckt: FW.circuit_fri_params(ckt, VARIANT))
    n_leaves = args.batch
    assert n_leaves & (n_leaves - 1) == 0
    # --trees independent trees per rank and step (the reference's independent rows / blocks), one host thread, GPU context and
    # prover each: one tree's witness programs run on the host while another's prove() occupies the GPU
    n_trees = max(1, args.trees)
    ctxs = [ctx] + [mp2.Context(local_rank) for _ in range(n_trees - 1)]
    provers = [prover] + [FW.GpuProver(c, VARIANT, witness_check=True, device_witness=not args.host_witness) for c in ctxs[1:]]
    sessions = [R.ProofSession(p) for p in provers]
    for name in ("map", "reduce"):
        fw.witness_programs(name)  # shared and read-only from here on
    datas = [C.rand_field(4 * n_leaves, SEED + 31 * rank + 7919 * t) for t in range(n_trees)]
    # the host's threads are shared by the trees in flight (and by the ranks of the node): a tree's witness programs run one proof
    # per thread and, where a level has fewer proofs than that, the parallel regions of each proof on the spare ones
    host_threads = max(1, (os.cpu_count() or 1) // (n_trees * int(os.environ.get("LOCAL_WORLD_SIZE", world))))

    sharding = importlib.import_module("mapreduce-plonky2_amd.sharding")
    nccl = dist is not None and dist.get_backend() == "nccl"
    dev = torch.device("cuda", local_rank) if nccl else None
    final_ckt = fw.chains["reduce"][-1][0]          # every final proof has this shape (the shared common data)
    final_fp = FW.circuit_fri_params(final_ckt, VARIANT)
    n_pis = 5 + 4

    def local_tree(t, out):
        sess, data = sessions[t], datas[t]
        level = fw.generate_proofs_batch("map", [([], [], data[4 * i:4 * i + 4]) for i in range(n_leaves)], threads=host_threads, session=sess)
        names = ["map"] * n_leaves
        while len(level) > 1:
            level = fw.generate_proofs_batch("reduce", [([level[2 * i], level[2 * i + 1]], [names[2 * i], names[2 * i + 1]], None)
                                                       for i in range(len(level) // 2)], threads=host_threads, session=sess)
            names = ["reduce"] * len(level)
        out[t] = (level[0], names[0])

    # the proof that leaves the framework: verifiable-db/src/api.rs:148-214, a PoseidonGoldilocksConfig circuit verifying the root
    wrap_prover = FW.GpuProver(ctx, mp2.POSEIDON, witness_check=True, device_witness=not args.host_witness)
    fin = R.FinalWrapCircuit(fw, wrap_prover, lambda ckt: FW.circuit_fri_params(ckt, mp2.POSEIDON))
    fin.program()

    def step():
        roots = tree_roots()
        if rank == 0:  # the last step of the pipeline: the final Poseidon wrap of every tree's root
            final[:] = fin.generate_proofs_batch(roots, ["reduce" if (n_leaves > 1 or world > 1) else "map"] * len(roots))
        return roots

    final = []

    def tree_roots():
        local = [None] * n_trees
        if n_trees == 1:
            local_tree(0, local)
        else:
            ths = [threading.Thread(target=local_tree, args=(t, local)) for t in range(n_trees)]
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            if any(r is None for r in local):
                raise SystemExit("bench.py: a tree thread failed")
        return [above_shards(*local[t], t=t) for t in range(n_trees)]

    proof_sizes = [n_pis, 3 * final_fp.cap_words, final_fp.n_openings * 2, final_fp.proof_words]

    def above_shards(root, root_name, t=0):
        sess = sessions[t]
        for lvl in range(world.bit_length() - 1):  # above the shard boundary
            bit = 1 << lvl
            if rank & (bit - 1):
                break
            if rank & bit:
                # the root proof leaves from the prover's output buffers (device tensors over RCCL; mp2g_proof_serialize is the
                # wire format for hosts that store proofs, mp2-common/src/proof.rs:42-57 -- not needed between GPUs)
                tag = torch.tensor([0 if root_name == "map" else 1], dtype=torch.int64)
                dist.send(tag.to(dev) if nccl else tag, rank - bit)
                sharding.send_device_proof(dist, sess.prover.ctx, sess.prover.last_device_proof(0), rank - bit, dev)
                break
            tag = torch.zeros(1, dtype=torch.int64, device=dev)
            dist.recv(tag, rank + bit)
            child = sharding.recv_device_proof(dist, proof_sizes, rank + bit, dev)
            (root,) = fw.generate_proofs_batch("reduce", [([root, child], [root_name, "map" if int(tag.item()) == 0 else "reduce"], None)], session=sess)
            root_name = "reduce"
        return root

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        for c in ctxs:
            c.sync()

    for _ in range(max(1, args.warmup)):  # the first pass creates the provers of every level width
        roots = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        roots = step()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device="cuda" if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    pis = roots[0][3]
    if rank == 0:
        for t in range(n_trees):
            want = 0
            for r in range(world):
                want = (want + sum(int(x) for x in C.rand_field(4 * n_leaves, SEED + 31 * r + 7919 * t) if int(x) % 2 == 0)) % C.P
            assert int(roots[t][3][0]) == want, "root sum != sum of the even elements of every rank's data"
    out = None
    if rank == 0:
        n_nodes = 2 * n_leaves - 1
        out = {"metric": "leaf proofs/sec (whole node) + NTT GB/s vs HBM peak, 2^20-row table build, 1/2/4/8 GPU",
               "value": world * n_trees * n_leaves * args.steps / dt, "unit": "leaf proofs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "u64 (Goldilocks field)", "data": "synthetic",
               "framework_proofs_per_s": n_trees * (world * n_nodes + world - 1 + 1) * args.steps / dt,
               "final_wrap": {"circuit": "PoseidonGoldilocksConfig wrap of every root (verifiable-db/src/api.rs:148-214), variant = Poseidon prove()", "rows_log2": fin.ckt.log_n,
                              "public_inputs": [int(x) for x in final[0][3]]},
               "config": {"workload": f"recursion: per rank {n_trees} independent {n_leaves}-leaf map-reduce tree(s) of REAL framework proofs, one host thread and GPU stream each ({n_nodes} per tree = map: base 2^6 + wrap 2^12 "
                                      "rows; reduce: two universal verifiers, base 2^13 + wrap 2^12 rows), witness generation " + ("on the host threads, " if args.host_witness else "on the device (level-scheduled witness programs), ") +
                                      "witness check on, every level inside the timed region",
                          "shapes": {k: [c[0].log_n for c in v] for k, v in fw.chains.items()}, "host_threads": os.cpu_count(),
                          "hasher": "Poseidon2" if VARIANT == 0 else "Poseidon", "root_public_inputs": [int(x) for x in pis]}}
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()
    wrap_prover.free()
    for p in provers:
        p.free()
    for c in ctxs:
        c.close()
    return out


def run_ntt_leg(args, local_rank, clocks):
    """--workload ntt: the roofline leg alone -- `--steps` forward 2^22-point NTTs (bit-reversed output), HIP events on the stream
    around each -- so that a `rocprofv3 --kernel-trace --stats` of this command holds nothing but the kernels `roofline` is about
    (their average durations there must add up to `launch_ms` minus the gap between the two launches)."""
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    C = importlib.import_module("mapreduce-plonky2_amd.circuits")
    ctx = mp2.Context(local_rank)
    n = 1 << LOG_NTT
    d_poly = ctx.to_device(C.rand_field((1, n), 0xC0FFEE02))
    d_out = ctx.alloc(n * 8)
    for _ in range(max(1, args.warmup)):
        ctx.ntt_dev(d_poly, d_out, LOG_NTT, 1, bitrev_out=True)
    ms = []
    for _ in range(args.steps):
        ctx.timer_start()
        ctx.ntt_dev(d_poly, d_out, LOG_NTT, 1, bitrev_out=True)
        ms.append(ctx.timer_stop())
    t = float(np.median(ms)) / 1e3
    out = {"metric": "leaf proofs/sec (whole node) + NTT GB/s vs HBM peak, 2^20-row table build, 1/2/4/8 GPU", "value": None, "unit": "leaf proofs/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "data": "synthetic", "dtype": "u64 (Goldilocks field)",
           "config": {"workload": "ntt: the roofline leg alone (2^22-point forward NTT, bit-reversed output); no proofs are made, `value` is null"},
           "roofline": {"bound": "hbm", "kernel": "ntt (2^22 forward, all launches)", "achieved": 16.0 * n / t / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": 16.0 * n / t / 1e9 / HBM_PEAK_GBPS, "launch_ms": t * 1e3, "algorithmic_bytes": 16 * n},
           "clocks": clocks.read(local_rank)}
    print(json.dumps(out))
    ctx.close()
    return out


def kernel_legs(ctx, mp2, C, VARIANT, hasher, rank=0):
    """the kernel-level half of the metric, measured in the same process as the proving loop: the `roofline` object (configs[1]'s
    2^22-point forward NTT, HIP events on the stream the kernels run on, algorithmic 16 B / point), the batched 2^12 shape the
    prover runs, and the sponge rate. Returns the three JSON objects."""
    n_ntt = 1 << LOG_NTT
    d_poly = ctx.to_device(C.rand_field((1, n_ntt), 0xC0FFEE02 + rank))
    d_out = ctx.alloc(n_ntt * 8)
    # roofline leg: the 2^22 NTT, HIP events on the stream the kernels are launched on. 1000 untimed transforms first: the leg is
    # 55-60 us long and follows the clocks, which need tens of ms of this kernel to settle after the prover's steps (tools/dbg/ntt_leg_burst.sh:
    # 61 / 58 / 55 us as the median of 20 / 200 / 1000 back-to-back transforms); then 50 timed ones, each between its own events
    for _ in range(1000):
        ctx.ntt_dev(d_poly, d_out, LOG_NTT, 1, bitrev_out=True)
    ntt_ms = []
    for _ in range(50):
        ctx.timer_start()
        ctx.ntt_dev(d_poly, d_out, LOG_NTT, 1, bitrev_out=True)
        ntt_ms.append(ctx.timer_stop())

    def median_ms(fn, runs=7):
        """one untimed call, then the median of `runs` calls, each between its own HIP events on the context's stream"""
        fn()
        ms = []
        for _ in range(runs):
            ctx.timer_start()
            fn()
            ms.append(ctx.timer_stop())
        return float(np.median(ms)), [round(x, 4) for x in ms]

    # the same kernel family on the shape the prover actually runs: 8192 transforms of 2^12 points
    # (LDE-sized batch, no tail effects); reported beside the roofline leg, not as `value`
    nb12 = 8192
    d_b12 = ctx.alloc(nb12 * 4096 * 8)
    ntt12_ms, ntt12_all = median_ms(lambda: ctx.ntt_dev(d_b12, d_b12, 12, nb12, bitrev_out=True))
    d_b12.free()

    # the sponge, the kernel that takes half of a step: 2^21 leaves of 136 limbs (17 permutations each), the rate
    # of the instruction-bound Poseidon2 permutation; reported beside the roofline leg
    n_hash, limbs = 1 << 21, 136
    d_hin = ctx.alloc(n_hash * limbs * 8)
    d_hout = ctx.alloc(n_hash * 4 * 8)
    # random field elements, not a zero buffer: the permutation's power draw (and with it the clock) depends on its data
    # (tools/dbg/sponge_ab.py: zeros hash 4.5 % faster)
    part = C.rand_field((1 << 17, limbs), 0xC0FFEE05 + rank)
    for k in range(n_hash >> 17):
        d_hin.upload_at(part, k * part.nbytes)
    hargs = (ctx.h, VARIANT, d_hin.ptr, limbs, n_hash, 4, d_hout.ptr)
    hash_ms, hash_all = median_ms(lambda: mp2._ck(mp2.load().mp2g_hash_no_pad_batch_dev(*hargs)))
    d_hin.free(); d_hout.free()

    # BASELINE configs[1](ii): PolynomialBatch::from_values of 135 polynomials of 2^15 values --
    # iNTT, LDE to 2^18 leaves x 135 (72 n w algorithmic bytes), Poseidon2 leaf sponges + tree levels to cap(4)
    # (L ceil(w / 8) + L - 2^cap permutations) -- on resident values; the parts timed apart with the same buffers
    lg, w135 = 15, 135
    n15, L = 1 << lg, 1 << (lg + 3)
    d_v = ctx.to_device(C.rand_field((w135, n15), 0xC0FFEE02 + 16 * rank))
    d_c = ctx.alloc(w135 * n15 * 8)
    d_lde = ctx.alloc(w135 * L * 8)
    pb = mp2.PolynomialBatch.from_values_dev(ctx, d_v, lg, w135, 3, 4, VARIANT)
    commit_ms, commit_all = median_ms(lambda: pb.recommit_from_values_dev(d_v), 5)
    intt_ms, _ = median_ms(lambda: ctx.ntt_dev(d_v, d_c, lg, w135, inverse=True), 5)
    lde_ms, lde_all = median_ms(lambda: ctx.lde_dev(d_c, lg, w135, 3, d_lde), 5)
    # the two halves of the Merkle part by themselves, over the LDE values the batch holds (mp2g_batch_rehash_dev)
    leafk_ms, _ = median_ms(lambda: pb.rehash_dev(1), 5)
    levels_ms, _ = median_ms(lambda: pb.rehash_dev(2), 5)
    pb.free(); d_v.free(); d_c.free(); d_lde.free()
    # the leaf sponge kernel ALONE at the size of the counter pass (profiles/r05/sponge_counters.json: 2^20 leaves x 135 limbs =
    # 17 permutations per lane): what `roofline_alu.isolated` is about -- the same kernel its instruction count was taken from
    lg17 = 17
    d_v17 = ctx.alloc(w135 * (1 << lg17) * 8)
    for k in range(w135 * (1 << lg17) * 8 // part.nbytes + 1):
        nb = min(part.nbytes, w135 * (1 << lg17) * 8 - k * part.nbytes)
        if nb > 0:
            d_v17.upload_at(part.reshape(-1)[:nb // 8], k * part.nbytes)
    pb17 = mp2.PolynomialBatch.from_values_dev(ctx, d_v17, lg17, w135, 3, 4, VARIANT)
    leaf17_ms, leaf17_all = median_ms(lambda: pb17.rehash_dev(1), 7)
    pb17.free(); d_v17.free()
    leaf_kernel_rate = (1 << (lg17 + 3)) * ((w135 + 7) // 8) / (leaf17_ms / 1e3)
    perms = L * ((w135 + 7) // 8) + L - 16
    merkle_ms = max(commit_ms - intt_ms - lde_ms, 1e-6)
    commit = {"workload": "configs[1](ii): PolynomialBatch::from_values of 135 x 2^15 resident values -> iNTT, LDE to 2^18 leaves x 135, Poseidon2 leaf sponges and tree "
                          "levels to cap(4); medians of 5 launches between HIP events", "seconds": commit_ms / 1e3, "runs_ms": commit_all,
              "intt_ms": intt_ms, "lde_ms": lde_ms, "lde_GBps": 72.0 * n15 * w135 / (lde_ms / 1e3) / 1e9, "lde_frac_of_hbm_peak": 72.0 * n15 * w135 / (lde_ms / 1e3) / 1e9 / HBM_PEAK_GBPS,
              "merkle_ms": merkle_ms, "merkle_permutations": perms, "merkle_permutations_per_s": perms / (merkle_ms / 1e3),
              "merkle_note": "merkle_ms = commit - iNTT - LDE (the same launches timed apart); 17 of 18 permutations are the leaf sponge's (leaf_hash_poly_major_kernel)",
              "leaf_sponge_ms": leafk_ms, "tree_levels_ms": levels_ms,
              "leaf_sponge_permutations_per_s": L * ((w135 + 7) // 8) / (leafk_ms / 1e3), "tree_levels_permutations_per_s": (L - 16) / (levels_ms / 1e3),
              "parts_note": "leaf_sponge_ms / tree_levels_ms: the two halves of MerkleTree::new by themselves over the resident LDE values (mp2g_batch_rehash_dev), medians of 5"}

    d_poly.free(); d_out.free()
    # HBM-side bytes of the same two launches from the TCC counters (collected in separate
    # --pmc passes and corrected as MI355X_MICROARCH.md prescribes; profiles/rNN/ntt_traffic.json)
    traffic, traffic_source = None, None
    for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
        try:
            with open(os.path.join(ROOT, "profiles", rnd, "ntt_traffic.json")) as f:
                traffic = json.load(f)["ntt_2p22_forward_bitrev"]["traffic_bytes"]
            traffic_source = f"profiles/{rnd}/ntt_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/dbg/traffic_run.py, committed; NOT measured in this run)"
            break
        except (OSError, KeyError, ValueError):
            pass
    ntt_s = float(np.median(ntt_ms)) / 1e3
    achieved = 16.0 * n_ntt / ntt_s / 1e9
    sponge_rate = n_hash * (limbs // 8) / (hash_ms / 1e3)
    out = {"roofline": {"bound": "hbm", "kernel": "ntt (2^22 forward, all launches)",
                        "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_source,
                        "launch_ms": ntt_s * 1e3, "algorithmic_bytes": 16 * n_ntt},
           "ntt_batched_2p12": {"transforms": nb12, "GBps": 16.0 * nb12 * 4096 / (ntt12_ms / 1e3) / 1e9,
                                "frac_of_hbm_peak": 16.0 * nb12 * 4096 / (ntt12_ms / 1e3) / 1e9 / HBM_PEAK_GBPS, "median_of": len(ntt12_all), "runs_ms": ntt12_all},
           "sponge": {"hasher": hasher, "permutations_per_s": sponge_rate, "bound": "VALU issue (integer ALU)", "median_of": len(hash_all), "runs_ms": hash_all,
                      "input": f"{n_hash} x {limbs} limbs of random field elements, hash_no_pad, resident"},
           "commit_135x2p15": commit}
    # the 2^22 NTT against the OTHER roof as well: VALU instructions per point from the committed counter pass
    # x this run's transforms per second, over the VALU issue peak
    for rnd in ("r04", "r03"):
        try:
            with open(os.path.join(ROOT, "profiles", rnd, "ntt_traffic.json")) as f:
                kk = json.load(f)["kernels"]
            insts = sum(v["SQ_INSTS_VALU"] for name, v in kk.items() if name.startswith("void mp2g::ntt_cols_v2_kernel") or name.startswith("void mp2g::ntt_rows_v2_kernel"))
            peak = None
            for rnd2 in ("r06", "r05"):
                try:
                    with open(os.path.join(ROOT, "profiles", rnd2, "sponge_counters.json")) as f:
                        peak = json.load(f)["peak_valu_wave_insts_per_s"]
                    break
                except (OSError, KeyError, ValueError):
                    pass
            if peak is None:
                raise KeyError("no sponge_counters.json")
            out["roofline"]["valu"] = {"valu_insts_per_point": insts * 64.0 / n_ntt, "valu_wave_insts_per_launch": insts, "valu_wave_insts_per_s": insts / ntt_s,
                                       "peak_valu_wave_insts_per_s": peak, "frac_of_valu_peak": insts / ntt_s / peak,
                                       "reading": "the transform sits at `frac` of the HBM roof and at `frac_of_valu_peak` of the VALU issue roof: bound by neither (DESIGN.md section 4: one generation of tiles, "
                                                  "load / butterfly / store phases that cannot overlap)",
                                       "source": f"profiles/{rnd}/ntt_traffic.json (SQ_INSTS_VALU of the two launches, committed rocprofv3 --pmc pass; the kernels are unchanged since) x this run's launch time"}
            break
        except (OSError, KeyError, ValueError):
            pass
    alu = roofline_alu(leaf_kernel_rate, commit["merkle_permutations_per_s"], sponge_rate, leaf17_all)
    if alu is not None:
        out["roofline_alu"] = alu
    return out


def roofline_alu(isolated_rate, commit_rate, row_major_rate=None, isolated_runs_ms=None):
    """the ALU roofline of the kernel that dominates a step (the Poseidon2 leaf sponge: ~40 % of the kernel time of a table build).
    Clock-free quantities come from committed rocprofv3 --pmc passes (profiles/rNN/sponge_counters.json): VALU instructions per
    permutation (SQ_INSTS_VALU / permutations) and the shader cycles the kernel ALONE spends per VALU wave-instruction and SIMD
    (GRBM_GUI_ACTIVE x 1024 / SQ_INSTS_VALU). The floor is 2 cycles per wave64 instruction on a SIMD-32, so the kernel alone sits at
    2 / cycles_alone of the VALU issue peak whatever the clock. THIS run's legs are rates (permutations/s); they are compared with the
    peak at the shader clock THIS run's isolated leaf-kernel leg implies (rate x instructions x cycles_alone / 1024 SIMDs -- it
    reproduces rocm-smi's reading), not with a peak at another run's clock: the sponge runs power-limited and its clock moves by
    10 % between boxes and loads. `isolated` = the LEAF kernel alone (mp2g_batch_rehash_dev over 2^20 resident leaves of 135 limbs:
    the launch the instruction count was taken from). `mix_model`: the kernel's instruction histogram priced with the cycles each
    opcode class costs as a single-instruction stream (tools/ubench under --pmc, profiles/r06/leaf_sponge_mix.json): the kernel issues
    FASTER than that additive price -- nothing of its time is left to scheduling."""
    for rnd in ("r06", "r05"):
        try:
            with open(os.path.join(ROOT, "profiles", rnd, "sponge_counters.json")) as f:
                k = json.load(f)
        except (OSError, ValueError):
            continue
        try:
            per_perm = k["valu_insts_per_perm"]  # VALU instructions of ONE permutation (one lane); a wave instruction serves 64 of them
            cyc_alone = k["cycles_per_valu_wave_inst_achieved"]  # shader cycles per VALU wave-instruction and SIMD of the kernel alone (counter pass: clock-free)
        except KeyError:
            continue
        mix = None
        try:
            with open(os.path.join(ROOT, "profiles", "r06", "leaf_sponge_mix.json")) as f:
                mix = json.load(f)
        except (OSError, ValueError):
            pass
        need = lambda rate: rate / 64.0 * per_perm
        sclk = need(isolated_rate) * cyc_alone / 1024.0  # the clock at which 3.0 cycles per instruction give this run's isolated rate
        peak = 1024.0 * sclk / 2.0
        additive = mix["cycles"]["cycles_per_valu_inst_additive"] if mix and "cycles" in mix else None

        def leg(rate, what):
            d = {"perms_per_s": rate, "frac": need(rate) / peak, "cycles_per_valu_wave_inst": 1024.0 * sclk / need(rate), "leg": what}
            if additive:
                d["additive_mix_price_over_achieved"] = additive / d["cycles_per_valu_wave_inst"]
            return d
        out = {"kernel": "leaf_hash_poly_major_kernel<0> (Poseidon2 sponge, one lane = one leaf)", "bound": "VALU issue", "unit": "VALU wave-instructions/s",
               "valu_insts_per_perm": per_perm, "cycles_per_valu_wave_inst_alone": cyc_alone, "floor_cycles_per_valu_wave_inst": 2.0,
               "frac_alone_clock_free": 2.0 / cyc_alone,
               "sclk_hz_this_run_inferred": sclk, "peak_valu_wave_insts_per_s": peak,
               "peak_note": "1024 SIMDs x sclk / 2 cycles per wave64 instruction, sclk = the clock this run's isolated leg implies at the counter pass's cycles per instruction "
                            "(rounds 4-5 divided this run's rates by a peak at the COUNTER pass's clock, 10 % lower: their 0.73 was 0.665)",
               "isolated": leg(isolated_rate, "the leaf kernel alone: mp2g_batch_rehash_dev(parts = 1) over 2^20 resident leaves x 135 limbs (17 permutations per lane), median of 7 launches between HIP events, this run; "
                                              "its frac is 2 / cycles_alone by construction (the run's clock is inferred from this leg)"),
               "commit": leg(commit_rate, "commit_135x2p15 (leaf sponge + tree levels: the levels' launches are in the time, their permutations counted at the leaf kernel's instruction count)"),
               "source": f"profiles/{rnd}/sponge_counters.json (committed rocprofv3 --pmc passes: instructions per permutation, cycles per instruction; the rates are this run's)"}
        if isolated_runs_ms is not None:
            out["isolated"]["runs_ms"] = isolated_runs_ms
        if row_major_rate is not None:
            out["row_major_sponge_perms_per_s"] = row_major_rate  # hash_no_pad_batch_kernel (the `sponge` leg): another kernel, NOT priced with this kernel's instruction count
        if mix and "cycles" in mix:
            c = mix["cycles"]
            out["mix_model"] = {"cycles_per_valu_inst_additive": additive, "cycles_per_valu_inst_achieved_alone": cyc_alone, "additive_over_achieved": additive / cyc_alone,
                                "cycles_per_valu_inst_additive_without_stream_overhead": c.get("cycles_per_valu_inst_additive_without_stream_overhead"),
                                "simd_busy_fraction_alone": c.get("busy_fraction_of_the_kernel_alone"),
                                "cycles_per_instruction_class": c["per_instruction_class"],
                                "top_of_the_mix": [[r["opcode"], r["share"], r.get("cycles_each")] for r in mix["histogram"][:6]],
                                "reading": c["reading"], "source": "profiles/r06/leaf_sponge_mix.json (tools/dbg/isa_mix.py: the kernel's histogram x " + c["source"] + ")"}
        if "step_valu_wave_insts_per_framework_proof" in k:
            out["step_valu_wave_insts_per_framework_proof"] = k["step_valu_wave_insts_per_framework_proof"]
            out["step_source"] = k.get("step_source")
        if "in_step_perms_per_s" in k:
            # the committed one-worker trace ran at ITS clock: its fraction is clock-free only as a ratio of rates measured in the same session
            alone_then = k.get("isolated_perms_per_s_kernel_trace")
            out["in_step"] = {"perms_per_s": k["in_step_perms_per_s"], "leg": k.get("in_step_source", "table build under rocprofv3 --kernel-trace (committed profile; not this run)")}
            if alone_then:
                out["in_step"]["over_alone_in_the_same_session"] = k["in_step_perms_per_s"] / alone_then
                out["in_step"]["frac"] = k["in_step_perms_per_s"] / alone_then * 2.0 / cyc_alone
        return out
    return None


def visible_gpus():
    """GPUs this process would see, counted WITHOUT the HIP / HSA runtime (the parent of the ranks must stay GPU-free: it starts
    child processes): the KFD topology in sysfs -- nodes with SIMDs are GPUs -- narrowed by the *_VISIBLE_DEVICES lists. None when
    sysfs does not tell (no amdgpu driver in this container): the ranks themselves then report a shortage."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        nodes = sorted(os.listdir(base), key=lambda x: int(x) if x.isdigit() else 1 << 30)
    except OSError:
        nodes = []
    gpus = 0
    for nd in nodes:
        try:
            with open(os.path.join(base, nd, "properties")) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
        except OSError:
            continue
        if int(props.get("simd_count", "0")) > 0:
            gpus += 1
    gpus = gpus or None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            listed = len([x for x in v.split(",") if x.strip() != ""])
            gpus = listed if gpus is None else min(gpus, listed)
    return gpus


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher around it: start N ranks (one per GPU, `torch.distributed.run` on
    127.0.0.1) as a CHILD process, before this process has imported torch or made any GPU call (a process that has
    initialised the GPU must not exec or fork workers), pass their output through and leave with their exit code."""
    import socket
    import subprocess
    if os.environ.get("MP2G_BENCH_BACKEND", "nccl") == "nccl":
        have = visible_gpus()
        if have is not None and have < n:
            raise SystemExit(f"bench.py: --gpus {n} needs {n} visible GPUs for the RCCL backend, this node shows {have} "
                             "(MP2G_BENCH_BACKEND=gloo shares the devices among the ranks: a plumbing check, not a measurement)")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))
    out = None
    for line in p.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
        if line.startswith("{"):
            try:
                out = json.loads(line)
            except ValueError:
                pass
    rc = p.wait()
    if rc:
        raise SystemExit(rc)
    return out


def main(argv=None):
    av = sys.argv[1:] if argv is None else list(argv)
    if av[:1] == ["--cpu-farm"]:
        return cpu_farm_main()
    if av[:1] == ["--cpu-farm-worker"]:
        return cpu_farm_worker(av[1:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=128, help="leaf proofs per step and rank")
    ap.add_argument("--base-bits", type=int, default=13)
    ap.add_argument("--streams", type=int, default=4, help="HIP streams: 1 = both shapes on one; 2 = one per shape; 4, 6, 8 ... = streams / 2 part-batches per shape")
    ap.add_argument("--host-inputs", action="store_true",
                    help="PCIe-inclusive variant: every step uploads its wire matrices from pinned host memory "
                         "on the prover's stream (never the headline value; see DESIGN.md)")
    ap.add_argument("--hasher", choices=("poseidon2", "poseidon"), default="poseidon2",
                    help="poseidon2 = the reference's default config (Poseidon2GoldilocksConfig); poseidon = its "
                         "`original_poseidon` feature (mp2-common/src/lib.rs:37-40), the variant pinned against the reference")
    ap.add_argument("--witness-check", action="store_true",
                    help="also run the device-side witness check (gate + copy constraints on H) inside every prove, "
                         "as plonky2's prove() does before it panics on a bad witness")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the timed CPU leg (the self-check still runs; --workload table: with --full)")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle self-check of the sampled proofs (--workload table: with --full)")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="seconds of CPU oracle work for the cpu_baseline sample (--workload table: with --full)")
    ap.add_argument("--trees", type=int, default=8, help="--workload recursion: independent trees per rank and step, one host thread + GPU stream each")
    ap.add_argument("--rows", type=int, default=None, help="--workload table: table rows per rank and step (5 framework proofs each). Unset: 1024 rows a step, so "
                    "that --steps 128 gives every rank a 2^17-row block and 8 ranks the metric's 2^20-row table (8 x 2^17 rows + 7 separator rows); see block_plan()")
    ap.add_argument("--full", action="store_true", help="after the headline, everything else the line reports: the self-check against the CPU oracle, cpu_baseline, "
                    "the whole-table digest, the kernel legs (roofline, sponge, commit, roofline_alu), config2, by_base_degree, --leaves-leg, the clocks. Off: the "
                    "run sets up, warms up, times the steps, writes --dump-outputs and prints the line. (--workload table; the other workloads and --resume-dir "
                    "always run their own checks)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="--workload table: after the timed steps write what the timed block returned -- its root proof "
                    "(public inputs, caps, openings, FRI proof) -- as DIR/<name>.npy, float64 (see dump_outputs)")
    ap.add_argument("--workers", type=int, default=4, help="--workload table: concurrent work-plan items per rank, one host thread + GPU stream + prover set each")
    ap.add_argument("--table-batch", type=int, default=48, help="--workload table: proofs per prove() launch sequence of a worker (round 5: 4 x 48 in flight does 912 proofs/s "
                    "where 4 x 32 does 842 -- the per-batch latency kernels, witness replay, transcript, tree tops, are paid once per 48 proofs; profiles/r05/variants_ab.txt -- and "
                    "takes 78 GB of the GPU's 288 with the provers' shared scratch, 238 GB with MP2G_SHARE_SCRATCH=0)")
    ap.add_argument("--subtree", type=int, default=64, help="--workload table: into_batched_workplan(subtree_size), the rows of one work-plan item")
    ap.add_argument("--native-build", action="store_true", default=True, help="--workload table: the table build's scheduler in C++ (mp2g_forest_*: worker threads, "
                    "level batching, job assembly, child proofs in a device pool): the default")
    ap.add_argument("--python-build", dest="native_build", action="store_false", help="--workload table: table.TableBuild's Python unit loop over mp2g_chain_run "
                    "instead of the native scheduler (the A/B switch; also what --host-witness uses)")
    ap.add_argument("--group-rows", type=int, default=None, help="--workload table: rows a worker takes at a time = several work-plan items of one wave proved as one unit "
                    "(cells trees in full batches, row-tree levels merged across the items); default 32 x --table-batch (capped at the wave's rows / workers), 1 = one item at a time")
    ap.add_argument("--host-witness", action="store_true", help="--workload table / recursion: replay the witness programs on host threads (mp2g_witness_program_run_rows) "
                    "instead of on the device (mp2g_witness_program_run_dev, the default): the A/B switch")
    ap.add_argument("--lean", action="store_true", help="--workload table: keep only the frontier of the row tree in host memory (automatic above 16384 rows); the "
                    "self-check is then the root's public inputs and the oracle's verifier on the root, not the re-proving of sampled nodes")
    ap.add_argument("--leaves-leg", action="store_true", help="--workload table at N = 1 with --full: also run the short prove()-only leg on synthetic circuits (round 2's headline, "
                    "`leaves_prove_only`); off by default since round 6: the driver's window goes to the 2^17-row block")
    ap.add_argument("--no-leaves-leg", action="store_true", help="(the default now; kept so that older command lines still parse)")
    ap.add_argument("--pad-base-bits", type=int, default=0, help="--workload table: pad every base circuit of both circuit sets to 2^k rows (no-op rows) and give it "
                    "the reference's leaf gate set (SURVEY 8(d): base degrees k = 12..15); 0 = the circuits' natural degrees (the headline)")
    ap.add_argument("--degree-sweep", default="12,13,14,15", help="--workload table at N = 1 with --full: after the headline, the table rate at these base degrees (one block of "
                    "--sweep-rows rows each) in the same line as `by_base_degree`; '' = skip")
    ap.add_argument("--sweep-rows", type=int, default=1024, help="rows of the block timed at every base degree of --degree-sweep (halved above k = 14)")
    ap.add_argument("--sweep-runs", type=int, default=2, help="builds of that block per base degree; the median is reported (of two builds: the later one, the first still grows buffers). "
                    "Round 5 ran 3; 2 keeps the driver's N = 1 command inside its window now that the timed block is 2^17 rows")
    ap.add_argument("--config2-leaves", type=int, default=1024, help="--workload table at N = 1 with --full: leaves of the BASELINE configs[2] leg (2-to-1 aggregation of real leaf proofs, "
                    "2 x leaves - 1 framework proofs) reported as `config2`; 0 = skip")
    ap.add_argument("--resume-dir", default=None, help="--workload table at N = 1: build the table as --table-blocks blocks of --steps x --rows rows ACROSS CALLS -- every "
                    "block's root proof is kept in this directory as ProofWithVK bytes (mapreduce-plonky2_amd/proofstore.py: the reference's proof store, "
                    "mp2-v1/tests/common/proof_storage.rs), blocks already there are skipped, and once all are present the join levels (separator rows) are "
                    "proved, the root is verified and the record is written (--record). One call does as many blocks as fit --max-seconds")
    ap.add_argument("--table-blocks", type=int, default=8, help="--resume-dir: blocks of the table (a power of two; block b holds the prefix 2 b, separator rows the odd ones)")
    ap.add_argument("--max-seconds", type=float, default=3000.0, help="--resume-dir: do not start another block when the call would run past this many seconds")
    ap.add_argument("--record", default=None, help="--resume-dir: where the record of the completed table goes (default: <resume-dir>/table_record.json)")
    ap.add_argument("--workload", choices=("table", "leaves", "tree", "recursion", "ntt"), default="table",
                    help="table (default, the headline): BASELINE configs[3] sampled -- per row 4 cells-tree + 1 row-tree REAL framework proofs, work-plan "
                         "scheduled, witness generation inside the timed region (run_table). leaves: prove() only on synthetic circuits with resident witnesses "
                         "(last round's headline). tree: every step also proves the 2-to-1 aggregation "
                         "levels above the leaves -- locally below the shard boundary, then log2(ranks) levels whose child proofs move "
                         "between ranks with point-to-point send/recv (RCCL on device tensors). recursion: REAL circuits -- the map / "
                         "reduce circuits of recursion-framework/tests/integration.rs with universal verifiers, wrapped to the shared "
                         "shape; witnesses by the recorded witness programs on host threads, inside the timed region")
    args = ap.parse_args(argv)
    if args.resume_dir and (args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        raise SystemExit("bench.py: --resume-dir builds the blocks one after another on ONE GPU (the single-GPU rehearsal of the N-rank run); "
                         "with N GPUs every rank builds its block in one call: drop --resume-dir and pass --gpus N")
    if args.dump_outputs and (args.workload != "table" or args.resume_dir):
        raise SystemExit("bench.py: --dump-outputs writes the root proof of the timed table block: --workload table without --resume-dir")
    if args.gpus > 1 and "RANK" not in os.environ:
        return launch_ranks(args.gpus, sys.argv[1:] if argv is None else list(argv))
    plain = args.workload == "table" and not args.resume_dir and not args.full  # the headline alone: no helper processes, no side legs
    clocks = NoClocks() if plain else ClockReader()  # before anything initialises the GPU
    # the CPU baseline's process farm (N = 1 only, like cpu_baseline itself): its helper too must exist before the GPU is touched
    farm = CpuFarm() if (args.workload == "table" and args.full and not args.resume_dir and not args.no_cpu_baseline and not args.no_verify
                         and int(os.environ.get("WORLD_SIZE", "1")) == 1) else None

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        # MP2G_BENCH_BACKEND=gloo runs the multi-rank code path on a box with fewer GPUs than ranks (ranks share
        # devices round-robin; collectives go through host tensors) -- a plumbing check, not a measurement
        backend = os.environ.get("MP2G_BENCH_BACKEND", "nccl")
        if backend != "nccl":
            local_rank %= max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_rank)
        # a bounded wait on every collective and point-to-point transfer: a rank that died or never arrived makes its peers fail
        # with the backend's error (non-zero exit) instead of waiting for ever. Longer than the longest stretch a rank proves alone.
        import datetime
        limit = datetime.timedelta(seconds=float(os.environ.get("MP2G_DIST_TIMEOUT_S", "1500")))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=limit)
        else:
            dist.init_process_group(backend, timeout=limit)

    VARIANT = 0 if args.hasher == "poseidon2" else 1
    if args.workload in ("tree", "recursion"):
        clocks.close()
        return (run_tree if args.workload == "tree" else run_recursion)(args, rank, local_rank, world, dist, torch, VARIANT)
    if args.workload == "ntt":
        out = run_ntt_leg(args, local_rank, clocks)
        clocks.close()
        return out
    if args.workload == "table" and args.resume_dir:
        assert world == 1, "--resume-dir builds the blocks one after another on one GPU (with N ranks, every rank builds its block in one call: --gpus N)"
        return run_table_resumable(args, local_rank, VARIANT, clocks)
    if args.workload == "table":
        try:
            return run_table(args, rank, local_rank, world, dist, torch, VARIANT, clocks, farm)
        finally:
            if farm is not None:
                farm.close()
    return run_leaves(args, rank, local_rank, world, dist, torch, VARIANT, clocks)


def cpu_model():
    """the host CPU's model string (printed beside every CPU number)"""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def cpu_medians(unit, runs=5):
    """medians of `runs` oracle runs of ONE fixed unit of work -- `unit` = a captured prove() call (label, circuit,
    oracle params, circuit digest, wires, pi_hash, ...) -- with all hardware threads (one run after the other) and with one thread
    (the `runs` single-thread runs side by side on otherwise idle cores, each timed by itself)."""
    import threading
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits as OC
    label, ckt, ofp, cd, make_wires, ph = unit[:6]
    wires = make_wires()
    omp = ctypes.CDLL("libgomp.so.1")
    cores = os.cpu_count() or 1

    def one(threads, out, i):
        omp.omp_set_num_threads(threads)
        t0 = time.perf_counter()
        OC.prove_witness(ckt, ofp, cd, wires, ph)
        out[i] = time.perf_counter() - t0

    warm = [0.0]
    one(cores, warm, 0)
    allt = [0.0] * runs
    for i in range(runs):
        one(cores, allt, i)
    single = [0.0] * runs
    ths = [threading.Thread(target=one, args=(1, single, i)) for i in range(runs)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    omp.omp_set_num_threads(cores)
    return {"unit_of_work": f"one prove() of {label} (2^{ckt.log_n} rows) by oracle/ from the GPU run's captured witness", "runs": runs,
            "all_threads": {"threads": cores, "median_s": float(np.median(allt)), "proofs_per_s": 1.0 / float(np.median(allt))},
            "one_thread": {"threads": 1, "median_s": float(np.median(single)), "proofs_per_s": 1.0 / float(np.median(single)),
                           "how": f"{runs} single-thread runs side by side on {cores} hardware threads, each timed by itself"}}


def native_oracle():
    """the CPU leg runs the oracle built for the machine at hand. `make -B liboracle_native.so` (-O3 -march=native
    -fopenmp; ~7 s) and point tests/oracle.py at it through ORC_LIB -- before that module is first imported. The file never travels
    (.gpurunignore). Returns what the line reports about the build; on any failure the portable build (-march=x86-64-v3) stays."""
    if "oracle" in sys.modules or os.environ.get("ORC_LIB"):
        return {"march": "as loaded", "lib": os.environ.get("ORC_LIB", "oracle/liboracle.so")}
    import subprocess
    try:
        subprocess.check_call(["make", "-s", "-B", "-C", os.path.join(ROOT, "oracle"), "liboracle_native.so"], timeout=300)
        os.environ["ORC_LIB"] = os.path.join(ROOT, "oracle", "liboracle_native.so")
        return {"march": "native", "lib": "oracle/liboracle_native.so (built by this run: -O3 -march=native -fopenmp)"}
    except Exception as e:
        return {"march": "x86-64-v3", "lib": f"oracle/liboracle.so (the native build failed: {type(e).__name__})"}


def host_memory_available():
    """bytes this process may still take: MemAvailable, narrowed by the cgroup's limit where there is one"""
    avail = None
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    avail = int(line.split()[1]) * 1024
    except OSError:
        pass
    for lim, cur in (("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory.current"),
                     ("/sys/fs/cgroup/memory/memory.limit_in_bytes", "/sys/fs/cgroup/memory/memory.usage_in_bytes")):
        try:
            with open(lim) as f:
                v = f.read().strip()
            with open(cur) as f:
                u = int(f.read().strip())
            if v != "max" and int(v) < 1 << 60:
                left = int(v) - u
                avail = left if avail is None else min(avail, left)
        except (OSError, ValueError):
            pass
    return avail


def cpu_throughput(samples, seconds_per_mode=8.0, modes=None):
    """The CPU's best configuration for THIS metric (framework proofs per second of a table build: embarrassingly parallel across
    proofs): P oracle proofs side by side x T OpenMP threads inside each, P x T = the host's hardware threads, for
    (P, T) = (cores, 1), (cores / 4, 4), (cores / 16, 16); the fourth point, one proof after the other with every thread inside
    it, is the latency mode `check_against_oracle` has already timed. Work of a mode: the sampled framework proofs of the timed
    block in the table's own proportion -- per two rows 2 x (4 cells-tree proofs) + a row leaf + a row full node --, each slot pulls
    the next one until `seconds_per_mode` have passed and finishes the one it holds; value = proofs completed / wall time to the
    last one. P is capped by the host's free memory (a proof's working set ~ 24 KB per row of its widest circuit).
    `samples`: the captured prove() calls grouped by framework proof. Returns (best mode's dict, all modes)."""
    import threading
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits as OC
    cores = os.cpu_count() or 1
    omp = ctypes.CDLL("libgomp.so.1")
    kind = lambda chain: chain[0][0].rsplit(" step", 1)[0]
    cells = [c for c in samples if kind(c).startswith("cells")]
    rows_leaf = [c for c in samples if kind(c) == "row_leaf"] or [c for c in samples if kind(c).startswith("row")][:1]
    rows_full = [c for c in samples if kind(c) == "row_full"] or rows_leaf
    cycle = (cells + rows_leaf[:1] + cells + rows_full[:1]) if cells else list(samples)
    widest = max(1 << part[1].log_n for c in cycle for part in c)
    per_proof_bytes = 24 * 1024 * widest
    avail = host_memory_available()
    p_cap = cores if avail is None else max(1, int(0.5 * avail) // per_proof_bytes)
    if modes is None:
        modes = []
        for t in (1, 4, 16):
            pt = (max(1, min(cores // t, p_cap)), t)
            if cores >= t and pt not in modes:
                modes.append(pt)
    out = []
    for P_, T_ in modes:
        nxt, done, lock = [0], [0], threading.Lock()
        t0 = time.perf_counter()

        def slot():
            omp.omp_set_num_threads(T_)  # per-thread ICV: the parallel regions this slot opens
            while True:
                with lock:
                    if time.perf_counter() - t0 > seconds_per_mode and nxt[0] >= P_:
                        return
                    j = nxt[0]
                    nxt[0] += 1
                for label, ckt, ofp, cd, make_wires, ph, *_ in cycle[j % len(cycle)]:
                    OC.prove_witness(ckt, ofp, cd, make_wires(), ph)
                with lock:
                    done[0] += 1

        ths = [threading.Thread(target=slot) for _ in range(P_)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        wall = time.perf_counter() - t0
        out.append({"mode": f"{P_} proofs side by side x {T_} thread(s) each", "concurrent_proofs": P_, "threads_per_proof": T_, "framework_proofs": done[0],
                    "wall_s": round(wall, 2), "proofs_per_s": done[0] / wall})
    omp.omp_set_num_threads(cores)
    best = max(out, key=lambda m: m["proofs_per_s"])
    return best, {"modes": out, "mix": "per two table rows: 2 x the 4 cells-tree proofs, 1 row leaf, 1 row full node (the sampled proofs of the timed block, their captured witnesses)",
                  "memory_cap": {"available_bytes": avail, "assumed_bytes_per_proof": per_proof_bytes, "max_concurrent": p_cap}}


def cpu_throughput_modes(samples, farm, seconds_per_mode):
    """cpu_baseline's throughput modes: P oracle proofs side by side x T OpenMP threads each with P x T = the host's hardware
    threads, for T = 1 and 4 -- as separate PROCESSES through the farm (CpuFarm: one address space per proof), or, without a farm
    (a profiler preloaded, the helper could not start), as threads of this process (cpu_throughput). Returns (best mode, sweep)."""
    cores = os.cpu_count() or 1
    if farm is None or farm.p is None:
        best, sweep = cpu_throughput(samples, seconds_per_mode)
        sweep["how"] = "threads of one process (no farm helper available)"
        return best, sweep
    import shutil
    import tempfile
    widest = max(1 << part[1].log_n for c in samples for part in c)
    per_proof_bytes = 24 * 1024 * widest
    avail = host_memory_available()
    p_cap = cores if avail is None else max(1, int(0.5 * avail) // per_proof_bytes)
    # cores / 4 x 4 and cores / 16 x 16 in every run; cores x 1 only on request (MP2G_CPU_MODES=1,4,16): every worker must finish a
    # whole framework proof, 167 s on the 256-thread host of the GPU box for the same 1.5 proofs/s (profiles/r06/cpu_throughput_modes.json)
    ts = [int(x) for x in os.environ.get("MP2G_CPU_MODES", "4,16").split(",") if x.strip()]
    modes = []
    for t in ts:
        pt = [max(1, min(cores // t, p_cap)), t]
        if cores >= t and pt not in modes:
            modes.append(pt)
    if not modes:
        modes = [[max(1, min(cores, p_cap)), 1]]
    spool = tempfile.mkdtemp(prefix="mp2g_cpu_spool_")
    try:
        spool_samples(samples, spool)
        res = farm.run(spool, modes, seconds_per_mode)
    finally:
        shutil.rmtree(spool, ignore_errors=True)
    if isinstance(res, dict):
        raise RuntimeError(f"CPU farm: {res.get('error')}")
    best = max(res, key=lambda m: m["proofs_per_s"])
    return best, {"modes": res, "how": "separate processes (bench.py --cpu-farm: a helper started before the GPU was touched spawns P workers per mode; each maps the "
                                       "spooled samples, all are released together; proofs completed / time to the last worker's end)",
                  "mix": "per two table rows: 2 x the 4 cells-tree proofs, 1 row leaf, 1 row full node (the sampled proofs of the timed block, their captured witnesses)",
                  "memory_cap": {"available_bytes": avail, "assumed_bytes_per_proof": per_proof_bytes, "max_concurrent": p_cap},
                  "recorded": recorded_cpu_modes()}


def recorded_cpu_modes():
    """the committed record of ALL modes (cores x 1 included: 167 s a run), measured on the GPU box's host in round 6"""
    try:
        with open(os.path.join(ROOT, "profiles", "r06", "cpu_throughput_modes.json")) as f:
            r = json.load(f)
        return {"source": "profiles/r06/cpu_throughput_modes.json (committed; not this run)", "cpu_model": r.get("cpu_model"),
                "proofs_per_s": {m["mode"]: round(m["proofs_per_s"], 3) for part in ("separate_processes", "threads_of_one_process") for m in r[part]["modes"]}}
    except (OSError, ValueError, KeyError):
        return None


class TableRig:
    """what a table build runs on at one base degree: `workers` GPU contexts (= streams) with a prover set and a proof session each,
    and the two circuit sets (table.TableParams) built for that degree. pad_bits = 0: the circuits at their natural degrees."""

    def __init__(self, mods, local_rank, variant, workers, batch, subtree, host_witness, ranks_here, pad_bits=0, group_rows=None, native=False):
        mp2, R, FW, C, T, IX = mods
        self.native, self.native_build = bool(native) and not host_witness, None
        self.mods, self.variant, self.batch, self.subtree, self.pad_bits, self.group_rows = mods, variant, batch, subtree, pad_bits, group_rows
        self.ctxs = [mp2.Context(local_rank) for _ in range(max(1, workers))]
        self.ctx = self.ctxs[0]
        self.provers = [FW.GpuProver(c, variant, witness_check=True, capacity=batch, device_witness=not host_witness) for c in self.ctxs]
        self.sessions = [R.ProofSession(p) for p in self.provers]
        t0 = time.perf_counter()
        self.params = T.TableParams(self.provers[0], lambda ckt: FW.circuit_fri_params(ckt, variant), IX.empty_poseidon_hash(self.ctx, variant),
                                    pad_base_bits=pad_bits, extra_gates=C.LEAF_KINDS if pad_bits else ())
        self.setup_s = time.perf_counter() - t0
        # host threads of one worker (host-witness replay only) and the device memory the provers will take, sized for every rank of
        # the node being at work at once; a configuration that cannot fit one GPU is refused here, not by an allocation in mid-run
        sharding = importlib.import_module("mapreduce-plonky2_amd.sharding")
        free, total = self.ctx.mem_info()
        self.plan = sharding.plan_rank_resources(self.params.shapes(), len(self.ctxs), batch, ranks_here, os.cpu_count() or 1, hbm_bytes=total)
        if not self.plan["fits"] and not os.environ.get("MP2G_BENCH_BACKEND"):
            self.close()
            raise SystemExit(f"bench.py: {len(self.ctxs)} workers x {batch} proofs in flight need ~{self.plan['device_bytes_per_rank'] / 1e9:.0f} GB of device memory at "
                             f"these circuit shapes, the GPU has {total / 1e9:.0f} GB: lower --table-batch or --workers")
        self.host_threads = self.plan["host_threads_per_worker"]
        self.mem_total = total
        self.n_proofs = 0

    def build(self, n_rows, block, seed=0xC0FFEE04, n_cols=4, lean=False):
        """one contiguous block of n_rows rows: off-circuit witness data, then every cells-tree and row-tree proof, work-plan scheduled"""
        mp2, R, FW, C, T, IX = self.mods
        table = T.SyntheticTable(n_rows, n_cols, seed=seed, block=block)
        root, nodes, spans = T.balanced_bst(n_rows)
        samples, keep = T.sample_nodes(nodes, spans)
        wit = T.TableWitness(self.ctx, table, spans, self.variant)
        if self.native:
            # the scheduler in C++ (csrc/forest.hip): nodes registered once, every wave of the plan one mp2g_forest_prove call
            if self.native_build is None:
                self.native_build = T.NativeTableBuild(self.params, self.provers, batch=self.batch, subtree_size=self.subtree, group_rows=self.group_rows)
            tb = self.native_build
            n0 = tb.n_proofs
            t0 = time.perf_counter()
            proof, name = tb.run(table, wit, root, nodes, keep=samples)
            self.n_proofs += tb.n_proofs - n0
            self.last_glue = {"scheduler": "native (mp2g_forest_*)", "block_s": round(time.perf_counter() - t0, 2),
                              "inside_libmp2gpu_s": round(tb.seconds_in_prove, 2)}  # mp2g_forest_prove_plan: the plan's waves, units, batches
        else:
            tb = T.TableBuild(self.params, self.sessions, batch=self.batch, subtree_size=self.subtree, host_threads=self.host_threads,
                              keep_proofs=not lean, keep_nodes=keep if lean else (), group_rows=self.group_rows)
            lib0 = tb.seconds_in_library()
            proof, name = tb.run(table, wit, root, nodes)
            self.n_proofs += tb.n_proofs
            self.last_glue = {"scheduler": "python (table.TableBuild)", "worker_busy_s": round(tb.seconds_in_units, 2),
                              "inside_libmp2gpu_s": round(tb.seconds_in_library() - lib0, 2)}
        return {"table": table, "root": root, "nodes": nodes, "spans": spans, "samples": samples, "build": tb, "wit": wit, "proof": proof, "name": name,
                "digest_w": wit.root_digest_w[root]}

    def join_build(self):
        """the TableBuild that proves a separator row above two blocks (its one-row cells tree and a full row node): the Python unit
        loop over this rig's sessions, whichever scheduler built the blocks"""
        mp2, R, FW, C, T, IX = self.mods
        if getattr(self, "_join_build", None) is None:
            self._join_build = T.TableBuild(self.params, self.sessions, batch=self.batch, subtree_size=self.subtree, host_threads=self.host_threads)
        return self._join_build

    def check_root(self, st, verify=True):
        """the block root against the off-circuit side (tree hash, multiset digest = compute_table_row_digest of the block, min / max,
        circuit-set digest) and, with `verify`, against the oracle's verifier (transcript, PLONK identity with the gate terms, FRI)"""
        mp2, R, FW, C, T, IX = self.mods
        table, pis = st["table"], st["proof"][3]
        want = T.expected_root_public_inputs(self.ctx, table, st["wit"], st["root"], st["nodes"], st["spans"], self.variant)
        assert np.array_equal(pis[:T.ROWS_IO], want), "the block root's public inputs differ from the off-circuit tree hash / digest / min / max"
        assert np.array_equal(pis[T.ROWS_IO:], np.asarray(self.params.rows.set_digest, dtype=np.uint64)), "circuit-set digest"
        w_all, wei_all = mp2.compute_table_row_digest(self.ctx, table.col_ids, table.values, table.values[:, 0:1])
        assert np.array_equal(wei_all, pis[4:15]), "individual digest != compute_table_row_digest of the block"
        if verify:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import circuits as OC
            import oracle as O
            wckt, _, wdig = self.params.rows.chains[st["name"]][-1]
            rc = OC.verify(wckt, OC.oracle_params(wckt), np.asarray(wdig, dtype=np.uint64), O.hash_n_to_m_no_pad(pis, 4), *st["proof"][:3])
            if rc:
                raise SystemExit(f"bench.py self-check FAILED: the oracle's verifier rejects the block root (code {rc})")
        return want, w_all

    def capture_samples(self, st):
        """one framework proof of every circuit kind of the block, re-proved WITH CAPTURE from the inputs the timed run used (row 0's
        cells tree; row 0 and the widest node of every other kind of the row tree) and required to equal the timed run's proofs.
        Returns the captured prove() calls grouped by framework proof: what the CPU oracle re-proves bit for bit."""
        mp2, R, FW, C, T, IX = self.mods
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import circuits as OC
        table, wit, nodes, build = st["table"], st["wit"], st["nodes"], st["build"]
        cap, sess, row0, cells, Cn = [], self.sessions[0], 0, {}, table.n_cols
        for k in sorted(range(1, Cn + 1), key=lambda k: ((k & -k).bit_length(), k)):
            kids = [c for c in T.sbbst_children(Cn, k) if c is not None]
            name = ("cells_leaf", "cells_partial", "cells_full")[len(kids)]
            flat = T._u64cat([table.col_ids[k]], table.values[row0, k], [0], wit.cell_digest[row0, k - 1], T.NEUTRAL_FIELDS)
            (pr,) = self.params.cells.generate_proofs_batch(name, [([cells[c][0] for c in kids], [cells[c][1] for c in kids], flat)], session=sess, capture=cap)
            cells[k] = (pr, name)
        root_cells = cells[T.sbbst_root(Cn)]
        assert all(np.array_equal(a, b) for a, b in zip(root_cells[0], build.cells_roots[row0][0])), "re-proved cells root != the timed run's"
        for k in st["samples"]:
            name, job = build.row_job(table, wit, nodes, k, build.cells_roots[k], build.row_proofs)
            (pr,) = self.params.rows.generate_proofs_batch(name, [job], session=sess, capture=cap)
            assert all(np.array_equal(a, b) for a, b in zip(pr, build.row_proofs[k][0])), f"re-proved {name} != the timed run's"
        samples, chain = [], []
        for (name, stp, ckt, digest, wires, ph, caps, openings, proof) in cap:
            if stp == 0 and chain:
                samples.append(chain)
                chain = []
            chain.append((f"{name} step {stp}", ckt, OC.oracle_params(ckt), np.asarray(digest, dtype=np.uint64), (lambda w=wires: w), ph, caps, openings, proof, True))
        samples.append(chain)
        return samples

    def close(self):
        if self.native_build is not None:
            self.native_build.free()
        for p_ in self.provers:
            p_.free()
        for c in reversed(self.ctxs):
            c.close()


class WorkerRig:
    """`workers` GPU contexts with a prover set and a proof session each -- what a leg that brings its own circuits runs on (the
    configs[2] leg: it runs after the table's rig is closed, so that its provers do not come on top of the table's)"""

    def __init__(self, mods, local_rank, variant, workers, batch, host_threads):
        mp2, R, FW, C, T, IX = mods
        self.mods, self.variant, self.batch, self.host_threads = mods, variant, batch, host_threads
        self.ctxs = [mp2.Context(local_rank) for _ in range(max(1, workers))]
        self.ctx = self.ctxs[0]
        self.provers = [FW.GpuProver(c, variant, witness_check=True, capacity=batch, device_witness=True) for c in self.ctxs]
        self.sessions = [R.ProofSession(p) for p in self.provers]

    def close(self):
        for p_ in self.provers:
            p_.free()
        for c in reversed(self.ctxs):
            c.close()


def config2_leg(rig, n_leaves, seed=0xC0FFEE03):
    """BASELINE configs[2] at full size on this rig's workers: the 2-to-1 aggregation of `n_leaves` REAL leaf proofs of
    recursion-framework/tests/integration.rs:138-261 -- n_leaves map proofs (base 2^6 + wrap 2^12 rows) and the n_leaves - 1 reduce
    proofs above them (two universal verifiers: base 2^13 + wrap 2^12), ONE tree, level by level, the batches of a level dealt to the
    workers. A 64-leaf tree first (untimed: creates the provers), then the timed tree. The root must expose (sum of the even elements,
    hash tree of the chunks, circuit-set digest) and pass the oracle's verifier."""
    from concurrent.futures import ThreadPoolExecutor
    import queue
    mp2, R, FW, C, T, IX = rig.mods
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits as OC
    import oracle as O
    t0 = time.perf_counter()
    fw = R.RecursiveCircuits([R.FrameworkCircuit("map", 0, R.map_logic, 5), R.FrameworkCircuit("reduce", 2, R.reduce_logic, 5)], rig.provers[0],
                             lambda ckt: FW.circuit_fri_params(ckt, rig.variant))
    for name in ("map", "reduce"):
        fw.witness_programs(name)
    setup_s = time.perf_counter() - t0
    pool = queue.Queue()
    for s_ in rig.sessions:
        pool.put(s_)

    def part(name, jobs):
        sess = pool.get()
        try:
            sess.prover.ctx.make_current()
            return fw.generate_proofs_batch(name, jobs, threads=rig.host_threads, session=sess)
        finally:
            pool.put(sess)

    def level_of(ex, name, jobs):
        # a level's jobs in batches of the provers' capacity, narrow levels in one batch per worker at most
        per = max(1, min(rig.batch, -(-len(jobs) // len(rig.sessions))))
        futs = [ex.submit(part, name, jobs[lo:lo + per]) for lo in range(0, len(jobs), per)]
        return [pr for f in futs for pr in f.result()]

    def tree(ex, n, data):
        level, names, count = level_of(ex, "map", [([], [], data[4 * i:4 * i + 4]) for i in range(n)]), ["map"] * n, n
        while len(level) > 1:
            level = level_of(ex, "reduce", [([level[2 * i], level[2 * i + 1]], [names[2 * i], names[2 * i + 1]], None) for i in range(len(level) // 2)])
            names = ["reduce"] * len(level)
            count += len(level)
        return level[0], names[0], count

    data = C.rand_field(4 * n_leaves, seed)
    with ThreadPoolExecutor(max_workers=len(rig.sessions)) as ex:
        tree(ex, min(64, n_leaves), data)
        for c in rig.ctxs:
            c.sync()
        t0 = time.perf_counter()
        root, root_name, count = tree(ex, n_leaves, data)
        for c in rig.ctxs:
            c.sync()
        dt = time.perf_counter() - t0
    pis = root[3]
    assert int(pis[0]) == sum(int(x) for x in data if int(x) % 2 == 0) % C.P, "configs[2] root: sum of the even elements"
    hs = rig.ctx.hash_no_pad_batch(data.reshape(n_leaves, 4), 4, rig.variant)
    while len(hs) > 1:
        hs = rig.ctx.hash_no_pad_batch(hs.reshape(len(hs) // 2, 8), 4, rig.variant)
    assert np.array_equal(pis[1:5], hs[0]) and np.array_equal(pis[5:], np.asarray(fw.set_digest, dtype=np.uint64)), "configs[2] root: hash tree / set digest"
    wckt, _, wdig = fw.chains[root_name][-1]
    rc = OC.verify(wckt, OC.oracle_params(wckt), np.asarray(wdig, dtype=np.uint64), O.hash_n_to_m_no_pad(pis, 4), *root[:3])
    if rc:
        raise SystemExit(f"bench.py self-check FAILED: the oracle's verifier rejects the configs[2] root (code {rc})")
    return {"workload": f"configs[2] at full size: 2-to-1 aggregation of {n_leaves} real leaf proofs (integration.rs:138-261), one tree, {count} framework proofs "
                        "(map: base 2^6 + wrap 2^12 rows; reduce: two universal verifiers, base 2^13 + wrap 2^12), witnesses on the device, witness check on",
            "framework_proofs": count, "seconds": dt, "value": count / dt, "unit": "framework proofs/s", "leaf_proofs_per_s": n_leaves / dt,
            "setup_s": round(setup_s, 1), "root_verified": True, "root_public_inputs": [int(x) for x in pis]}


DEFAULT_STEP_ROWS = 1024      # rows of a step when --rows is not given: 128 steps = a 2^17-row block, 8 ranks x 2^17 = BASELINE configs[3]'s 2^20-row table
WARMUP_ROWS_CAP = 5120         # the warm-up block creates the provers of every circuit; more rows than this add nothing to that


def block_plan(rows, steps, warmup, default_step_rows=None):
    """Rows of a rank's timed block and of its warm-up block: the block is steps x (rows per step), a step `rows` rows or, with `rows`
    None, `default_step_rows` (DEFAULT_STEP_ROWS; MP2G_BENCH_STEP_ROWS scales the default down for tests). The block is ONE work plan,
    steps are the unit of the timed work and of ms_per_step. The warm-up block is warmup steps, never more than WARMUP_ROWS_CAP rows.
    Returns (block rows, rows per step, warm-up rows)."""
    steps = max(1, int(steps))
    if rows is None:
        per_step = int(default_step_rows if default_step_rows is not None else os.environ.get("MP2G_BENCH_STEP_ROWS", DEFAULT_STEP_ROWS))
    else:
        per_step = int(rows)
    assert per_step >= 1
    n_rows = steps * per_step
    warm = min(max(0, int(warmup)) * per_step, WARMUP_ROWS_CAP)
    return n_rows, per_step, warm


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, proof):
    """--dump-outputs: what a caller of the timed block receives -- its root proof (caps, openings, FRI proof, public inputs; with
    several ranks the joined tree's) -- as DIR/root_<part>.npy. The parts are Goldilocks words (u64); float64 holds them exactly as
    two 32-bit halves, so every file has the part's own shape plus a last axis [low 32 bits, high 32 bits]. The inputs of a run are
    fixed by its arguments (seeded), so two builds of the project can be compared file for file. Returns the files written."""
    os.makedirs(path, exist_ok=True)
    parts = {"root_caps": proof[0], "root_openings": proof[1], "root_fri_proof": proof[2], "root_public_inputs": proof[3]}
    arrays = {}
    for name, words in parts.items():
        w = np.ascontiguousarray(words, dtype=np.uint64)
        arrays[name] = np.stack([(w & np.uint64(0xFFFFFFFF)).astype(np.float64), (w >> np.uint64(32)).astype(np.float64)], axis=-1)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes exceed {DUMP_LIMIT_BYTES}"
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(arrays)


def run_table(args, rank, local_rank, world, dist, torch, VARIANT, clocks, farm=None):
    """--workload table (the default, the headline): BASELINE configs[3] as ONE contiguous block of `--steps` x `--rows` table rows per
    rank. Per row the reference proves C = 4 cells-tree nodes (ryhope sbbst over the value columns: two leaves, a full node, a partial
    node) and one row-tree node that verifies the cells root against the cells circuit set and its 0 / 1 / 2 row children
    (mapreduce-plonky2_amd/table.py; verifiable-db/src/cells_tree/api.rs, row_tree/api.rs; mp2-v1/tests/common/celltree.rs:54-189,
    rowtree.rs:78-337). Every one of the 5 x rows framework proofs is REAL: witness generation from its recorded witness program (on
    the device), base prove() with the device-side witness check, the wrap chain down to 2^12 rows (one wrap, two for the
    three-verifier row full node: 2^14 -> 2^13 -> 2^12). The row tree of the block (a BST over the secondary index, every node a row)
    is scheduled by ryhope's batched work plan (mp2g_update_plan_*, updatetree.rs:154-163,449-531): an item = a spun-off subtree = the
    unit one worker (GPU stream + provers) proves bottom-up, `--workers` of them concurrently. The off-circuit side of the same rows
    -- value digests, their accumulation up both trees, row ids (mp2g_map_to_curve_batch, mp2g_row_digests, mp2g_curve_sum_ranges) --
    is inside the timed region too.

    A STEP is `--rows` rows (5 x rows framework proofs), 1024 without `--rows` (block_plan).
    The W warm-up steps are one contiguous block of W steps' rows, 5120 at most (other rows than the timed ones; it creates the
    provers), the K timed steps one contiguous block -- one work plan, a row tree log2(rows) deep -- not K rebuilds of the same rows. With several ranks every rank builds its own block and log2(ranks) join
    levels follow inside the timed region: the owner of a parent receives the other block's root proof (device to device over RCCL)
    and proves the separator row between the blocks. value = framework proofs per second.

    After the timed region: `--dump-outputs` writes the root proof (rank 0). With `--full`: the root's public inputs are compared with
    the off-circuit tree hash / digest / min / max and the root passes the oracle's verifier; one framework proof of every circuit kind
    is re-proved from its captured witness by the CPU oracle -- bit-exact and verified; those oracle proofs are the cpu_baseline
    sample. With `--full` at N = 1 the same line then carries: BASELINE
    configs[2] at full size (`config2`), the table rate at base degrees k = 12..15 (`by_base_degree`: every base circuit padded to
    2^k rows with the reference's leaf gate set), the prove()-only loop of round 2 (`leaves_prove_only`), the kernel
    legs (`roofline` = configs[1]'s 2^22-point NTT) and the whole-table multiset digest of 2^20 rows."""
    assert VARIANT == 0, "the recursive verifier circuit of recursion.py hashes with Poseidon2 gates (the reference's default config)"
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    R = importlib.import_module("mapreduce-plonky2_amd.recursion")
    FW = importlib.import_module("mapreduce-plonky2_amd.framework")
    C = importlib.import_module("mapreduce-plonky2_amd.circuits")
    T = importlib.import_module("mapreduce-plonky2_amd.table")
    IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
    sharding = importlib.import_module("mapreduce-plonky2_amd.sharding")
    mods = (mp2, R, FW, C, T, IX)
    n_cols, seed = 4, 0xC0FFEE04
    ranks_here = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    oracle_build = native_oracle() if args.full and world == 1 and not args.no_cpu_baseline and not args.no_verify else None  # before tests/oracle.py is first imported
    rig = TableRig(mods, local_rank, VARIANT, args.workers, args.table_batch, args.subtree, args.host_witness, ranks_here, pad_bits=args.pad_base_bits,
                   group_rows=args.group_rows, native=args.native_build)
    params, ctx = rig.params, rig.ctx
    n_rows, rows_per_step, warm_rows = block_plan(args.rows, args.steps, args.warmup)  # the timed block of this rank, and its warm-up block
    lean = args.lean or n_rows > 16384                # a block this large keeps the frontier of the tree + the sampled nodes only
    nccl = dist is not None and dist.get_backend() == "nccl"
    dev = torch.device("cuda", local_rank) if nccl else None
    final_ckt = params.rows.chains["row_leaf"][-1][0]  # every final proof of the row set has this shape (the shared common data)
    final_fp = FW.circuit_fri_params(final_ckt, VARIANT)
    n_pis = T.ROWS_IO + 4
    proof_sizes = [n_pis, 3 * final_fp.cap_words, final_fp.n_openings * 2, final_fp.proof_words]
    names = list(params.rows.circuits)
    n_levels = world.bit_length() - 1
    assert world & (world - 1) == 0, "ranks: a power of two (binary join levels)"

    def block(rows_, seed_, lean_):
        st = rig.build(rows_, 2 * rank, seed_, n_cols, lean_)
        cur = (st["proof"], st["name"], st["digest_w"])
        for lvl in range(n_levels):  # above the shard boundary: the separator rows between the ranks' blocks
            bit = 1 << lvl
            if rank & (bit - 1):
                break
            if rank & bit:
                # the root proof goes to the parent's rank from where the prover left it: device to device over RCCL
                head = torch.from_numpy(np.concatenate([[names.index(cur[1])], np.asarray(cur[2], dtype=np.uint64).view(np.int64)]).astype(np.int64))
                dist.send(head.to(dev) if nccl else head, rank - bit)
                pv = (st["build"].last_session or rig.sessions[0]).prover
                ch = getattr(pv, "last_chain", None)
                own_root = cur[0] is st["proof"]  # this rank's block root (not a joined tree: those are proved by the Python unit loop)
                if rig.native and own_root:
                    # the block root where the native scheduler left it: its slot of the forest's device pool, split into the four ranges
                    ptr, n_words = st["build"].forest.device_proof(st["root"])
                    assert n_words == sum(proof_sizes)
                    parts, at = [], 0
                    for n_ in proof_sizes:
                        parts.append((ptr + 8 * at, n_))
                        at += n_
                    out = R.DeviceProof(parts, keep=st["build"].forest)
                elif ch is not None and not args.host_witness and not rig.native:
                    assert ch.last_batch == 1, "the chain's last run was the root alone: its proof 0 is the root"
                    out = pv.last_device_proof(0)
                else:
                    out = cur[0]  # no chain outputs left on the device for it (host-witness back end; a joined tree under the native scheduler): the host proof goes (uploaded for RCCL)
                sharding.send_device_proof(dist, pv.ctx, out, rank - bit, dev)
                break
            head = torch.zeros(6, dtype=torch.int64, device=dev)
            dist.recv(head, rank + bit)
            head = head.cpu().numpy()
            other = sharding.recv_device_proof(dist, proof_sizes, rank + bit, dev)
            cur = T.join_blocks(rig.join_build(), ctx, cur, (other, names[int(head[0])], head[1:6].view(np.uint64)), 2 * (rank + bit) - 1, n_cols, seed_, VARIANT)
            rig.n_proofs += n_cols + 1  # the separator row: its cells tree (one proof per value column) and its row node
        return st, cur

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        for c in rig.ctxs:
            c.sync()

    rccl_ranks = None
    if dist is not None:  # every rank is there and the backend's collective works before anything is timed
        one = torch.ones(1, dtype=torch.int64, device=dev)
        dist.all_reduce(one)
        rccl_ranks = int(one.item())
        assert rccl_ranks == world, f"{rccl_ranks} of {world} ranks answered"
        # every join pair moves one small buffer the way its root proof will move -- under RCCL a view of a buffer allocated by
        # libmp2gpu, the one thing single-GPU tests cannot exercise; if any pair's direct send fails, ALL levels use the staged
        # hand-off (download + torch tensor). Decided here, before t0; the line's config.sharding names the mode.
        def direct(words):
            buf = ctx.to_device(words)
            ctx.sync()
            if os.environ.get("MP2G_HANDOFF_PROBE_FAIL") == str(rank):  # test knob: this rank's direct send "fails"
                raise RuntimeError("MP2G_HANDOFF_PROBE_FAIL")
            if not nccl:  # (the knob under gloo: the other ranks' "direct" tensors are host tensors)
                return staged(words)
            return torch.as_tensor(sharding._RawView(buf.ptr.value, len(words), buf), device=dev)

        def staged(words):
            t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64).copy())
            return t.to(dev) if nccl else t
        handoff = sharding.probe_handoff(dist, direct if nccl or os.environ.get("MP2G_HANDOFF_PROBE_FAIL") else None, staged, dev)
    else:
        handoff = {"mode": None, "reason": None}
    if warm_rows > 0:  # the warm-up block creates the provers of every circuit (with --warmup 0 that falls into the timed region)
        block(warm_rows, seed ^ 0x5A5A5A, args.lean or warm_rows > 16384)
    barrier()
    n0, perms0 = rig.n_proofs, mp2.leaf_permutations_queued()
    t0 = time.perf_counter()
    st, cur = block(n_rows, seed, lean)
    barrier()
    dt = time.perf_counter() - t0
    n_local = rig.n_proofs - n0
    leaf_perms = mp2.leaf_permutations_queued() - perms0
    mem_free_build, _ = ctx.mem_info()  # what the table build itself holds (the planner's estimate is for this): before any side leg creates its own provers
    if dist is not None:
        t = torch.tensor([dt, float(n_local)], device="cuda" if nccl else "cpu", dtype=torch.float64)
        dist.all_reduce(t[0:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(t[1:2], op=dist.ReduceOp.SUM)
        dt, n_total = float(t[0].item()), int(t[1].item())
    else:
        n_total = n_local
    if args.dump_outputs and rank == 0:  # what the timed block returned: the root proof (the joined tree's with several ranks)
        dump_outputs(args.dump_outputs, cur[0])

    # ---- checks (outside the timed region; --full) -------------------------------------------------------------------------
    # every rank: its block's root exposes the off-circuit tree hash, multiset digest, min / max of the block; the oracle verifies it
    verified, cpu_base, medians = 0, None, None
    if args.full:
        want, w_all = rig.check_root(st, verify=not args.no_verify)
        verified = 0 if args.no_verify else 1
    if args.full and rank == 0 and world > 1:  # the joined tree: digest = the whole table's (blocks and separators), min of block 0
        root_pis = cur[0][3]
        ws = [w_all]
        for r in range(1, world):
            tb = T.SyntheticTable(n_rows, n_cols, seed, 2 * r)
            ws.append(mp2.compute_table_row_digest(ctx, tb.col_ids, tb.values, tb.values[:, 0:1])[0])
        for s_ in range(world - 1):
            tb = T.SyntheticTable(1, n_cols, seed, 2 * s_ + 1)
            ws.append(mp2.compute_table_row_digest(ctx, tb.col_ids, tb.values, tb.values[:, 0:1])[0])
        assert np.array_equal(mp2.curve_sum(ctx, np.stack(ws), weierstrass=True)[1], root_pis[4:15]), "root digest != digest of the whole table"
        assert np.array_equal(root_pis[26:34], want[26:34]), "root min != min of block 0"
    if args.full and not args.no_verify:
        samples = rig.capture_samples(st)
        timed = world == 1 and not args.no_cpu_baseline
        v, cpu_base = check_against_oracle(samples, args.cpu_budget, timed, ranks_here)
        verified += v
        if cpu_base is not None:
            kinds = [c[0][0].rsplit(" step", 1)[0] for c in samples]
            cpu_base["unit"] = "proofs/s"
            cpu_base["sample_wall_s"] = cpu_base.pop("single_leaf_latency_s")
            cpu_base["cpu_model"] = cpu_model()
            cpu_base["sample"] = (f"{len(samples)} framework proofs of the timed block ({', '.join(kinds)}: {sum(len(c) for c in samples)} prove() calls of 2^6..2^14 rows) re-proved "
                                  "from their captured witnesses by oracle/ (our C restatement, not the Rust prover), all hardware threads; every one compared bit for bit with "
                                  "the GPU's and verified (`latency_mode`). `value` = the best of `throughput_sweep` (the same proofs, P side by side x T threads each, in the table's proportion) "
                                  "and the latency mode. `medians`: the same oracle on one fixed prove() call, 5 runs with all threads and 5 with one thread")
            # the fixed unit of the medians: the final wrap step of the first sampled proof (2^12 rows: the shape every framework proof ends with)
            cpu_base["medians"] = cpu_medians(samples[0][-1])
            # the CPU's best configuration for this metric: proofs side by side. `value` = the maximum over the modes,
            # the one-proof-after-the-other figure stays as `latency_mode`
            lat = {"value": cpu_base["value"], "sample_wall_s": cpu_base["sample_wall_s"], "mode": "one framework proof after the other, every hardware thread inside each prove() "
                   "(the self-check's own run: its proofs are the ones compared bit for bit)"}
            best, sweep = cpu_throughput_modes(samples, farm, max(2.0, args.cpu_budget * 0.4))
            cpu_base["latency_mode"] = lat
            cpu_base["throughput_sweep"] = sweep
            if best["proofs_per_s"] > cpu_base["value"]:
                cpu_base["value"], cpu_base["mode"], cpu_base["cores"] = best["proofs_per_s"], best["mode"], best["concurrent_proofs"] * best["threads_per_proof"]
            else:
                cpu_base["mode"] = lat["mode"]
            cpu_base["oracle_build"] = oracle_build
    if args.full and dist is not None:
        v = torch.tensor([verified], device="cuda" if nccl else "cpu", dtype=torch.int64)
        dist.all_reduce(v)
        verified = int(v.item())

    # the whole-table multiset digest at BASELINE size (2^20 rows x 5 columns), device resident, timed once
    digest_ms = None
    if args.full and rank == 0:
        big = 1 << 20
        rng = np.random.default_rng(seed)
        d_ids = ctx.to_device(st["table"].col_ids)
        d_values = ctx.to_device(rng.integers(0, 1 << 32, size=(big, n_cols + 1, 8), dtype=np.uint32))
        d_unique = ctx.to_device(rng.integers(0, 1 << 32, size=(big, 1, 8), dtype=np.uint32))
        mp2.compute_table_row_digest_dev(ctx, d_ids, n_cols + 1, d_values, d_unique, 1, 1 << 12)
        t1 = time.perf_counter()
        mp2.compute_table_row_digest_dev(ctx, d_ids, n_cols + 1, d_values, d_unique, 1, big)
        digest_ms = (time.perf_counter() - t1) * 1e3
        for b_ in (d_ids, d_values, d_unique):
            b_.free()

    side = world == 1 and args.full  # the side legs run at N = 1 only (like cpu_baseline): the scaling runs time the table build and nothing else
    # a side leg that fails must not take the headline with it: its field then carries the error, `side_leg_errors` names it
    side_errors = []

    def guarded(name, fn):
        try:
            return fn()
        except BaseException as e:  # SystemExit of a failed self-check included
            import traceback
            traceback.print_exc()
            side_errors.append(name)
            return {"error": f"{type(e).__name__}: {e}"[:400]}

    legs = kernel_legs(ctx, mp2, C, VARIANT, args.hasher, rank) if args.full and rank == 0 else None
    shapes = params.shapes()
    mem_free, mem_total = ctx.mem_info()  # with every prover of the run still alive: what the planner's estimate is calibrated on
    setup_s, workers, host_threads, plan = rig.setup_s, len(rig.ctxs), rig.host_threads, rig.plan
    root_pis_out = [int(x) for x in cur[0][3]]
    waves = [[n_items, n_pr, (round(sec, 2) if sec is not None else None)] for n_items, n_pr, sec in st["build"].wave_log]
    glue = dict(rig.last_glue)
    if "worker_busy_s" in glue:
        glue["host_glue_share"] = round(1.0 - glue["inside_libmp2gpu_s"] / max(glue["worker_busy_s"], 1e-9), 4)
    else:
        glue["host_glue_share"] = round(1.0 - glue["inside_libmp2gpu_s"] / max(glue["block_s"], 1e-9), 4)  # registration (numpy) + the plan's waves
    del st
    perms_total = mp2.leaf_permutations_queued()  # everything this process hashed up to here (warm-up, timed block, checks, side legs so far): what a kernel trace of the run holds
    rig.close()

    # BASELINE configs[2] at full size, on workers of its own (the table's provers are gone: the two circuit families never share the GPU)
    config2 = None
    if side and args.config2_leaves > 0:
        def c2():
            r2 = WorkerRig(mods, local_rank, VARIANT, workers, args.table_batch, host_threads)
            try:
                out2 = config2_leg(r2, args.config2_leaves)
                f2, t2 = r2.ctx.mem_info()
                out2["device_memory_used_bytes"] = t2 - f2
                return out2
            finally:
                r2.close()
        config2 = guarded("config2", c2)

    # the table rate bracketed by base degree: every base circuit padded to 2^k rows + the reference's leaf gate set
    by_degree = None
    if side and args.degree_sweep:
        by_degree = {}
        def at_degree(k):
            # with the provers' shared scratch (the default) the full batch fits at every degree; provers with buffers of their own
            # (MP2G_SHARE_SCRATCH=0) halve the proofs in flight per degree step to keep the device memory constant
            bk = args.table_batch if sharding.scratch_is_shared() else max(4, args.table_batch >> max(0, k - 12))
            while True:
                try:
                    rk = TableRig(mods, local_rank, VARIANT, args.workers, bk, args.subtree, args.host_witness, ranks_here, pad_bits=k, group_rows=args.group_rows, native=args.native_build)
                    break
                except SystemExit:  # the resource plan refused this many proofs in flight at these shapes (row_full is a degree above the rest)
                    if bk <= 4:
                        raise
                    bk = max(4, 3 * bk // 4)
            try:
                # the full block up to k = 14 (1024 rows by default), half of it at k = 15 (a run there is 15 s as it is), never below 64 rows
                rows_k = max(min(64, args.sweep_rows), args.sweep_rows >> max(0, k - 14))
                rk.build(min(128, rows_k), 0, seed ^ 0x5A5A5A, n_cols, False)  # creates the provers and grows the scratch (4 x 48 proofs in flight: 640 proofs are several full batches)
                runs = []
                for rep in range(max(1, args.sweep_runs)):  # the same block proved again: one work plan each, the median reported
                    for c in rk.ctxs:
                        c.sync()
                    n0k = rk.n_proofs
                    t1 = time.perf_counter()
                    stk = rk.build(rows_k, 0, seed, n_cols, False)
                    for c in rk.ctxs:
                        c.sync()
                    dtk = time.perf_counter() - t1
                    runs.append(((rk.n_proofs - n0k) / dtk, dtk))
                    if rep == 0:
                        rk.check_root(stk, verify=not args.no_verify)
                    del stk
                # the first build after the provers were created still grows buffers to the block's size (round 5's three builds: 413 / 442 / 444
                # at k = 12): with three or more builds the median is reported, with two the LATER one (the steady state), both listed in order
                in_order = [round(v, 1) for v, _ in runs]
                val, dtk = sorted(runs)[len(runs) // 2] if len(runs) >= 3 else runs[-1]
                return {"value": val, "unit": "proofs/s", "rows": rows_k, "seconds": dtk, "median_of": len(runs), "runs": in_order,
                        "value_is": "the median of the builds" if len(runs) >= 3 else "the later of the two builds (the first still grows buffers): `runs` lists them in order",
                        "trace_rows_per_s": val / (n_cols + 1) * sum(sum(1 << d for d in rk.params.shapes()[nm]) * cnt for nm, cnt in
                                                                      (("cells_leaf", 2.0), ("cells_full", 1.0), ("cells_partial", 1.0), ("row_leaf", 0.5), ("row_full", 0.5))),
                        "batch": bk, "shapes": rk.params.shapes(), "setup_s": round(rk.setup_s, 1), "root_verified": not args.no_verify}
            finally:
                rk.close()

        for k in [int(x) for x in args.degree_sweep.split(",") if x]:
            by_degree[str(k)] = guarded(f"by_base_degree[{k}]", lambda k=k: at_degree(k))

    # the prove()-only loop on synthetic circuits (round 2's headline) beside it, briefly
    leaves = None
    if side and args.leaves_leg and not args.no_leaves_leg:
        import copy
        a2 = copy.copy(args)
        a2.steps, a2.warmup, a2.batch = 3, 1, 128
        leaves = guarded("leaves_prove_only", lambda: run_leaves(a2, rank, local_rank, world, dist, torch, VARIANT, clocks, brief=True))
    out = None
    full_rec = completed_table_record()
    if rank == 0:
        rows_per_s = (world * n_rows + world - 1) / dt
        depth = max(1, (n_rows - 1).bit_length())
        out = {"metric": "leaf proofs/sec (whole node) + NTT GB/s vs HBM peak, 2^20-row table build, 1/2/4/8 GPU",
               "value": n_total / dt, "unit": "proofs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": dt / max(1, args.steps) * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "u64 (Goldilocks field)", "data": "synthetic", "verified": verified,
               "rows_per_s": rows_per_s,
               "table_2p20_rows_extrapolated_s": (1 << 20) / rows_per_s + (digest_ms or 0) / 1e3,  # = the measured time when this run is the whole table
               "table_rows_total": world * n_rows + world - 1,  # the ranks' blocks and the separator rows between them
               "table_digest_2p20_rows_ms": digest_ms,
               "config": {"workload": f"table: configs[3], ONE contiguous block of {n_rows} rows per rank (= {args.steps} steps of {rows_per_step} rows" +
                                      f"; row tree {depth} levels deep, one work plan" + (f"; {world} blocks + {world - 1} separator rows = {world * n_rows + world - 1} rows, joined in {n_levels} level(s)" if world > 1 else "") + ") "
                                      f"-- per row {n_cols} cells-tree proofs (2 leaves, 1 full, 1 partial) + 1 row-tree proof (leaf / partial / full + the cells root through the "
                                      "cells-set verifier gadget), all REAL framework proofs = witness program + base prove() + wrap chain to 2^12 rows, witness check on; row tree "
                                      "scheduled by the batched UpdateTree work plan; the rows' multiset digests (map-to-curve, row ids, accumulation up both trees) inside the timed "
                                      "region; value = framework proofs/s (5 per row). " + ("THIS IS the full 2^20-row build of configs[3]" if world * n_rows >= 1 << 20 else
                                      full_table_note(full_rec)) + "; with --full: configs[2] at "
                                      "full size = `config2`; base degrees 12..15 = `by_base_degree`; roofline leg = configs[1] 2^22-point NTT",
                          "rows_per_rank": n_rows, "rows_per_step": rows_per_step, "row_tree_depth": depth, "warmup_rows_per_rank": warm_rows,
                          "value_columns": n_cols, "workers": workers, "batch": args.table_batch, "subtree_size": args.subtree, "group_rows": args.group_rows or 32 * args.table_batch, "pad_base_bits": args.pad_base_bits,
                          "lean": bool(lean), "host_orchestration": glue,  # the workers' time in the timed block: total, inside the C ABI (mp2g_chain_run), the rest = Python glue
                          "work_plan_waves": waves,  # (the native scheduler drains the plan inside the library and reports the items per wave only)  # per wave of the work plan: [items, framework proofs, seconds]
                          "witness_generation": "host threads (mp2g_witness_program_run_rows)" if args.host_witness else "device (mp2g_witness_program_run_dev: level-scheduled witness programs, one block per proof; base -> wrap hand-off by device copies)",
                          "host_threads_per_worker": host_threads, "host_cores": os.cpu_count(), "ranks_on_host": ranks_here, "shapes": shapes,
                          "host_peak_rss_bytes": __import__("resource").getrusage(__import__("resource").RUSAGE_SELF).ru_maxrss * 1024,
                          "leaf_sponge_permutations": leaf_perms, "leaf_sponge_permutations_process_total": perms_total,  # queued by this rank's timed block (mp2g_stat_leaf_permutations): per framework proof, x value = the sponge work per second
                          "device_memory_used_bytes": mem_total - mem_free_build, "device_memory_planned_bytes": plan["device_bytes_per_rank"],
                          "device_memory_note": "`used` = with every prover of the table build alive, before any side leg; the configs[2] leg runs on provers of its own after the table's are freed (round 4 kept both alive: its `used` was 33 GB above the plan)",
                          "setup_s": round(setup_s, 1), "hasher": "Poseidon2", "backend": (dist.get_backend() if dist is not None else None), "rccl_ranks": rccl_ranks,
                          "join_levels": n_levels,
                          "sharding": f"{world} rank(s): one block of rows each, no collective below the block roots; {n_levels} join level(s) move a root proof point to point "
                                      f"({sum(proof_sizes) * 8} B" + (")" if world == 1 else
                                          ", device to device over RCCL straight from the prover's buffers into the parent's device-side witness inputs; path chosen by the pre-timing probe: every join pair moved a libmp2gpu-allocated buffer)" if nccl and handoff["mode"] == "device" else
                                          f", STAGED: downloaded by the sender, sent as a torch tensor -- chosen before t0 because the pre-timing probe of the direct path failed: {handoff['reason']})" if handoff["mode"] == "staged" else
                                          ", host tensors over gloo; every join pair probed before t0)"),
                          "handoff": handoff,
                          "root_public_inputs": root_pis_out,
                          "verified": (f"{verified} prove() calls: on every rank the block root passes the oracle's verifier and one framework proof of every circuit kind of the timed "
                                       "block equals the CPU oracle's proofs of the same witnesses bit for bit and passes its verifier; the block roots expose the off-circuit "
                                       "tree hash, digest (= compute_table_row_digest of the block), min, max and the circuit-set digest") if args.full else
                                      "nothing checked: the self-check runs with --full"}}
        if args.full:
            out["clocks"] = clocks.read(local_rank)
        if full_rec is not None:  # the metric's named configuration, completed across calls (bench.py --resume-dir): a committed record, not this run
            out["table_2p20_rows_completed"] = full_rec
        if config2 is not None:
            out["config2"] = config2
        if by_degree is not None:
            out["by_base_degree"] = by_degree
        if leaves is not None:
            out["leaves_prove_only"] = leaves if "error" in leaves else {
                "value": leaves["value"], "unit": "leaf proofs/s (base 2^13 + wrap 2^12 prove() on synthetic circuits, resident witnesses: "
                "`--workload leaves`, round 2's headline)", "ms_per_step": leaves["ms_per_step"], "batch": 128}
        if side_errors:
            out["side_leg_errors"] = side_errors
        if legs is not None:
            out.update(legs)
        alu = out.get("roofline_alu")
        if alu is not None and alu.get("step_valu_wave_insts_per_framework_proof"):
            # the whole table build against the same peak: (every kernel's VALU wave-instructions per framework proof, a committed counter pass) x this run's proofs/s
            rate = out["value"] / world * alu["step_valu_wave_insts_per_framework_proof"]
            alu["table_build"] = {"valu_wave_insts_per_s_per_gpu": rate, "frac": rate / alu["peak_valu_wave_insts_per_s"],
                                  "how": "a committed counter pass (VALU wave-instructions per framework proof of a 512-row build, profiles/r05/step_counters_4workers.json) x THIS run's proofs/s: "
                                         "not an in-run counter measurement",
                                  "leg": "the headline: every kernel of the build (sponges 71 % of the instructions), four workers' streams overlapped",
                                  "over_the_sponge_alone": rate / alu["peak_valu_wave_insts_per_s"] / alu["frac_alone_clock_free"],
                                  "reading": "`over_the_sponge_alone`: the whole build's VALU issue rate over the leaf sponge's with the chip to itself, both at this run's clock: the build issues "
                                             "almost as fast as its dominant kernel alone -- the headline is bound by the instruction count, not by scheduling"}
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
        print(json.dumps(out))
    clocks.close()
    if dist is not None:
        dist.destroy_process_group()
    if side_errors:  # the headline stands (exit code 0); the line names the failed legs in `side_leg_errors` and in their own fields
        print(f"bench.py: side leg(s) failed: {', '.join(side_errors)}", file=sys.stderr)
    return out


FULL_TABLE_RECORD = os.path.join("profiles", "r05", "table_2p20_rows.json")


def completed_table_record():
    """the record of the completed 2^20-row build (bench.py --resume-dir, one GPU, several calls), if the repository holds one"""
    try:
        with open(os.path.join(ROOT, FULL_TABLE_RECORD)) as f:
            r = json.load(f)
        blocks = r["blocks"]
        rows_each = sorted({b.get("rows") for b in blocks if isinstance(b, dict)} - {None})
        return {"source": FULL_TABLE_RECORD + f" (bench.py --resume-dir: {len(blocks)} blocks" + (f" of {rows_each[0]} rows" if len(rows_each) == 1 else "") +
                          f" + {r['separator_rows']} separator rows built on one MI355X across calls; committed, not this run)",
                "table_rows_total": r["table_rows_total"], "framework_proofs": r["framework_proofs"], "gpu_seconds": r["gpu_seconds"], "value": r["value"], "unit": r["unit"],
                "join_levels": r["join_levels"], "verified": r["verified"],  # the record's own statement of what the completing call checked
                "root_proof_with_vk_fnv1a64": r["root_proof_with_vk_fnv1a64"]}
    except (OSError, ValueError, KeyError):
        return None


def full_table_note(rec):
    if rec is not None:
        return (f"The full table was built ONCE, block by block across calls on one GPU: {rec['table_rows_total']} rows, {rec['framework_proofs']} framework proofs in "
                f"{rec['gpu_seconds']:.0f} GPU-seconds = {rec['value']:.1f} proofs/s, root verified (`table_2p20_rows_completed`, {FULL_TABLE_RECORD}); this run times one block of it")
    return ("The full 2^20-row build does not fit one GPU in a bench run (extrapolated below); the one attempt as a single run is PARTIAL: "
            "profiles/r04/table_2p20_rows_progress.txt (56 % of the proofs at 852 proofs/s sustained when the call's time limit ended it; no root, nothing verified)")


def run_table_resumable(args, local_rank, VARIANT, clocks):
    """BASELINE configs[3] at FULL size on one GPU, across calls: the table is `--table-blocks` contiguous blocks of `--steps` x
    `--rows` rows (block b = the rows with prefix 2 b, exactly the blocks `--gpus N` deals to N ranks) plus the separator rows that
    join them (prefixes 2 s + 1). Every call builds the blocks that are not yet in the proof store (`--resume-dir`) for as long as
    `--max-seconds` allows -- a block = run_table's timed block: one work plan, 5 real framework proofs per row, the root checked
    against the off-circuit tree hash / digest / min / max and by the oracle's verifier before it is stored as ProofWithVK bytes
    (mp2g_proof_with_vk_serialize; the reference's harness does the same per node: mp2-v1/tests/common/rowtree.rs:78-337 with
    proof_storage.rs:139-140) --; the call that finds all blocks present takes them out of the store (mp2g_proof_with_vk_deserialize),
    proves the log2(blocks) join levels, verifies the root and writes the record. The single-GPU rehearsal of the 8-rank run."""
    assert VARIANT == 0
    t_call = time.perf_counter()
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    R = importlib.import_module("mapreduce-plonky2_amd.recursion")
    FW = importlib.import_module("mapreduce-plonky2_amd.framework")
    C = importlib.import_module("mapreduce-plonky2_amd.circuits")
    T = importlib.import_module("mapreduce-plonky2_amd.table")
    IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
    PS = importlib.import_module("mapreduce-plonky2_amd.proofstore")
    mods = (mp2, R, FW, C, T, IX)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits as OC
    import oracle as O
    n_cols, seed, blocks = 4, 0xC0FFEE04, args.table_blocks
    assert blocks >= 1 and blocks & (blocks - 1) == 0, "--table-blocks: a power of two (binary join levels)"
    n_rows, _, warm_rows = block_plan(args.rows, args.steps, args.warmup)
    table_id = f"synthetic_{seed:x}_{blocks}x{n_rows}"
    store = PS.ProofStore(args.resume_dir)
    rig = TableRig(mods, local_rank, VARIANT, args.workers, args.table_batch, args.subtree, False, 1, pad_bits=args.pad_base_bits,
                   group_rows=args.group_rows, native=args.native_build)
    params, ctx = rig.params, rig.ctx
    final_ckt = params.rows.chains["row_leaf"][-1][0]
    final_fp = FW.circuit_fri_params(final_ckt, VARIANT)
    n_pis = T.ROWS_IO + 4
    ints = lambda v: sum(int(x) << (32 * (7 - j)) for j, x in enumerate(v))

    def block_key(b, table):
        # RowProofIdentifier {table, primary, tree_key} (proof_storage.rs:41-46): the tree key of a block's root = the secondary-index value of its root row
        root, _, _ = T.balanced_bst(table.rows)
        return PS.ProofKey.row(table_id, 1, f"{ints(table.values[root, 0]):064x}")

    # ---- blocks: build what the store does not hold yet ---------------------------------------------------------------------
    tables = {b: T.SyntheticTable(n_rows, n_cols, seed, 2 * b) for b in range(blocks)}
    keys = {b: block_key(b, tables[b]) for b in range(blocks)}
    built, warm, est = [], False, None
    for b in range(blocks):
        if store.contains(keys[b]):
            continue
        elapsed = time.perf_counter() - t_call
        if est is not None and elapsed + 1.15 * est > args.max_seconds:
            break
        if not warm and warm_rows > 0:  # creates the provers of every circuit, outside the block's clock
            rig.build(warm_rows, 2 * b, seed ^ 0x5A5A5A, n_cols, warm_rows > 16384)
            warm = True
        for c in rig.ctxs:
            c.sync()
        n0, t0 = rig.n_proofs, time.perf_counter()
        st = rig.build(n_rows, 2 * b, seed, n_cols, n_rows > 16384)
        for c in rig.ctxs:
            c.sync()
        dt = time.perf_counter() - t0
        est = dt
        want, w_all = rig.check_root(st, verify=True)
        caps, openings, fri, pis = st["proof"]
        vk_cap, vk_dig = params.rows.vds[st["name"]]
        blob = mp2.serialize_proof_with_vk(mp2.serialize_proof(final_fp, final_ckt.num_constants, caps, openings, fri, pis), vk_cap, vk_dig)
        note = {"block": b, "prefix": 2 * b, "rows": n_rows, "framework_proofs": rig.n_proofs - n0, "gpu_seconds": dt, "proofs_per_s": (rig.n_proofs - n0) / dt,
                "circuit": st["name"], "digest_w": [int(x) for x in st["digest_w"]], "digest_weierstrass": [int(x) for x in pis[4:15]],
                "min": f"{ints(st['table'].values[0, 0]):064x}", "max": f"{ints(st['table'].values[-1, 0]):064x}", "root_verified_by_oracle": True,
                "clocks": clocks.read(local_rank), "library_sha16": lib_sha16(mp2.LIB_PATH), "workers": len(rig.ctxs), "batch": args.table_batch, "host": os.uname().nodename, "unix_time": time.time()}
        store.store_proof(keys[b], blob, note)
        built.append(b)
        print(f"bench.py: block {b} of {blocks}: {n_rows} rows, {rig.n_proofs - n0} framework proofs in {dt:.1f} s = {(rig.n_proofs - n0) / dt:.1f} proofs/s, root stored "
              f"({len(blob)} B)", file=sys.stderr, flush=True)
        del st
    missing = [b for b in range(blocks) if not store.contains(keys[b])]
    if missing:
        out = {"resume_dir": args.resume_dir, "blocks_built_this_call": built, "blocks_missing": missing, "call_seconds": time.perf_counter() - t_call}
        print(json.dumps(out))
        rig.close()
        clocks.close()
        return out

    # ---- every block is in the store: take the roots out, check each, prove the join levels ----------------------------------
    names = list(params.rows.circuits)
    by_digest = {tuple(int(x) for x in params.rows.vds[n][1]): n for n in names}
    cur, notes, ws = {}, {}, {}

    def stored_block_is_bad(b, why):
        # a stored root that fails its checks would block the join for ever: it is dropped, and the next call rebuilds that block
        store.remove(keys[b])
        rig.close()
        clocks.close()
        raise SystemExit(f"bench.py: the stored root of block {b} failed its check ({why}); it was removed from {args.resume_dir}: run the same command again to rebuild the block")

    for b in range(blocks):
        try:
            proof, vk_cap, vk_dig = mp2.deserialize_proof_with_vk(final_fp, final_ckt.num_constants, store.get_proof_exact(keys[b]), n_pis)
        except (mp2.Mp2gError, KeyError, ValueError) as e:
            stored_block_is_bad(b, f"not a ProofWithVK of this shape: {e}")
        name = by_digest[tuple(int(x) for x in vk_dig)]  # the verifier key names the circuit (KeyError: not a circuit of this set)
        assert np.array_equal(vk_cap.ravel(), np.asarray(params.rows.vds[name][0], dtype=np.uint64).ravel()), "stored verifier key: cap"
        pis = proof[3]
        # the stored root against the table, not against its note: digest of the block's rows, min / max, circuit-set digest; the oracle verifies it
        w_b, wei_b = mp2.compute_table_row_digest(ctx, tables[b].col_ids, tables[b].values, tables[b].values[:, 0:1])
        if not np.array_equal(wei_b, pis[4:15]):
            stored_block_is_bad(b, "its digest != compute_table_row_digest of the block")
        if not (np.array_equal(pis[26:34], T.u256_to_limbs([ints(tables[b].values[0, 0])])[0]) and np.array_equal(pis[34:42], T.u256_to_limbs([ints(tables[b].values[-1, 0])])[0])):
            stored_block_is_bad(b, "min / max")
        if not np.array_equal(pis[T.ROWS_IO:], np.asarray(params.rows.set_digest, dtype=np.uint64)):
            stored_block_is_bad(b, "circuit-set digest")
        wckt, _, wdig = params.rows.chains[name][-1]
        rc = OC.verify(wckt, OC.oracle_params(wckt), np.asarray(wdig, dtype=np.uint64), O.hash_n_to_m_no_pad(pis, 4), *proof[:3])
        if rc:
            stored_block_is_bad(b, f"the oracle's verifier rejects it (code {rc})")
        cur[b], notes[b], ws[b] = (proof, name, w_b), store.note(keys[b]), w_b
    for c in rig.ctxs:
        c.sync()
    n_levels, seps, t0 = blocks.bit_length() - 1, [], time.perf_counter()
    for lvl in range(n_levels):
        bit = 1 << lvl
        for b in range(0, blocks, 2 * bit):
            sep = 2 * (b + bit) - 1
            cur[b] = T.join_blocks(rig.join_build(), ctx, cur[b], cur[b + bit], sep, n_cols, seed, VARIANT)
            seps.append(sep)
    for c in rig.ctxs:
        c.sync()
    join_s = time.perf_counter() - t0
    root_proof, root_name, root_w = cur[0]
    root_pis = root_proof[3]
    for sp in seps:
        tb = T.SyntheticTable(1, n_cols, seed, sp)
        ws[-sp] = mp2.compute_table_row_digest(ctx, tb.col_ids, tb.values, tb.values[:, 0:1])[0]
    whole_w, whole_wei = mp2.curve_sum(ctx, np.stack([ws[k] for k in sorted(ws)]), weierstrass=True)
    assert np.array_equal(whole_wei, root_pis[4:15]), "root digest != compute_table_row_digest of the whole table (blocks and separator rows)"
    assert np.array_equal(root_pis[26:34], T.u256_to_limbs([ints(tables[0].values[0, 0])])[0]), "root min != the table's smallest secondary value"
    assert np.array_equal(root_pis[34:42], T.u256_to_limbs([ints(tables[blocks - 1].values[-1, 0])])[0]), "root max != the table's largest secondary value"
    assert np.array_equal(root_pis[T.ROWS_IO:], np.asarray(params.rows.set_digest, dtype=np.uint64)), "circuit-set digest"
    wckt, _, wdig = params.rows.chains[root_name][-1]
    rc = OC.verify(wckt, OC.oracle_params(wckt), np.asarray(wdig, dtype=np.uint64), O.hash_n_to_m_no_pad(root_pis, 4), *root_proof[:3])
    if rc:
        raise SystemExit(f"bench.py: the oracle's verifier rejects the table's root (code {rc})")
    vk_cap, vk_dig = params.rows.vds[root_name]
    root_blob = mp2.serialize_proof_with_vk(mp2.serialize_proof(final_fp, final_ckt.num_constants, *root_proof), vk_cap, vk_dig)
    store.store_proof(PS.ProofKey.row(table_id, 1, "root"), root_blob, {"rows": blocks * n_rows + len(seps), "circuit": root_name})
    block_s = sum(notes[b]["gpu_seconds"] for b in range(blocks))
    block_proofs = sum(notes[b]["framework_proofs"] for b in range(blocks))
    total_proofs, total_s = block_proofs + (n_cols + 1) * len(seps), block_s + join_s
    out = {"metric": "leaf proofs/sec (whole node) + NTT GB/s vs HBM peak, 2^20-row table build, 1/2/4/8 GPU",
           "value": total_proofs / total_s, "unit": "proofs/s", "n_gpus": 1, "higher_is_better": True, "dtype": "u64 (Goldilocks field)", "data": "synthetic",
           "table_rows_total": blocks * n_rows + len(seps), "framework_proofs": total_proofs, "gpu_seconds": total_s, "gpu_seconds_blocks": block_s,
           "gpu_seconds_join_levels": join_s, "join_levels": n_levels, "separator_rows": len(seps),
           "config": {"workload": f"table: configs[3] COMPLETED -- {blocks} contiguous blocks of {n_rows} rows + {len(seps)} separator rows = {blocks * n_rows + len(seps)} rows, "
                                  f"{total_proofs} real framework proofs ({n_cols} cells-tree + 1 row-tree per row: witness program + base prove() + wrap chain to 2^12 rows, witness check "
                                  "on), built block by block on ONE MI355X across calls; block roots kept as ProofWithVK bytes in a proof store between the calls, re-checked against "
                                  "the table and the oracle's verifier when taken out, then joined by log2(blocks) levels of separator rows; gpu_seconds = the sum of the blocks' "
                                  "timed regions (each as bench.py's timed block: barrier to barrier, provers created before) + the join levels",
                      "blocks": blocks, "rows_per_block": n_rows, "value_columns": n_cols, "workers": len(rig.ctxs), "batch": args.table_batch, "subtree_size": args.subtree,
                      "shapes": params.shapes(), "hasher": "Poseidon2", "table_id": table_id},
           "blocks": [{k: notes[b][k] for k in ("block", "rows", "framework_proofs", "gpu_seconds", "proofs_per_s", "circuit", "host", "unix_time", "clocks")} for b in range(blocks)],
           "root_circuit": root_name, "root_public_inputs": [int(x) for x in root_pis], "root_proof_with_vk_bytes": len(root_blob),
           "root_proof_with_vk_fnv1a64": f"{fnv1a64(root_blob):016x}",
           "root_digest_w": [int(x) for x in whole_w],
           "verified": "every stored block root: digest = compute_table_row_digest of its rows, min / max, circuit-set digest, the oracle's verifier; the table's root: "
                       "digest = compute_table_row_digest of all rows (blocks + separators), min of block 0, max of the last block, circuit-set digest, the oracle's verifier",
           "resume_dir": args.resume_dir, "blocks_built_this_call": built, "call_seconds": time.perf_counter() - t_call}
    rec = args.record or os.path.join(args.resume_dir, "table_record.json")
    with open(rec, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    rig.close()
    clocks.close()
    return out


def lib_sha16(path):
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in np.frombuffer(bytes(data), dtype=np.uint8).tolist():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def run_leaves(args, rank, local_rank, world, dist, torch, VARIANT, clocks, brief=False):
    """--workload leaves: prove() only, on synthetic circuits with resident witnesses (the module docstring's first paragraph). With
    `brief` (the table workload's side leg) nothing is verified or printed and the kernel legs are skipped: returns the line's dict."""
    mp2 = importlib.import_module("mapreduce-plonky2_amd")
    sharding = importlib.import_module("mapreduce-plonky2_amd.sharding")
    C = importlib.import_module("mapreduce-plonky2_amd.circuits")  # synthetic circuit + witness generator (pure Python)
    FW = importlib.import_module("mapreduce-plonky2_amd.framework")
    # several contexts = several HIP streams on the same GPU: the base and the wrap provers run concurrently, so
    # the latency-bound stretches of one (transcript, top Merkle levels) hide under the other's sponges
    ctx = mp2.Context(local_rank)
    n_ctx = max(1, args.streams)
    ctxs = [ctx] + [mp2.Context(local_rank) for _ in range(n_ctx - 1)]
    B = args.batch
    # provers: (shape, context, share of the batch). 1 stream: both shapes on it; 2: one each;
    # 4: every shape split into two half-batches
    if n_ctx >= 4:
        parts = n_ctx // 2  # streams per shape: every shape's batch is cut into that many parts
        sizes = [B * (k + 1) // parts - B * k // parts for k in range(parts)]
        plan = [(role, bits, ctxs[2 * k + j], sizes[k]) for k in range(parts) for j, (role, bits) in enumerate((("base", args.base_bits), ("wrap", 12)))]
    elif n_ctx >= 2:
        plan = [("base", args.base_bits, ctxs[0], B), ("wrap", 12, ctxs[1], B)]
    else:
        plan = [("base", args.base_bits, ctx, B), ("wrap", 12, ctx, B)]
    plan = [p for p in plan if p[3] > 0]

    # ---- synthetic inputs, resident in HBM before the timed region -----------------------------
    provers = []
    circuits = {}
    for pi, (role, k, cx, nb) in enumerate(plan):
        # a satisfied gate-level circuit of the role's gate set: rows dealt over the gates, random copy constraints
        if role not in circuits:
            circuits[role] = C.build(k, C.LEAF_KINDS if role == "base" else C.VERIFIER_KINDS, SEED + k + (0 if role == "base" else 100))
        ckt = circuits[role]
        cp = FW.CircuitProver(cx, ckt, nb, VARIANT, witness_check=args.witness_check, bind_public_inputs=True)
        wseed = SEED + 1000 * pi + 31 * rank
        d_w = FW.tile_witness(cx, ckt, nb, wseed)
        pi_hash = C.rand_field((nb, 4), wseed + 17)  # every proof has its own public inputs
        d_ph = cx.to_device(pi_hash)
        staging = []
        if args.host_inputs:
            view, hptr = cx.host_alloc(d_w.nbytes)
            view[:] = np.frombuffer(d_w.download((d_w.nbytes // 8,)).tobytes(), dtype=np.uint8)
            staging.append((d_w, hptr, d_w.nbytes))
        provers.append((cp, d_w, d_ph, cx, staging, wseed, pi_hash, role))
    def step():
        for cp, d_w, d_ph, cx, staging, *_ in provers:
            for buf, hptr, nbytes in staging:
                cx.h2d_async(buf, hptr, nbytes)
            cp.prove(d_w, d_ph)

    def sync_all():
        for c in ctxs:
            c.sync()

    for _ in range(args.warmup):
        step()
    sync_all()

    legs = None if brief else kernel_legs(ctx, mp2, C, VARIANT, args.hasher, rank)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        sync_all()

    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync_all()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device="cuda" if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    if args.witness_check:
        for cp, *_ in provers:
            cp.pr.witness_status()  # raises on a violated constraint

    # ---- self-check: sampled proofs of the LAST timed step vs the CPU oracle (also the cpu_baseline sample) ------
    verified, cpu_base = 0, None
    if not args.no_verify and not brief:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle as O
        results = [cp.results() for cp, *_ in provers]

        def sample(idx, b, mandatory):
            cp, _, _, _, _, wseed, pi_hash, role = provers[idx]
            ofp = O.standard_params(cp.ckt.log_n, (int(cp.ckt.pre.shape[0]), 135, 20, 16), variant=VARIANT)
            caps, openings, proofs = results[idx]
            return (f"{role} prover {idx} proof {b}", cp.ckt, ofp, cp.circuit_digest, lambda: FW.witness_of(cp.ckt, wseed, b, pi_hash[b]),
                    pi_hash[b], caps[b], openings[b], proofs[b], mandatory)

        # a leaf proof = the base and the wrap proof with the same batch index of a (base, wrap) prover pair; the first
        # and the last index of every pair are mandatory, further ones follow while the CPU budget lasts
        base_ids = [i for i, pv in enumerate(provers) if pv[7] == "base"]
        wrap_ids = [i for i, pv in enumerate(provers) if pv[7] == "wrap"]
        samples, rounds = [], 0
        while len(samples) < 64:
            added = False
            for ib, iw in zip(base_ids, wrap_ids):
                nb = min(provers[ib][0].batch, provers[iw][0].batch)
                order = [0, nb - 1] + list(range(1, nb - 1))
                order = order[:nb] if nb > 1 else [0]
                if rounds < len(order):
                    b = order[rounds]
                    samples.append([sample(ib, b, rounds < 2), sample(iw, b, rounds < 2)])
                    added = True
            rounds += 1
            if not added:
                break
        samples.sort(key=lambda leaf: not leaf[0][-1])
        timed = world == 1 and not args.no_cpu_baseline
        # every rank checks its own proofs; the timed sample is rank 0 at N=1 only
        verified, cpu_base = check_against_oracle(samples, args.cpu_budget, timed, int(os.environ.get("LOCAL_WORLD_SIZE", world)))

    # per-stage split of one batch per shape, each prover alone on the GPU (outside the timed region)
    stages = {}
    if rank == 0 and not brief:
        seen_shapes = set()
        for (role, k, cx, nb), (cp, d_w, d_ph, *_rest) in zip(plan, provers):
            if role in seen_shapes:
                continue
            seen_shapes.add(role)
            sync_all()
            cp.pr.enable_timing(True)
            cp.prove(d_w, d_ph)
            ms = cp.pr.stage_ms()
            cp.pr.enable_timing(False)
            stages[f"{role} 2^{k} x {nb}"] = {s: round(v, 3) for s, v in ms.items()}

    # the per-rank multiset digest (2^16 rows x 4 value columns, device resident) meets in one
    # all_gather of one encoded point per rank, outside the per-proof path
    rows, n_cols = (1 << 16, 4) if not brief else (256, 4)
    rng = np.random.default_rng(0xC0FFEE04 + rank)
    d_ids = ctx.to_device(C.rand_field(n_cols, 0xC0FFEE04))
    d_values = ctx.to_device(rng.integers(0, 1 << 32, size=(rows, n_cols, 8), dtype=np.uint32))
    d_unique = ctx.to_device(rng.integers(0, 1 << 32, size=(rows, 1, 8), dtype=np.uint32))
    mp2.compute_table_row_digest_dev(ctx, d_ids, n_cols, d_values, d_unique, 1, rows)
    t1 = time.perf_counter()
    w = mp2.compute_table_row_digest_dev(ctx, d_ids, n_cols, d_values, d_unique, 1, rows)
    digest_s = time.perf_counter() - t1
    if dist is not None and not brief:
        allw = sharding.all_gather_words(dist, w, device=torch.device("cuda", local_rank) if dist.get_backend() == "nccl" else None)
        w = mp2.curve_sum(ctx, allw)
        v = torch.tensor([verified], device="cuda" if dist.get_backend() == "nccl" else "cpu", dtype=torch.int64)
        dist.all_reduce(v)
        verified = int(v.item())

    out = None
    if rank == 0:
        out = {
            "metric": "leaf proofs/sec (whole node) + NTT GB/s vs HBM peak, 2^20-row table build, 1/2/4/8 GPU",
            "value": world * args.steps * B / dt,
            "unit": "leaf proofs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u64 (Goldilocks field)", "data": "synthetic",
            "verified": verified,
            "config": {"workload": f"configs[3]-shaped leaf proofs, steady state after witness generation: base 2^{args.base_bits} + wrap 2^12 prove() from "
                                   "the wire matrix (commitments, permutation argument, quotient with gate constraints, Fiat-Shamir, openings, FRI) at "
                                   "standard_recursion_config; base circuit = 19 gates (recursive-verifier set + u32 / comparison logic), wrap circuit = the 13 "
                                   "gates of plonky2's recursive verifier; every proof has its own public inputs and free cells; "
                                   "roofline leg = configs[1] 2^22-point NTT",
                       "batch_per_rank": B, "streams": args.streams, "witness_check": bool(args.witness_check), "host_inputs": bool(args.host_inputs),
                       "oracle_polys": {r: [int(c.pre.shape[0]), 135, 20, 16] for r, c in circuits.items()},
                       "gates": {r: len(c.gates) for r, c in circuits.items()}, "hasher": "Poseidon2" if VARIANT == 0 else "Poseidon (original_poseidon feature)",
                       "sharding": f"{world} rank(s), leaf proofs independent, digest all_gather 160 B",
                       "verified": f"{verified} sampled GPU proofs (first and last of every prover's batch on every rank, then more while the CPU budget "
                                   "lasts) equal the CPU oracle's proofs of the same witnesses bit for bit and pass its verifier"},
            "stage_ms": stages,
            "clocks": clocks.read(local_rank),
            "digest_rows_per_s": rows / digest_s,
            "digest_check": [int(x) for x in w],
        }
        if legs is not None:
            out.update(legs)
        # (no roofline_alu.table_build here: the instructions-per-framework-proof counter was taken on the TABLE build, and this workload
        # proves synthetic circuits with resident witnesses -- only run_table multiplies it with a rate)
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
        if not brief:
            print(json.dumps(out))
    for cp, *_ in provers:
        cp.free()
    if not brief:
        clocks.close()
        if dist is not None:
            dist.destroy_process_group()
    for c in reversed(ctxs):
        c.close()
    return out


if __name__ == "__main__":
    main()
