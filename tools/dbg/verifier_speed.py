"""Time the device verifier at the wrap shape (the table of profiles/verifier/README.md): one JSON line.
    python tools/dbg/verifier_speed.py            (MP2G_LIB selects another build of the library)
The recursive verifier's gate set at 2^12 rows under standard_recursion_config; one proved batch of 48, replicated on the device to
1024 proofs; mp2g_verifier_verify_dev over 1, 48 and 1024 of them, device events, median of 5 after 2 warm-up calls."""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
mp2 = importlib.import_module("mapreduce-plonky2_amd")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
import circuits as C

ctx = mp2.Context(0)
ckt = C.build(12, C.VERIFIER_KINDS, 3)
B = 48
cp = FW.CircuitProver(ctx, ckt, B, 0)
d_w = FW.tile_witness(ctx, ckt, B, 0x5EED, rand_row=True)
ph = np.tile(np.asarray(ckt.pi_hash, dtype=np.uint64), (B, 1))
d_ph = ctx.to_device(ph)


def timed(f, reps=5, warm=2):
    ms = []
    for i in range(warm + reps):
        ctx.timer_start(); f(); t = ctx.timer_stop()
        if i >= warm: ms.append(t)
    return ms


out = {}
all_ms = timed(lambda: (cp.prove(d_w, d_ph), ctx.sync()))
out["prove_48_ms"], out["prove_48_all"] = float(np.median(all_ms)), all_ms
caps, openings, proofs = cp.results()
cv = cp.verifier(capacity=1024)
words = np.tile(cv.pack(caps, openings, proofs, ph), (22, 1))[:1024]
d_words = ctx.to_device(np.ascontiguousarray(words))
pw, parts = cv.v.proof_words, cv.v.part_words
offs = np.concatenate([[0], np.cumsum(parts)[:3]])
d_parts = [d_words.ptr.value + 8 * int(o) for o in offs]
for count in (1024, 48, 1):
    status = []
    all_ms = timed(lambda: status.append(cv.v.verify_dev(d_parts, [pw] * 4, count)))
    assert all((s == 0).all() for s in status), "the verifier rejected a valid proof"
    out[f"verify_{count}_ms"], out[f"verify_{count}_all"] = float(np.median(all_ms)), all_ms
out["proof_words"] = int(pw)
out["lib"] = os.path.basename(os.path.dirname(mp2.LIB_PATH))
print(json.dumps(out))
