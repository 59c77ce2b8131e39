"""Stored proofs as nodes of a forest (csrc/forest.hip: mp2g_forest_put_proofs, mp2g_forest_proofs, mp2g_forest_staging_words): the
words that go in come out, through one staging chunk and across the chunk boundary, from aligned and unaligned slots; every refusal
returns an error code, registers nothing and gives every slot back. The words here are canonical random values, not proofs: a proof as
a child of a real node is tests/test_gpu_table_update.py's subject."""
import ctypes
import importlib
import threading

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
T = importlib.import_module("mapreduce-plonky2_amd.table")
R = importlib.import_module("mapreduce-plonky2_amd.recursion")
FW = importlib.import_module("mapreduce-plonky2_amd.framework")
IX = importlib.import_module("mapreduce-plonky2_amd.indexing")
BASE = 1 << 50  # ids of the external nodes: no row or cells-tree node of a small table


@pytest.fixture(scope="module")
def params(ctx):
    prover = FW.GpuProver(ctx, capacity=4)
    p = T.TableParams(prover, FW.circuit_fri_params, IX.empty_poseidon_hash(ctx))
    yield p
    prover.free()


@pytest.fixture(scope="module")
def nb(ctx, params):
    b = T.NativeTableBuild(params, [params.cells.prover], batch=4, subtree_size=4, group_rows=4)
    b.slot_words = max(b.pw_cells, b.pw_rows)
    yield b
    b.free()


def forest(mp2, nb, pool):
    return mp2.Forest([nb.provers[0].ctx], nb.desc, nb.chains, nb.slot_words, pool)


def unknown(mp2, F, ids):
    for i in ids:
        with pytest.raises(mp2.Mp2gError, match="unknown node"):
            F.proof_words(i)
    return True


def raw_put(mp2, F, ids, words, stride, n_words, keep=None):
    """the bare library call: (return code, message)"""
    ids, words, n_words = mp2._arr(ids), mp2._arr(words), mp2._arr(n_words, np.uint32)
    rc = mp2.load().mp2g_forest_put_proofs(F.h, int(ids.size), mp2._p(ids), mp2._p(words), int(stride), mp2._p(n_words), keep)
    return rc, mp2.load().mp2g_last_error().decode()


@pytest.mark.parametrize("which", ["1", "255", "257", "slot"])
def test_one_proof_round_trip(ctx, mp2, nb, which):
    n = nb.slot_words if which == "slot" else int(which)
    F = forest(mp2, nb, 3)
    words = O.rand_field(n, 0x1390 + n)
    for k in range(3):  # three slots: whatever slot_words is, an even and an odd slot number are both used
        F.put_proofs([BASE + k], [words[::-1] if k else words], keep=[1])
        assert F.free_slots == 3 - k - 1
    assert np.array_equal(F.proof_words(BASE), words) and np.array_equal(F.proof_words(BASE + 2), words[::-1])
    got = F.proofs([BASE + 2, BASE, BASE + 1])
    assert [g.size for g in got] == [n] * 3
    assert np.array_equal(got[1], words) and np.array_equal(got[0], words[::-1]) and np.array_equal(got[2], words[::-1])
    assert F.device_proof(BASE)[1] == n and F.proved == 0
    for k in range(3):
        F.release(BASE + k)
    assert F.free_slots == 3
    with pytest.raises(mp2.Mp2gError, match="released"):
        F.proofs([BASE])
    F.free()


def test_across_the_staging_chunk(ctx, mp2, nb):
    """total words = the staging chunk and one proof more: two chunks up, two chunks down, proofs of every parity of length and slot"""
    S, W = mp2.forest_staging_words(), nb.slot_words
    padded = lambda ns: sum((n + 1) & ~1 for n in ns)  # a proof starts at an even word of the staging buffer
    lens = [W, W - 1, W - 2]
    while padded(lens) <= S:
        lens.append(W)
    count = len(lens)
    assert padded(lens) - S <= W + 1 and count >= 4  # the second chunk holds the last proof alone
    F = forest(mp2, nb, count + 2)
    before = F.free_slots
    proofs = [O.rand_field(n, 0xA000 + i) for i, n in enumerate(lens)]
    ids = [BASE + 7 * i for i in range(count)]
    F.put_proofs(ids, proofs)
    assert F.free_slots == before - count and F.proved == 0
    got = F.proofs(ids)
    for i, g, p in zip(ids, got, proofs):
        assert np.array_equal(g, p) and np.array_equal(F.proof_words(i), p), i
    # more ids than one chunk holds, some twice, in another order
    order = ids[::-1] + ids[:3]
    again = F.proofs(order)
    want = dict(zip(ids, proofs))
    assert all(np.array_equal(g, want[i]) for i, g in zip(order, again))
    for i in ids:
        F.release(i)
    assert F.free_slots == before
    F.free()


def test_bulk_download_of_proved_nodes(ctx, mp2, nb):
    """after a 5-row build: Forest.proofs of the kept rows and cells roots = proof_words of each, also when the list crosses a chunk"""
    n = 5
    table = T.SyntheticTable(n, 4, seed=0xC0FFEE04, block=4)
    root, nodes, spans = T.balanced_bst(n)
    wit = T.TableWitness(ctx, table, spans)
    nb.run(table, wit, root, nodes, keep=range(n))
    assert nb.forest.proved == 5 * n
    ids = list(range(n)) + [nb.cell_id(k, T.sbbst_root(4)) for k in range(n)]
    one_by_one = [nb.forest.proof_words(i) for i in ids]
    assert {w.size for w in one_by_one} == {nb.pw_cells, nb.pw_rows}
    assert all(np.array_equal(a, b) for a, b in zip(nb.forest.proofs(ids), one_by_one))
    reps = mp2.forest_staging_words() // (len(ids) * min(nb.pw_cells, nb.pw_rows)) + 1  # more words than one chunk holds
    assert all(np.array_equal(a, b) for a, b in zip(nb.forest.proofs(ids * reps + ids[::-1]), one_by_one * reps + one_by_one[::-1]))
    # a cells-tree leaf was returned to the pool when its parent was proved: the whole call fails, nothing is written
    lib = mp2.load()
    bad_ids = mp2._arr([ids[0], nb.cell_id(0, 1)])
    out, lens = np.full((2, nb.slot_words), 7, dtype=np.uint64), np.full(2, 9, dtype=np.uint32)
    assert lib.mp2g_forest_proofs(nb.forest.h, mp2._p(bad_ids), 2, mp2._p(out), nb.slot_words, mp2._p(lens)) != 0
    assert b"released" in lib.mp2g_last_error() and (out == 7).all() and (lens == 9).all()
    bad_ids[1] = 12345
    assert lib.mp2g_forest_proofs(nb.forest.h, mp2._p(bad_ids), 2, mp2._p(out), nb.slot_words, mp2._p(lens)) != 0
    assert b"unknown node" in lib.mp2g_last_error() and (out == 7).all() and (lens == 9).all()
    # rows too short for a proof
    assert lib.mp2g_forest_proofs(nb.forest.h, mp2._p(bad_ids), 1, mp2._p(out), nb.pw_rows - 1, mp2._p(lens)) != 0
    assert (out == 7).all() and (lens == 9).all()
    # a unit that lists an external node is refused like any proved node; the node is not counted as proved
    w = O.rand_field(9, 3)
    if nb.forest.free_slots:
        nb.forest.put_proofs([BASE], [w])
        with pytest.raises(mp2.Mp2gError, match="already proved"):
            nb.forest.prove([[BASE]])
        assert nb.forest.proved == 5 * n and np.array_equal(nb.forest.proofs([BASE])[0], w)
    else:
        pytest.fail("the build's pool has no free slot left")


def test_refusals_register_nothing(ctx, mp2, nb):
    W, S = nb.slot_words, mp2.forest_staging_words()
    count = S // W + 1
    F = forest(mp2, nb, count + 1)
    F.put_proofs([BASE], [O.rand_field(5, 1)], keep=[1])
    free = F.free_slots
    assert free == count
    proofs = np.stack([O.rand_field(W, 0xB000 + i) for i in range(count)])
    ids = [BASE + 1 + i for i in range(count)]

    def refused(rc_msg, *needles):
        rc, msg = rc_msg
        assert rc != 0 and all(s in msg for s in needles), msg
        assert F.free_slots == free and unknown(mp2, F, [i for i in ids if i != BASE])

    # an id the forest knows, alone and behind good ones; an id listed twice
    refused(raw_put(mp2, F, [BASE], proofs[:1], W, [W]), "registered twice", str(BASE))
    refused(raw_put(mp2, F, ids[:2] + [BASE], proofs[:3], W, [W] * 3), "registered twice", str(BASE))
    refused(raw_put(mp2, F, [ids[0], ids[1], ids[0]], proofs[:3], W, [W] * 3), "registered twice", str(ids[0]))
    # lengths
    refused(raw_put(mp2, F, ids[:2], proofs[:2], W, [W, 0]), str(ids[1]), "0 words")
    refused(raw_put(mp2, F, ids[:2], np.zeros((2, W + 1), dtype=np.uint64), W + 1, [W, W + 1]), str(ids[1]), f"{W + 1} words")
    refused(raw_put(mp2, F, ids[:2], proofs[:2], W - 1, [W - 1, W]), str(ids[1]), f"{W - 1}")
    # the pool: count + 1 proofs for count free slots
    more = np.concatenate([proofs, proofs[:1]])
    refused(raw_put(mp2, F, ids + [BASE + 999], more, W, [W] * (count + 1)), f"need {count + 1} pool slots", f"{count} are free")
    with pytest.raises(mp2.Mp2gError, match="pool slots"):
        F.put_proofs(ids + [BASE + 999], more)
    # a word that is not canonical: the last word of the last proof of a call of two chunks
    for word in (O.P, (1 << 64) - 1):
        bad = proofs.copy()
        bad[-1, -1] = np.uint64(word)
        refused(raw_put(mp2, F, ids, bad, W, [W] * count), "not canonical", str(ids[-1]))
    # ... and the first such id is the one named: the first chunk's second proof beside the last chunk's last
    bad = proofs.copy()
    bad[1, W // 2], bad[-1, -1] = np.uint64(O.P), np.uint64(O.P + 5)
    refused(raw_put(mp2, F, ids, bad, W, [W] * count), "not canonical", str(ids[1]))
    # p - 1 is canonical: the same call goes through, and the forest was usable all along
    ok = proofs.copy()
    ok[-1, -1] = np.uint64(O.P - 1)
    F.put_proofs(ids, ok)
    assert F.free_slots == 0 and all(np.array_equal(a, b) for a, b in zip(F.proofs(ids), ok))
    for i in ids:
        F.release(i)
    assert F.free_slots == free
    F.free()


def test_no_import_while_proving(ctx, mp2, nb):
    """mp2g_forest_put_proofs is refused while mp2g_forest_prove runs (the node index must not grow beneath the workers), and goes
    through once it has returned"""
    n = 2
    table = T.SyntheticTable(n, 4, seed=0xC0FFEE04, block=4)
    root, nodes, spans = T.balanced_bst(n)
    wit = T.TableWitness(ctx, table, spans)
    F = forest(mp2, nb, 16)
    old, nb.forest = nb.forest, F
    nb.register(table, wit, root, nodes, keep={root})
    nb.forest = old
    unit = [nb.cell_id(k, c) for k in range(n) for c in range(1, 5)] + list(range(n))
    w = O.rand_field(33, 9)
    errors = []

    def work():
        try:
            F.prove([unit])
        except Exception as e:  # reported below
            errors.append(e)

    before = F.free_slots
    t = threading.Thread(target=work)
    t.start()
    while F.free_slots == before and t.is_alive():  # the first batch of the unit has taken its slots: the call is well inside
        pass
    rc, msg = raw_put(mp2, F, [BASE], w, 33, [33])
    running = t.is_alive()
    t.join()
    assert not errors, errors
    assert running and rc != 0 and "mp2g_forest_prove is running" in msg, (running, rc, msg)
    assert F.proved == 5 * n and unknown(mp2, F, [BASE])
    free = F.free_slots
    F.put_proofs([BASE], [w])
    assert F.free_slots == free - 1 and np.array_equal(F.proof_words(BASE), w) and F.proved == 5 * n
    F.free()
