"""The Ecgfp5 group kernels (csrc/ec_curve.cuh, csrc/ecgfp5.hip) on the structured cases of tests/ec_cases.py, bit for bit against
the CPU oracle: equal operands and cancellations at every level of the sums' LDS trees, in the lane-serial loops and across the
two passes, row counts at which sum_kernel's lanes take a second point, scalars at the recoding's limb carries, simple_swu on the
sgn0 ladder, whole sponge blocks and the empty input, and encodings that must be refused. tests/test_ec_cases.py checks the same
cases on the references alone."""
import numpy as np
import pytest

import ec_cases as K
import oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(K.SUM_LABELS)), ids=lambda i: K.SUM_LABELS[i].replace(" ", "_"))
def test_curve_sum_structured(ctx, mp2, i):
    label, pts = K.sum_cases()[i]
    want = K.orc_sum(pts)
    got = mp2.curve_sum(ctx, pts, weierstrass=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), label
    if "inverse pairs only" in label:
        assert not got[0].any() and got[1].tolist() == [0] * 10 + [1]


@pytest.mark.parametrize("k", range(len(K.BIG_LABELS)), ids=lambda k: K.BIG_LABELS[k].replace(" ", "_"))
def test_curve_sum_lane_serial_loop_and_strided_second_pass(ctx, mp2, k):
    """16384 points are 128 block partials, 16385 make the second pass stride; 131072 points fill the capped grid once, 131073
    give lane 0 a second point, 140001 give one to 8929 lanes; the last case cancels inside one lane's serial loop"""
    pts, terms = K.big_sum_case(k)
    want = K.big_sum_expected(terms)
    got = mp2.curve_sum(ctx, pts, weierstrass=True)
    assert want[0].any()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_curve_sum_ranges_structured(ctx, mp2):
    pts, ranges = K.range_cases()
    w, wei = mp2.curve_sum_ranges(ctx, pts, ranges)
    for k, (lo, hi) in enumerate(ranges):
        want = K.orc_sum(pts[lo:hi])
        assert np.array_equal(w[k], want[0]) and np.array_equal(wei[k], want[1]), (lo, hi)
        if lo == hi:
            assert not w[k].any() and wei[k].tolist() == [0] * 10 + [1]
    # one range alone, and the ranges in reverse order: a block's result does not depend on its neighbours
    w1, wei1 = mp2.curve_sum_ranges(ctx, pts, ranges[-1:])
    assert np.array_equal(w1[0], w[-1]) and np.array_equal(wei1[0], wei[-1])
    wr, weir = mp2.curve_sum_ranges(ctx, pts, ranges[::-1])
    assert np.array_equal(wr[::-1], w) and np.array_equal(weir[::-1], wei)


@pytest.mark.parametrize("count", K.SCALAR_COUNTS)
def test_scalar_mul_structured(ctx, mp2, count):
    pts, ks = K.scalar_cases()
    want_w, want_wei = K.scalar_expected()
    w, wei = mp2.scalar_mul_batch(ctx, pts[:count], ks[:count], weierstrass=True)
    bad = [i for i in range(count) if not (np.array_equal(w[i], want_w[i]) and np.array_equal(wei[i], want_wei[i]))]
    assert not bad, (bad, [hex(ks[i]) for i in bad])
    # scalar 0 on P and on -P, and the neutral base: the neutral point in both forms
    for i in (0, 34, 73, 74, 75, 76):
        assert not w[i].any() and wei[i].tolist() == [0] * 10 + [1], i
    assert np.array_equal(mp2.scalar_mul_batch(ctx, pts[:count], ks[:count]), want_w[:count])


def test_swu_structured(ctx, mp2):
    u = K.swu_inputs()
    w, wei = mp2.swu_batch(ctx, u, weierstrass=True)
    ow, owei = K.orc_swu(u)
    bad = [i for i in range(len(u)) if not (np.array_equal(w[i], ow[i]) and np.array_equal(wei[i], owei[i]))]
    assert not bad, (bad, u[bad[:4]].tolist())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("in_len", [0, 8, 16, 24])
def test_map_to_curve_whole_sponge_blocks(ctx, mp2, variant, in_len):
    """in_len a whole number of rate-8 blocks; in_len = 0 maps the untouched zero state, the same point for every row"""
    for count in (1, 128, 129):
        ins = O.rand_field((count, in_len), 0xEC20 + in_len) if in_len else np.zeros((count, 0), dtype=np.uint64)
        w, wei = mp2.map_to_curve_batch(ctx, ins, variant, weierstrass=True)
        ow, owei = K.orc_map(ins, variant)
        assert np.array_equal(w, ow) and np.array_equal(wei, owei), count
        assert np.array_equal(mp2.map_to_curve_batch(ctx, ins, variant), ow)
        if in_len == 0:
            zw, zwei = K.orc_swu(np.zeros((1, 5), dtype=np.uint64))
            assert w[0].any() and (w == zw[0]).all() and (wei == zwei[0]).all()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("rows", [128, 129])
def test_row_digests_without_columns(ctx, mp2, variant, rows):
    """n_cols = 0: every row's digest is row_id * neutral, the neutral point, whatever the unique columns hold"""
    rng = np.random.default_rng(rows)
    col_ids = np.zeros(0, dtype=np.uint64)
    values = np.zeros((rows, 0, 8), dtype=np.uint32)
    unique = rng.integers(0, 1 << 32, size=(rows, 2, 8), dtype=np.uint32)
    ow, owei = np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    O.lib().orc_row_digest_batch(variant, O.p(col_ids), O.sz(0), O.p(values), O.p(unique), O.sz(2), O.sz(rows), O.p(ow), O.p(owei))
    assert not ow.any() and owei.tolist() == [0] * 10 + [1]
    w, wei = mp2.compute_table_row_digest(ctx, col_ids, values, unique, variant)
    assert np.array_equal(w, ow) and np.array_equal(wei, owei)
    ws, weis = mp2.row_digests(ctx, col_ids, values, unique, variant)
    assert ws.shape == (rows, 5) and not ws.any() and (weis == owei).all()


@pytest.mark.parametrize("rows", [128, 129])
def test_row_digests_full_and_one_lane_last_block(ctx, mp2, rows):
    rng = np.random.default_rng(1000 + rows)
    n_cols, n_unique = 2, 1
    col_ids = O.rand_field(n_cols, 0xEC30)
    values = rng.integers(0, 1 << 32, size=(rows, n_cols, 8), dtype=np.uint32)
    unique = np.ascontiguousarray(values[:, :n_unique, :])
    ow, owei = np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    O.lib().orc_row_digest_batch(0, O.p(col_ids), O.sz(n_cols), O.p(values), O.p(unique), O.sz(n_unique), O.sz(rows), O.p(ow), O.p(owei))
    w, wei = mp2.compute_table_row_digest(ctx, col_ids, values, unique)
    assert np.array_equal(w, ow) and np.array_equal(wei, owei)
    ws, weis = mp2.row_digests(ctx, col_ids, values, unique)
    # the last row alone, through the oracle; and the per-row terms sum to the table's digest
    lw, lwei = np.zeros(5, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    O.lib().orc_row_digest_batch(0, O.p(col_ids), O.sz(n_cols), O.p(np.ascontiguousarray(values[-1:])), O.p(np.ascontiguousarray(unique[-1:])),
                                 O.sz(n_unique), O.sz(1), O.p(lw), O.p(lwei))
    assert np.array_equal(ws[-1], lw) and np.array_equal(weis[-1], lwei)
    total = K.orc_sum(ws)
    assert np.array_equal(total[0], ow) and np.array_equal(total[1], owei)


def entry_points(ctx, mp2, pts):
    """the three entries that decode caller-given encodings, as thunks; the range leaves out both ends of the batch"""
    n = len(pts)
    rng = (1, 2) if n > 2 else (0, 0)
    return {"curve_sum": lambda: mp2.curve_sum(ctx, pts),
            "curve_sum_ranges": lambda: mp2.curve_sum_ranges(ctx, pts, [rng]),
            "scalar_mul_batch": lambda: mp2.scalar_mul_batch(ctx, pts, [3] * n)}


def test_valid_batch_is_accepted(ctx, mp2):
    for name, call in entry_points(ctx, mp2, K.refusal_batch()).items():
        call()


@pytest.mark.parametrize("index", K.REFUSAL_INDICES)
def test_invalid_encoding_is_refused_wherever_it_sits(ctx, mp2, index):
    """one canonical encoding that is no point, in the first block, at the end of it, alone at the start of the second, and in the
    partial last block; curve_sum_ranges decodes the whole array, so a range that leaves the bad index out is refused too"""
    pts = K.refusal_batch()
    pts[index] = K.bad_encodings(4)[K.REFUSAL_INDICES.index(index)]
    for name, call in entry_points(ctx, mp2, pts).items():
        with pytest.raises(mp2.Mp2gError, match="invalid point encoding"):
            call()


@pytest.mark.parametrize("k", range(16))
def test_noncanonical_encoding_is_refused(ctx, mp2, k):
    """a limb >= p is refused on the host, alone and at index 299 of a valid batch; (p, 0, 0, 0, 0) is not the neutral point"""
    row = K.NONCANONICAL[k]
    batch = K.refusal_batch()
    batch[299] = row
    for pts in (row.reshape(1, 5), batch):
        for name, call in entry_points(ctx, mp2, pts).items():
            with pytest.raises(mp2.Mp2gError, match="not canonical"):
                call()
