"""tests/dataprep_oracle.py against hand-computed cases and, on every entry of its case tables, against the project's
host torch paths (``ops/vector.py``, ``ops/rff.py``): both sides are validated without a GPU, which entitles the oracle
to judge the HIP kernels in tests/test_dataprep_kernels_gpu.py. The last test shows that the histogram case table
tells fused split arithmetic from the reference's."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import dataprep_oracle as O
from transmogrifai_amd.data.columns import NumericColumn
from transmogrifai_amd.features import types as T
from transmogrifai_amd.ops import rff as R
from transmogrifai_amd.ops import vector as V

NAN, INF = float("nan"), float("inf")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _cols(vals, valid):
    return [NumericColumn(T.Real, _t(v), _t(ok)) for v, ok in zip(vals, valid)]


# ================================================================================================= hand-computed
def test_vectorize_by_hand():
    vals = [np.array([1.0, NAN, -0.0], np.float32), np.array([INF, 5.0, NAN], np.float32)]
    valid = [np.array([True, False, True]), np.array([False, True, False])]
    fills = np.array([7.0, -2.0], np.float32)
    assert O.bits(O.vectorize(vals, valid, fills, False)).tolist() == O.bits(
        np.array([[1.0, -2.0], [7.0, 5.0], [-0.0, -2.0]], np.float32)).tolist()
    assert O.bits(O.vectorize(vals, valid, fills, True)).tolist() == O.bits(
        np.array([[1.0, 0, -2.0, 1], [7.0, 1, 5.0, 0], [-0.0, 0, -2.0, 1]], np.float32)).tolist()
    payload = np.array([0x7FC00123], np.uint32).view(np.float32)
    got = O.vectorize([payload], [np.array([True])], np.array([0.0], np.float32), False)
    assert got.view(np.uint32)[0, 0] == 0x7FC00123


def test_onehot_by_hand():
    lut = np.array([2, -1, 0, 1], np.int32)         # codes 0, 1, 2 are dictionary entries, entry 3 is "other"
    codes = np.array([0, 1, 2, 3, -1, 7, -4], np.int32)
    got = O.onehot([codes, codes[:7] * 0], [lut, np.array([0], np.int32)], [1, 0], 7, 5)
    want = np.zeros((7, 5), np.float32)
    want[:, 0] = 1.0                                # the length-1 lut: every code is "other" -> slot 0
    want[0, 3] = 1.0                                # code 0 -> slot 2
    want[2, 1] = 1.0                                # code 1 -> slot -1 (nothing); code 2 -> slot 0
    want[[3, 4, 5, 6], 2] = 1.0                     # ln - 1, -1, past the lut, negative -> lut[3] = slot 1
    assert (got == want).all()


def test_gather_by_hand():
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = np.arange(100, 108, dtype=np.float32).reshape(4, 2)
    got = O.gather([(a[:, 1:], None), (b, np.array([1, 1, 0]))], np.array([3, 0, 3]), 4)
    assert got.tolist() == [[10, 11, 107, 107, 106], [1, 2, 101, 101, 100], [10, 11, 107, 107, 106]]
    assert O.gather([(b, None)], None, 4).tolist() == b.tolist()


def test_masked_sums_by_hand():
    v = [np.array([1.0, 2.0, NAN, 4.0, 8.0]), np.array([1, 1, 1, 1, 1], np.float32)]
    ok = [np.array([True, True, False, True, True]), None]
    assert O.masked_sums(v, ok, 5, 2).tolist() == [[[3, 2], [4, 1], [8, 1]], [[2, 2], [2, 2], [1, 1]]]
    assert O.masked_sums(v, ok, 5, 5).tolist() == [[[15, 4]], [[5, 5]]]
    assert O.exact_sum([1e16, 1.0, -1e16]) == 1


def test_summary_by_hand():
    s = O.summary([np.array([1.0, 2.0, 9.0])], [np.array([True, True, False])], np.array([0.0, 0.0, 1.0]))
    assert s[0].tolist() == [2, 1, 1, 2, 3, 5, 9, 17, 1]
    e = O.summary([np.array([1.0, 2.0], np.float32)], [np.array([False, False])], np.array([2, 3]))
    assert e[0].tolist() == [0, 2, INF, -INF, 0, 0, 0, 0, 5]
    n = O.summary([np.array([1.0, NAN, -3.0])], [None])[0]
    assert n[:2].tolist() == [3, 0] and np.isnan(n[2:8]).all() and n[8] == 0
    b = O.summary([np.array([1.0, -2.0, 9.0])], [None], np.array([5.0, 5.0, 5.0]), bounds=True)[0]
    assert b == [0, 0, 0, 0] + [6 * O.U * s for s in (12, 86, 738, 6578)] + [0]


def test_hist_by_hand():
    # step = 10 / 10 = 1 -> buckets [0,1),[1,2),...,[10,11); 10.0 is in bucket 10, nothing out of range
    assert O.hist([0.0, 0.5, 1.0, 2.0, 5.0, 10.0], None, 0.0, 10.0, 12) == [2, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert O.hist([3.0, 3.0, 4.0], None, 3.0, 3.0, 12)[:3] == [2, 1, 0]
    # below min, NaN, the last split and beyond -> the last bucket; null rows do not count
    assert O.hist([-0.5, NAN, 2.0, 7.0, 1.0, 1.0], [True] * 5 + [False], 0.0, 1.0, 3) == [0, 1, 4]
    assert O.hist_splits(0.0, 1.0, 3) == [0.0, 1.0, 2.0]
    assert O.hist([0.0, NAN, -INF], None, INF, -INF, 4) == [1, 2, 0, 0]


@pytest.mark.parametrize("fixture,value,bucket", [((100, -3.0, 6.0), 6.0, 98), ((100, -3.0, 15.0), 6.0, 49),
                                                  ((100, -3.0, 15.0), 15.0, 98), ((100, -2.0, 7.0), 7.0, 98)])
def test_hist_integer_fixtures_by_hand(fixture, value, bucket):
    """98 steps of (max - min) / 98 from min: the rounded product plus min lands on the integer itself, so the integer
    opens its bucket; the single rounding of a fused multiply-add lands one ulp above it and pushes it one bucket down."""
    bins, mn, mx = fixture
    assert value in O.FIXTURE_MOVERS[fixture]
    step = (mx - mn) / 98.0
    assert mn + step * bucket == value
    assert float(Fraction(mn) + Fraction(step) * bucket) == np.nextafter(value, INF)
    assert O.hist_bucket(value, O.hist_splits(mn, mx, bins)) == bucket
    assert O.hist_bucket(value, O.hist_splits(mn, mx, bins, fused=True)) == bucket - 1


# ======================================================================================== the host paths, per table
@pytest.mark.parametrize("F", O.VECTORIZE_F)
@pytest.mark.parametrize("n", O.VECTORIZE_N)
def test_vectorize_host_path(n, F):
    vals, valid, fills = O.vectorize_case(n, F)
    if F >= 4:
        assert valid[0].all() and not valid[3].any()
    for track in (False, True):
        got = V.fill_and_track(_cols(vals, valid), [float(f) for f in fills], track, torch.float32)
        assert np.array_equal(O.bits(got.numpy()), O.bits(O.vectorize(vals, valid, fills, track)))


@pytest.mark.parametrize("n", O.ONEHOT_N)
def test_onehot_host_path(n):
    codes = O.onehot_case(n)
    want = O.onehot(codes, O.ONEHOT_LUTS, O.ONEHOT_OFFS, n, O.ONEHOT_W)
    if n >= 4:
        for c, lut in zip(codes, O.ONEHOT_LUTS):
            assert {-1, len(lut) - 2, len(lut) - 1, len(lut) + 3} <= set(c.tolist())
    got = torch.zeros(n, O.ONEHOT_W)
    V.onehot_pivot(got, [_t(c) for c in codes], list(O.ONEHOT_LUTS), list(O.ONEHOT_OFFS))
    assert np.array_equal(got.numpy(), want)


def test_onehot_scatter_maps_codes_past_the_lut_to_the_last_entry():
    out = torch.zeros(4, 3)
    V.onehot_scatter(out, torch.tensor([3, 4, 9, 1], dtype=torch.int32), torch.tensor([0, 1, -1, 2]), 0)
    assert out.tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, 0]]


@pytest.mark.parametrize("listed", [False, True], ids=["allrows", "rowlist"])
@pytest.mark.parametrize("k", O.GATHER_K)
@pytest.mark.parametrize("m", O.GATHER_M)
def test_gather_host_path(m, k, listed):
    blocks, rows, n = O.gather_case(m, k, listed)
    want = O.gather(blocks, rows, n)
    assert want.shape == (m, k)
    if listed and m >= 5:
        r = rows.tolist()
        assert 0 in r and n - 1 in r and len(set(r)) < m and r != sorted(r)
    tb = [(torch.from_numpy(mat), _t(ci)) for mat, ci in blocks]
    if k > 1:
        assert tb[1][0].stride(0) == 29 and tb[1][0].shape[1] == 20
    got = V.gather_rows_cols(tb, _t(rows), n)
    assert np.array_equal(O.bits(got.numpy()), O.bits(want))


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
@pytest.mark.parametrize("n", O.COLSUM_N)
def test_masked_sums_host_path(n, integer):
    """``column_means`` is sum / count (0 for an all-null column). Integer data: equal. Real data: the host sum is
    some order of fp64 additions, within ``n 2^-53 sum |x|`` of the exact sum, and the division rounds once more."""
    vals, valid = O.colsum_case(n, integer)
    ref = O.masked_sums(vals, valid, n, n)[:, 0]
    got = V.column_means(_cols(vals, valid))
    for c, (v, ok) in enumerate(zip(vals, valid)):
        s, k = ref[c]
        if k == 0:
            assert got[c] == 0.0
        elif integer:
            assert got[c] == s / k
        else:
            xs = [float(x) for r, x in enumerate(v) if ok is None or ok[r]]
            bound = (n + 1) * O.U * O.exact_sum([abs(x) for x in xs])
            assert abs(Fraction(got[c]) * int(k) - O.exact_sum(xs)) <= bound


def _assert_summary(got, vals, valid, label, integer):
    """count, nulls, min and max equal; the five sums equal on integer data, within the oracle's bound else."""
    ref = O.summary(vals, valid, label)
    got = np.asarray(got, np.float64)
    assert np.array_equal(got[:, :4], ref[:, :4])
    if integer:
        assert np.array_equal(got[:, 4:], ref[:, 4:])
        return
    bound = O.summary(vals, valid, label, bounds=True)
    for f in range(len(vals)):
        for s in range(4, O.NSTAT):
            assert abs(Fraction(got[f, s]) - Fraction(ref[f, s])) <= bound[f][s], (f, s, got[f, s], ref[f, s])


@pytest.mark.parametrize("n,F,integer", O.SUMMARY_CASES)
def test_summary_host_path(n, F, integer):
    vals, valid, label = O.summary_case(n, F, integer)
    got = R.numeric_summary([_t(v) for v in vals], [_t(ok) for ok in valid], _t(label))
    _assert_summary(got.numpy(), vals, valid, label, integer)


@pytest.mark.parametrize("n,F", O.SUMMARY_NAN_SHAPES)
def test_summary_nan_host_path(n, F):
    """A NaN among the valid values propagates into min and max (and the sums)."""
    vals, valid = O.summary_nan_case(n, F)
    ref = O.summary(vals, valid)
    assert np.isnan(ref[:2, 2:8]).all() and (F < 3 or np.isfinite(ref[2]).all())
    got = R.numeric_summary([_t(v) for v in vals], [_t(ok) for ok in valid]).numpy()
    assert np.array_equal(got[:, :4], ref[:, :4], equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(ref))


@pytest.mark.parametrize("gid", list(O.hist_groups()))
def test_hist_host_path(gid):
    bins, cols = O.hist_groups()[gid]
    got = R.numeric_hist([_t(c["values"]) for c in cols], [_t(c["valid"]) for c in cols],
                         torch.tensor([c["lo"] for c in cols], dtype=torch.float64),
                         torch.tensor([c["hi"] for c in cols], dtype=torch.float64), bins)
    want = O.hist_group_counts(gid)
    bad = [c["name"] for c, g, w in zip(cols, got.numpy(), want) if not np.array_equal(g, w)]
    assert not bad
    empty = [i for i, c in enumerate(cols) if c["name"] == "empty-summary"]
    for i in empty:
        assert want[i, 1] == cols[i]["valid"].sum() and want[i].sum() == want[i, 1]


def test_hist_table_discriminates_fused_splits():
    """A kernel that compares against fused splits fails the GPU test: over the table, the fused oracle differs from
    the reference one in each of the three integer fixtures, and in at least 20 (column, value) pairs in all."""
    pairs = 0
    named = set()
    for gid, (bins, cols) in O.hist_groups().items():
        for c in cols:
            if not c["lo"] < c["hi"]:
                continue
            s, sf = O.hist_splits(c["lo"], c["hi"], bins), O.hist_splits(c["lo"], c["hi"], bins, fused=True)
            xs = {float(x) for r, x in enumerate(c["values"]) if c["valid"] is None or c["valid"][r]}
            moved = {x for x in xs if O.hist_bucket(x, s) != O.hist_bucket(x, sf)}
            pairs += len(moved)
            key = (bins, c["lo"], c["hi"])
            if key in O.FIXTURE_MOVERS and set(O.FIXTURE_MOVERS[key]) <= moved:
                named.add(key)
        ref, fused = O.hist_group_counts(gid), O.hist_group_counts(gid, fused=True)
        for c, a, b in zip(cols, ref, fused):
            if (bins, c["lo"], c["hi"]) in O.FIXTURE_MOVERS:
                assert not np.array_equal(a, b), c["name"]
    assert named == set(O.INTEGER_FIXTURES)
    assert pairs >= 20
