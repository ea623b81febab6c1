"""tests/stats_oracle.py against hand-computed cases, independent facts (the three bf16 parts sum to the value, a
Gramian is symmetric, the exact and the rational references agree) and, on every entry of its case tables, against the
host paths of ``ops/stats.py`` and ``models/linear.py``: both sides are validated without a GPU, which entitles the
oracle to judge the HIP kernels in tests/test_stats_kernels_gpu.py."""
import numpy as np
import pytest
import torch

import stats_oracle as O
from transmogrifai_amd.models import linear as LM
from transmogrifai_amd.ops import stats as ST


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


# ========================================================================================================== bf16
def test_bf16_rounding_by_hand():
    words = [0x3F800000, 0x3F800001, 0x3F80FFFF, 0x3F808000, 0x3F818000, 0x80000000, 0x7F800000, 0x00012345,
             0x7F7F7FFF]
    want = [0x3F80, 0x3F80, 0x3F81, 0x3F80, 0x3F82, 0x8000, 0x7F80, 0x0001, 0x7F7F]
    assert O.bf16_bits(O.f32_from_bits(words)).tolist() == want
    assert O.bf16_round(np.array([1.0 + 2.0 ** -7 + 2.0 ** -9], np.float32))[0] == np.float32(1.0 + 2.0 ** -7)


def test_split3_parts_sum_to_the_value():
    """h + mid + lo == c exactly for c = 0 and every |c| >= 2^-100 below the bf16 range's end; each part is a bf16
    value."""
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    keep = np.isfinite(c) & (np.abs(c) >= 2.0 ** -100) & (np.abs(c) < 3.0e38)
    c = np.concatenate([c[keep], O.PACK_SPECIAL[np.abs(O.PACK_SPECIAL) >= 2.0 ** -100], np.zeros(2, np.float32),
                        np.array([2.0 ** -100, -2.0 ** -100], np.float32)])
    h, mid, lo = O.split3(c)
    for part in (h, mid, lo):
        assert (part.view(np.uint32) & 0xFFFF == 0).all()
    assert ((h.astype(np.float64) + mid.astype(np.float64)) + lo.astype(np.float64) == c.astype(np.float64)).all()
    h, mid, lo = O.split3(np.array([1.0 + 2.0 ** -9 + 2.0 ** -18], np.float32))
    assert (h[0], mid[0], lo[0]) == (1.0, 2.0 ** -9, 2.0 ** -18)


def test_bf16_pack_by_hand():
    X = np.array([[1.0 + 2.0 ** -9, -0.0, 3.0], [2.0, 0.5, 1.0 + 2.0 ** -8]], np.float32)
    y = np.array([2, 0], np.int32)
    src, mode = [0, 0, 1, 0, 0, 0, 2, 2], [O.ZERO, O.ONE, O.RAW, O.HI, O.MID, O.LO, O.LABEL, O.RAW]
    got = O.bf16_pack(X, y, src, mode, np.zeros(8, np.float32), np.ones(8, np.float32), 16, 3)
    b = lambda v: int(O.bf16_bits(np.array([v], np.float32))[0])       # noqa: E731
    assert got[0].tolist()[:8] == [0, b(1.0), 0x8000, b(1.0), b(2.0 ** -9), 0, b(1.0), b(3.0)]
    assert got[1].tolist()[:8] == [0, b(1.0), b(0.5), b(2.0), 0, 0, 0, b(1.0)]      # 1 + 2^-8 ties to even: 1.0
    assert not got[2].any() and not got[:, 8:].any()
    mu, sc = np.full(8, 1.0, np.float32), np.full(8, 0.25, np.float32)
    got = O.bf16_pack(X, y, [0] * 8, [O.HI] * 8, mu, sc, 8, 2)
    assert got[:, 0].tolist() == [b(2.0 ** -11), b(0.25)]


@pytest.mark.parametrize("name", sorted(O.PACK_CASES))
def test_bf16_pack_cases_parts_sum(name):
    """On every packing case: HI + MID + LO columns of one source give back fp32((x - mu) * sc) wherever that is 0 or
    at least 2^-100, the columns past the sources are zero and so are the rows past n."""
    X, y, src, mode, mu, sc, ldb, rows, _ = O.pack_case(name)
    n, k = X.shape[0], len(src)
    got = O.bf16_pack(X, y, src, mode, mu, sc, ldb, rows)
    assert got.shape == (rows, ldb) and not got[n:].any() and not got[:, k:].any()
    reads = np.array([O.RAW <= m <= O.LO for m in mode])             # the columns whose source is a column of X
    src, mu, sc, k = src[reads], mu[reads], sc[reads], int(reads.sum())
    parts = O.bf16_pack(X, y, np.repeat(src, 3), [O.HI, O.MID, O.LO] * k, np.repeat(mu, 3), np.repeat(sc, 3), 3 * k, n)
    vals = (parts.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(n, k, 3)
    c = ((X[:, src] - mu[None, :]) * sc[None, :]).astype(np.float64)
    ok = (c == 0) | (np.abs(c) >= 2.0 ** -100)
    assert ((vals[:, :, 0] + vals[:, :, 1]) + vals[:, :, 2] == c)[ok].all()


@pytest.mark.parametrize("name,n,d,pad", O.BF16_EXACT_CASES)
def test_col_bf16_exact_cases(name, n, d, pad):
    X, exact = O.bf16_exact_data(n, d)
    assert ((O.col_bf16_exact(X) == 0) == exact).all()
    if n >= 8 and d >= 8:
        assert not exact[1:7].any() and exact[0] and exact[7]


# ===================================================================================================== col_stats
def test_col_stats_by_hand():
    X = np.array([[1.0, -0.0, -2.0], [2.0, 0.0, -2.0], [6.0, 0.0, -5.0]], np.float32)
    s = O.col_stats(X)
    assert s["mean"].tolist() == [3.0, 0.0, -3.0] and s["m2"].tolist() == [14.0, 0.0, 6.0]
    assert s["min"].tolist() == [1.0, 0.0, -5.0] and s["max"].tolist() == [6.0, 0.0, -2.0]
    assert s["nnz"].tolist() == [3.0, 0.0, 3.0] and s["count"] == 3
    big = np.array([[1e6], [1e6 + 0.0625], [1e6 + 0.125]], np.float32)
    assert O.col_stats(big)["m2"][0] == 2 * 0.0625 ** 2


def test_col_stats_launch_arithmetic():
    """The shapes the case table names do what it says of them."""
    assert O.col_stats_launch(76800, 3) == (301, 256, 1)          # 300 chunks hold the rows, the last holds none
    assert O.col_stats_launch(2305, 8)[0] == 10 and O.col_stats_launch(2305, 8)[2] == 0
    assert [O.col_stats_launch(n, 8)[0] for n in (1, 255, 256, 257)] == [1, 1, 2, 2]


@pytest.mark.parametrize("name,n,d,pad", O.COL_STATS_CASES)
def test_col_stats_cases_vs_host(name, n, d, pad):
    X = O.col_stats_data(n, d)
    want = O.col_stats(X)
    cnt, mean, m2, mn, mx, nnz = ST._col_partials(_t(X))
    assert cnt == want["count"]
    np.testing.assert_allclose(mean.numpy(), want["mean"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(m2.numpy(), want["m2"], rtol=1e-9, atol=0)
    for got, key in ((mn, "min"), (mx, "max"), (nnz, "nnz")):
        assert np.array_equal(got.numpy(), want[key])
    assert (want["m2"][[j for j in range(d) if O.COL_KINDS[j % 8] in ("constant", "zero")]] == 0).all()


# ================================================================================================== class_colsum
@pytest.mark.parametrize("name,n,d,P,L,real", O.CLASS_COLSUM_CASES)
def test_class_colsum_cases_vs_host(name, n, d, P, L, real):
    X, codes = O.class_colsum_data(n, d, P, L, real)
    want, mag = O.class_colsum(X, codes, L)
    got = ST.class_column_sums(_t(X), _t(codes), L).numpy()
    if real:
        assert (np.abs(got - want) <= n * 2.0 ** -52 * mag).all()
    else:
        assert np.array_equal(got, want)
    if P > 1:
        assert not want[P - 1].any()


def test_class_colsum_by_hand():
    X = np.array([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], np.float32)
    codes = np.array([[0, 1, 0], [-1, 2, 5]], np.int32)
    want, mag = O.class_colsum(X, codes, 3)
    assert want[0].tolist() == [[101.0, 202.0], [10.0, 20.0], [0.0, 0.0]]
    assert want[1].tolist() == [[0.0, 0.0], [0.0, 0.0], [10.0, 20.0]]
    assert np.array_equal(want, mag)


# ============================================================================================== weighted_colsums
@pytest.mark.parametrize("name,n,d,P", O.WEIGHTED_COLSUMS_CASES)
def test_weighted_colsums_cases_vs_host(name, n, d, P):
    """The fp32 sums of the host path are exact on this data (eighths of integers under 2^24), so its mean and
    unbiased std must be what the oracle's sums give."""
    X, W = O.weighted_colsums_data(n, d, P)
    s = O.weighted_colsums_exact(X, W)
    assert np.abs(s).max() * 8 < 2 ** 24
    std, mean = LM._feature_std(_t(X), _t(W))
    cnt = W.astype(np.float64).sum(0)
    m = s[:, 0].T / np.maximum(cnt, 1)[None, :]
    var = (s[:, 1].T - cnt[None, :] * m * m) / np.maximum(cnt - 1, 1)[None, :]
    np.testing.assert_allclose(mean.numpy(), m, rtol=1e-15, atol=0)
    np.testing.assert_allclose(std.numpy(), np.sqrt(np.maximum(var, 0)), rtol=1e-12, atol=1e-12)


def test_weighted_colsums_references_agree():
    X, W = O.weighted_colsums_data(37, 3, 2)
    real, mag = O.weighted_colsums_real(X, W)
    assert np.array_equal(real, O.weighted_colsums_exact(X, W))
    assert np.array_equal(mag[:, 1], real[:, 1])


# ========================================================================================================= wgram
@pytest.mark.parametrize("name,n,d,K,ymode", O.WGRAM_CASES)
def test_wgram_cases_vs_host(name, n, d, K, ymode):
    X, W, Y = O.wgram_data(n, d, K, ymode)
    want = O.wgram_exact(X, W, Y)
    assert want.shape == (K, d + 1 + (ymode != "none"), d + 1 + (ymode != "none"))
    assert np.array_equal(want, want.transpose(0, 2, 1))
    assert np.array_equal(ST.weighted_gram(_t(X), _t(W), _t(Y)).numpy(), want)


def test_wgram_real_reference():
    _, n, d, K, ymode = O.WGRAM_REAL_CASE
    X, W, Y = O.wgram_data(n, d, K, ymode, real=True)
    want, mag = O.wgram_real(X, W, Y)
    got = ST.weighted_gram(_t(X), _t(W), _t(Y)).numpy()
    assert (np.abs(got - want) <= n * 2.0 ** -52 * mag).all()
    assert np.array_equal(want, want.transpose(0, 2, 1)) and (mag >= np.abs(want)).all()
    Xe, We, Ye = O.wgram_data(9, 2, 2, "per_weight")
    assert np.array_equal(O.wgram_real(Xe, We, Ye)[0], O.wgram_exact(Xe, We, Ye))


# ====================================================================================================== Gramians
@pytest.mark.parametrize("name,n,d,L", O.GRAM_AUG_CASES)
def test_gram_aug_cases_vs_host(name, n, d, L):
    """The fp32 centring is exact on this data, so the host Gramian centred on the same integers is the oracle's."""
    X, mu, y = O.gram_aug_data(n, d, L)
    want = O.gram_int(O.gram_aug(X, mu, y, L), 0.25)
    assert np.array_equal(want, want.T) and want.shape == (d + L, d + L)
    inside = (y >= 0) & (y < L)
    got = ST.gram_centered(_t(X[inside]), _t(mu.astype(np.float64)), _t(y[inside]), L).numpy() if L and inside.any() \
        else None
    if got is not None:                     # the host path takes codes in [0, L) only: the rows outside are compared
        rest = O.gram_int(O.gram_aug(X[~inside], mu, y[~inside], L), 0.25)       # through the oracle's additivity
        assert np.array_equal(got + rest, want)
    if L == 0:
        assert np.array_equal(ST.gram_centered(_t(X), _t(mu.astype(np.float64))).numpy(), want)


def _centered_cases():
    for name, n, d, kind, L in O.GRAM_CENTERED_CASES:
        yield name, O.gram_centered_data(n, d, kind, L) + (L,), 2.0 ** -10
    yield "three_parts_non_zero", O.gram_lo_case(), 2.0 ** -19


@pytest.mark.parametrize("name,case,unit", list(_centered_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_gram_centered_cases_vs_host(name, case, unit):
    X, mean, y, L = case
    want = O.gram_int(O.gram_centered(X, mean, y, L), unit)
    assert np.array_equal(want, want.T)
    assert np.array_equal(ST.gram_centered(_t(X), _t(mean), _t(y), L).numpy(), want)


def test_gram_centered_data_is_what_the_exactness_argument_needs():
    """Non-exact columns: every centred value has a non-zero integer high part, the dyadic rest as its middle part and
    no low part; the three-part case has all parts non-zero somewhere, within the magnitudes its docstring uses."""
    for _, n, d, kind, L in O.GRAM_CENTERED_CASES:
        X, mean, _ = O.gram_centered_data(n, d, kind, L)
        mix = O._mix(d, kind)
        assert ((O.col_bf16_exact(X) == 0) == np.array(mix)).all()
        for j in [j for j in range(d) if not mix[j]]:
            h, mid, lo = O.split3((X[:, j] - np.float32(mean[j])).astype(np.float32))
            assert (h == np.round(h)).all() and (np.abs(h) >= 2).all() and (np.abs(h) <= 6).all() and not lo.any()
            assert (mid * 1024 == np.round(mid * 1024)).all() and (np.abs(mid) <= 3 / 1024).all() and mid.any()
    X, mean, _, _ = O.gram_lo_case()
    h, mid, lo = O.split3((X[:, 1:] - np.float32(-4.0)).astype(np.float32))
    assert (np.abs(h) >= 2).all() and (np.abs(h) <= 6).all() and (h == np.round(h)).all()
    assert (np.abs(mid) <= 1.51 * 2.0 ** -10).all() and (np.abs(mid) >= 2.0 ** -10).all() and (mid * 2.0 ** 17 == np.round(mid * 2.0 ** 17)).all()
    assert (np.abs(lo) <= 2.0 ** -18).all() and lo.any() and (lo * 2.0 ** 19 == np.round(lo * 2.0 ** 19)).all()


def test_gram_real_case_vs_host():
    X, mean, y, L = O.gram_real_case()
    A = O.gram_centered(X, mean, y, L)
    np.testing.assert_allclose(ST.gram_centered(_t(X), _t(mean), _t(y), L).numpy(), A.T @ A, rtol=1e-12, atol=1e-9)
    assert (mean.astype(np.float32).astype(np.float64) != mean).any()


@pytest.mark.parametrize("name,n,D,pad", O.GRAM_BF16_CASES)
def test_gram_bf16_cases(name, n, D, pad):
    A = O.gram_bf16_data(n, D, pad)
    assert A.shape[1] == (D + 127) // 128 * 128 + pad and not A[:, D:].any()
    assert np.array_equal(O.bf16_round(A), A)
    G = O.gram_int(A[:, :D], 1.0)
    assert np.array_equal(G, A[:, :D].astype(np.float64).T @ A[:, :D].astype(np.float64))
