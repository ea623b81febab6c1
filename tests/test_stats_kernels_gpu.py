"""Kernel-level oracle tests of the column-statistics and Gramian kernels (``ops/csrc/hip/stats_kernels.hip``:
``col_partials`` / ``col_fold``, ``class_colsum``, ``weighted_colsums``, ``wgram``, ``gram_aug``, ``gram_bf16``,
``bf16_pack``, ``col_bf16_exact`` and their folds) against tests/stats_oracle.py, which tests/test_stats_oracle.py
validates against the host paths on the same case tables. Each case is named after the path it forces and is the
smallest shape that reaches it. Semantics go through the wrappers of ``ops/stats.py``; row strides, guards and write
regions go through the direct C entries with sentinel-filled, padded outputs. Wherever the arithmetic can be exact
(integers, dyadic fractions, weights in eighths) the comparison is bit for bit, and every direct entry is called twice
and must give the same bits."""
import numpy as np
import pytest
import torch

import stats_oracle as O
from transmogrifai_amd.models import linear as LM
from transmogrifai_amd.ops import stats as ST

pytestmark = pytest.mark.gpu

SENT = -1.5e300
PAD = 64
JUNK = np.float32(7.5e29)            # what the padding columns of a row-strided input hold


def _lib():
    from transmogrifai_amd.ops import _native
    return _native.hip()


def _st():
    from transmogrifai_amd.ops import _native
    return _native.stream()


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _strided(X, pad, junk=JUNK):
    """``X`` on the device as the first columns of rows ``pad`` elements wider, the rest holding junk."""
    n, d = X.shape
    buf = np.full((n, d + pad), junk, X.dtype)
    buf[:, :d] = X
    return _d(buf)[:, :d]


def _sentinel(count):
    return _d(np.full(PAD + count + PAD, SENT, np.float64))


def _body(buf, count):
    """The ``count`` doubles between the pads of a sentinel buffer, after checking that both pads are untouched."""
    got = buf.cpu().numpy()
    assert (got[:PAD] == SENT).all() and (got[PAD + count:] == SENT).all()
    return got[PAD:PAD + count]


def _twice(count, call):
    """Run ``call(pointer to the body)`` on two sentinel buffers: rc 0 both times, same bits, pads untouched."""
    bodies = []
    for _ in range(2):
        buf = _sentinel(count)
        rc = call(buf.data_ptr() + 8 * PAD)
        torch.cuda.synchronize()
        assert rc == 0
        bodies.append(_body(buf, count))
    assert bodies[0].tobytes() == bodies[1].tobytes()
    assert not (bodies[0] == SENT).any()                 # fully written
    return bodies[0]


# ===================================================================================================== col_stats
@pytest.mark.parametrize("name,n,d,pad", O.COL_STATS_CASES)
def test_col_stats(name, n, d, pad):
    """Fewer rows than the 4 waves, one short of / on / one past a 256-row chunk, ten chunks (the fold's unroll of 8
    wraps), a launch whose last chunk holds no row, column counts around the 64-column tile, a row-strided view;
    columns: offset 1e6 and 1e4 with a small spread, constant, all zero, all negative, -0.0, indicator, normal."""
    X = O.col_stats_data(n, d)
    want = O.col_stats(X)
    Xd = _strided(X, pad)
    cs = ST.col_stats(Xd)
    assert cs["count"] == n
    var = want["m2"] / max(n - 1, 1)
    got_var = cs["variance"].cpu().numpy()
    np.testing.assert_allclose(cs["mean"].cpu().numpy(), want["mean"], rtol=1e-12, atol=0)
    live = var != 0
    np.testing.assert_allclose(got_var[live], var[live], rtol=1e-9, atol=0)
    assert (got_var[~live] == 0).all()
    for key, ref in (("min", "min"), ("max", "max"), ("numNonzeros", "nnz")):
        assert np.array_equal(cs[key].cpu().numpy(), want[ref])
    out = _twice(6 * d, lambda p: _lib().tmog_hip_col_stats(Xd.data_ptr(), None, n, d, Xd.stride(0), p, _st()))
    out = out.reshape(6, d)                               # rows: sum, M2, min, max, non-zeros, mean
    np.testing.assert_allclose(out[5], want["mean"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out[0], want["mean"] * n, rtol=1e-12, atol=0)
    np.testing.assert_allclose(out[1][live], want["m2"][live], rtol=1e-9, atol=0)
    assert (out[1][~live] == 0).all()
    assert np.array_equal(out[2], want["min"]) and np.array_equal(out[3], want["max"])
    assert np.array_equal(out[4], want["nnz"])
    if name == "empty_trailing_chunk":
        assert O.col_stats_launch(n, d)[2] == 1


# ================================================================================================== class_colsum
@pytest.mark.parametrize("name,n,d,P,L,real", O.CLASS_COLSUM_CASES)
def test_class_colsum(name, n, d, P, L, real):
    """Rows below the 4 waves and past a 256-row chunk, columns around the 64-column tile, P * L from 1 to the 64 the
    entry admits (128 KB of dynamic LDS), codes of -1 and a whole problem of -1; integer data bit for bit, real data
    within n 2^-52 of each entry's sum of magnitudes. The direct entry reads a row-strided X."""
    X, codes = O.class_colsum_data(n, d, P, L, real)
    want, mag = O.class_colsum(X, codes, L)
    Xd, cd = _strided(X, 3), _d(codes)
    got = ST.class_column_sums(Xd, cd, L).cpu().numpy()
    direct = _twice(P * L * d, lambda p: _lib().tmog_hip_class_colsum(Xd.data_ptr(), n, d, Xd.stride(0),
                                                                      cd.data_ptr(), P, L, p, _st()))
    for g in (got, direct.reshape(P, L, d)):
        if real:
            assert (np.abs(g - want) <= n * 2.0 ** -52 * mag).all()
        else:
            assert np.array_equal(g, want)


def test_class_colsum_rejects_more_than_64_accumulators():
    """P * L = 65: -2 before anything is launched, nothing written."""
    X, codes = O.class_colsum_data(17, 3, 5, 13)
    Xd, cd = _d(X), _d(codes)
    buf = _sentinel(65 * 3)
    rc = _lib().tmog_hip_class_colsum(Xd.data_ptr(), 17, 3, 3, cd.data_ptr(), 5, 13, buf.data_ptr() + 8 * PAD, _st())
    torch.cuda.synchronize()
    assert rc == -2 and (buf.cpu().numpy() == SENT).all()


# ============================================================================================== weighted_colsums
def _wcs(X, W, ldx_pad, ldw_pad):
    n, d = X.shape
    P = W.shape[1]
    Xd, Wd = _strided(X, ldx_pad), _strided(W, ldw_pad, np.float32(3.0e28))
    out = _twice(P * 2 * d, lambda p: _lib().tmog_hip_weighted_colsums(Xd.data_ptr(), n, d, Xd.stride(0), Wd.data_ptr(),
                                                                      Wd.stride(0), P, p, _st()))
    return out.reshape(P, 2, d)


@pytest.mark.parametrize("name,n,d,P", O.WEIGHTED_COLSUMS_CASES)
def test_weighted_colsums(name, n, d, P):
    """Rows below the 4 waves, around the 4096-row chunk and in three chunks; columns around the 64-column tile;
    problems around the 16 of a workgroup; fractional weights; ``ldx > d`` and ``ldw > P``. Bit for bit."""
    X, W = O.weighted_colsums_data(n, d, P)
    assert np.array_equal(_wcs(X, W, 3, 2), O.weighted_colsums_exact(X, W))


def test_weighted_colsums_real_valued_and_feature_std():
    """Real data over two chunks: each entry within n 2^-52 of its sum of magnitudes; and ``_feature_std`` on the
    device gives the mean and unbiased std of the oracle's exact sums."""
    rng = np.random.default_rng(5)
    n, d, P = 4097, 3, 2
    X, W = rng.standard_normal((n, d)).astype(np.float32), rng.random((n, P)).astype(np.float32)
    want, mag = O.weighted_colsums_real(X, W)
    assert (np.abs(_wcs(X, W, 1, 1) - want) <= n * 2.0 ** -52 * mag).all()
    X, W = O.weighted_colsums_data(4097, 65, 17)
    s = O.weighted_colsums_exact(X, W)
    std, mean = LM._feature_std(_d(X), _d(W))
    cnt = W.astype(np.float64).sum(0)
    m = s[:, 0].T / np.maximum(cnt, 1)[None, :]
    var = (s[:, 1].T - cnt[None, :] * m * m) / np.maximum(cnt - 1, 1)[None, :]
    np.testing.assert_allclose(mean.cpu().numpy(), m, rtol=1e-15, atol=0)
    np.testing.assert_allclose(std.cpu().numpy(), np.sqrt(np.maximum(var, 0)), rtol=1e-12, atol=1e-12)


# ========================================================================================================= wgram
def _wgram_direct(X, W, Y):
    """The direct entry with every leading dimension larger than its width; returns [K, D, D]."""
    n, d = X.shape
    K = W.shape[1]
    D = d + 1 + (Y is not None)
    Xd, Wd = _strided(X, 3), _strided(W, 3, 9.0e200)
    per = int(Y is not None and Y.ndim == 2)
    Yd = None if Y is None else _strided(Y if per else Y[:, None], 2, -4.0e200)
    out = _twice(K * D * D, lambda p: _lib().tmog_hip_wgram(
        Xd.data_ptr(), n, d, Xd.stride(0), Wd.data_ptr(), Wd.stride(0), K, None if Yd is None else Yd.data_ptr(),
        0 if Yd is None else Yd.stride(0), per, p, _st()))
    return out.reshape(K, D, D)


@pytest.mark.parametrize("name,n,d,K,ymode", O.WGRAM_CASES)
def test_wgram(name, n, d, K, ymode):
    """Rows below, on and past the 16-row stage and in several chunks; D around the 64-column tile with the ones
    column, then the response column, alone in the last tile; weight columns around the 4 of a workgroup; no, a shared
    and a per-weight response. Dyadic data and weights in eighths: bit for bit and bitwise symmetric, through the
    wrapper and through the direct entry with ``ldx > d``, ``ldw > K`` and ``ldy > K``."""
    X, W, Y = O.wgram_data(n, d, K, ymode)
    want = O.wgram_exact(X, W, Y)
    got = ST.weighted_gram(_d(X), _d(W), _d(Y)).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got, got.transpose(0, 2, 1))
    assert np.array_equal(_wgram_direct(X, W, Y), want)


def test_wgram_real_valued():
    """Each entry within n 2^-52 of its own sum of magnitudes (not of the largest entry); bitwise symmetric."""
    _, n, d, K, ymode = O.WGRAM_REAL_CASE
    X, W, Y = O.wgram_data(n, d, K, ymode, real=True)
    want, mag = O.wgram_real(X, W, Y)
    for got in (ST.weighted_gram(_d(X), _d(W), _d(Y)).cpu().numpy(), _wgram_direct(X, W, Y)):
        assert (np.abs(got - want) <= n * 2.0 ** -52 * mag).all()
        assert np.array_equal(got, got.transpose(0, 2, 1))


# ====================================================================================================== gram_aug
def _gram_aug_direct(X, mu, y, L):
    n, d = X.shape
    D = d + L
    Xd, md, yd = _strided(X, 3), _d(mu), _d(y)
    out = _twice(D * D, lambda p: _lib().tmog_hip_gram_aug(Xd.data_ptr(), n, d, Xd.stride(0), md.data_ptr(),
                                                          yd.data_ptr() if L else None, L, p, _st()))
    return out.reshape(D, D)


@pytest.mark.parametrize("name,n,d,L", O.GRAM_AUG_CASES)
def test_gram_aug_fp32_mfma(name, n, d, L):
    """The fp32 matrix-core Gramian through its entry: rows below, on and past the 32-row stage and the 256-row
    flush, two row chunks; D around the 128-column tile, the label block last in a tile and astride two; codes outside
    [0, L); row-strided X. Quarters centred on integers: every product and 256-row sum is exact, so bit for bit."""
    X, mu, y = O.gram_aug_data(n, d, L)
    want = O.gram_int(O.gram_aug(X, mu, y, L), 0.25)
    got = _gram_aug_direct(X, mu, y, L)
    assert np.array_equal(got, want)


def test_gram_aug_real_valued():
    """fp32 accumulation over 256-row slices: each entry within 2e-6 of sum |a_i| |a_j| (worst case 256 * 2^-24)."""
    X, mu, y = O.gram_aug_data(300, 7, 3, real=True)
    A = O.gram_aug(X, mu, y, 3)
    got = _gram_aug_direct(X, mu, y, 3)
    assert (np.abs(got - A.T @ A) <= 2e-6 * (np.abs(A).T @ np.abs(A))).all()
    assert np.array_equal(got, got.T)


# ===================================================================================================== gram_bf16
def _bf16(A):
    return _d(A).to(torch.bfloat16)


@pytest.mark.parametrize("name,n,D,pad", O.GRAM_BF16_CASES)
def test_gram_bf16(name, n, D, pad):
    """The bf16 matrix-core Gramian on a hand-built matrix of small integers: the row and D edges of the fp32 kernel,
    with the row stride on and 8 past the tile width. Bit for bit."""
    A = O.gram_bf16_data(n, D, pad)
    Ad = _bf16(A)
    out = _twice(D * D, lambda p: _lib().tmog_hip_gram_bf16(Ad.data_ptr(), n, A.shape[1], D, p, _st()))
    assert np.array_equal(out.reshape(D, D), O.gram_int(A[:, :D], 1.0))


def test_gram_bf16_guards():
    """Rejected before any launch, nothing written: a row stride below the tile width or off a multiple of 8, a base
    off 16 bytes (-2); no rows (-1)."""
    Ad = _bf16(O.gram_bf16_data(33, 5, 16))               # [33, 144]: room for every call below, were it to run
    buf = _sentinel(25)
    g = buf.data_ptr() + 8 * PAD
    fn = _lib().tmog_hip_gram_bf16
    assert fn(Ad.data_ptr(), 33, 120, 5, g, _st()) == -2
    assert fn(Ad.data_ptr(), 33, 132, 5, g, _st()) == -2
    assert fn(Ad.data_ptr() + 8, 32, 136, 5, g, _st()) == -2
    assert fn(Ad.data_ptr(), 0, 144, 5, g, _st()) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENT).all()


# ================================================================================================= gram_centered
def _centered_cases():
    for name, n, d, kind, L in O.GRAM_CENTERED_CASES:
        yield name, (n, d, kind, L), 2.0 ** -10
    yield "three_parts_non_zero", None, 2.0 ** -19


@pytest.mark.parametrize("name,spec,unit", list(_centered_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_gram_centered_bf16_exact(name, spec, unit):
    """The default path (exactness scan, packing, bf16 Gramian, fp64 re-assembly of the E / R / label blocks): all
    columns exact in bf16, none, interleaved, a single column; with and without labels. Dyadic data centred on
    integers chosen so that every fp32 block sum is exact (tests/stats_oracle.py): bit for bit the fp64 Gramian."""
    X, mean, y, L = O.gram_lo_case() if spec is None else O.gram_centered_data(*spec) + (spec[3],)
    want = O.gram_int(O.gram_centered(X, mean, y, L), unit)
    Xd = _strided(X, 3)
    got = ST._gram_centered_bf16(Xd, _d(mean), _d(y) if L else None, L).cpu().numpy()
    assert np.array_equal(got, want)
    again = ST.gram_centered(Xd, _d(mean), _d(y) if L else None, L).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    if spec is not None:
        exact = ST.bf16_exact_columns(Xd).cpu().numpy()
        assert exact.tolist() == O._mix(spec[1], spec[2])


def test_gram_centered_bf16_real_valued():
    """Real columns centred on an fp64 mean that fp32 does not hold: within 2e-6 of sum |b_i| |b_j| per entry, the
    bf16-exact column raw and the others centred, as the kernel sums them."""
    X, mean, y, L = O.gram_real_case()
    A = O.gram_centered(X, mean, y, L)
    exact = O.col_bf16_exact(X) == 0
    assert exact.tolist() == [j == 2 for j in range(X.shape[1])]
    B = np.abs(np.concatenate([np.where(exact[None, :], X.astype(np.float64), A[:, :X.shape[1]]), A[:, X.shape[1]:]], 1))
    got = ST._gram_centered_bf16(_d(X), _d(mean), _d(y), L).cpu().numpy()
    assert (np.abs(got - A.T @ A) <= 2e-6 * (B.T @ B)).all()


# ===================================================================================================== bf16_pack
def _view(X, view):
    n, d = X.shape
    if view == "aligned":
        return _d(X)
    if view == "ld_odd":
        return _strided(X, 3)
    flat = _d(np.concatenate([np.full(1, JUNK, np.float32), X.ravel(), np.full(3, JUNK, np.float32)]))
    return flat[1:1 + n * d].view(n, d)


@pytest.mark.parametrize("name", sorted(O.PACK_CASES))
def test_bf16_pack_bits(name):
    """The bf16 bit patterns of every output column against the oracle's round-to-nearest-even split: the 16-byte
    fast path and each of its four preconditions failing in turn, all seven modes in one group of eight, labels that
    match no code, rows around the 16 of a block, one and two 512-column tiles, ``rows > n``; scales 1, 1/4 and 1/3;
    zeros of both signs, a subnormal, 2^-120, 2^100, ties and near-ties of the bf16 rounding. Then the direct entry
    into a sentinel buffer."""
    X, y, src, mode, mu, sc, ldb, rows, view = O.pack_case(name)
    n = X.shape[0]
    want = O.bf16_pack(X, y, src, mode, mu, sc, ldb, rows)
    Xd, yd = _view(X, view), _d(y)
    assert (Xd.data_ptr() % 16 == 4) == (view == "base_off") and (Xd.stride(0) % 4 != 0) == (view == "ld_odd")
    got = ST.bf16_pack(Xd, src, mode, mu, sc, ldb, rows=rows, y=yd)
    assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), want)

    def full(v, dtype):
        a = np.zeros(ldb, dtype)
        a[:len(v)] = v
        return _d(a)
    cols = [full(src, np.int32), full(mode, np.int32), full(mu, np.float32), full(sc, np.float32)]
    bodies = []
    for _ in range(2):
        buf = _d(np.full(PAD + n * ldb + PAD, 0x7A7A, np.uint16).view(np.int16))
        rc = _lib().tmog_hip_bf16_pack(Xd.data_ptr(), n, Xd.stride(0), yd.data_ptr(), cols[0].data_ptr(),
                                       cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(),
                                       buf.data_ptr() + 2 * PAD, ldb, _st())
        torch.cuda.synchronize()
        assert rc == 0
        raw = buf.cpu().numpy().view(np.uint16)
        assert (raw[:PAD] == 0x7A7A).all() and (raw[PAD + n * ldb:] == 0x7A7A).all()
        bodies.append(raw[PAD:PAD + n * ldb].reshape(n, ldb))
    assert np.array_equal(bodies[0], want[:n]) and np.array_equal(bodies[1], want[:n])


def test_bf16_pack_guards():
    """Rejected before any launch, nothing written: a row stride off a multiple of 8, an output off 16 bytes (-2)."""
    X, y, src, mode, mu, sc, _, _, _ = O.pack_case("all_seven_modes_rows_17")
    Xd, yd = _d(X), _d(y)
    cols = [_d(np.resize(a, 16)) for a in (src, mode, mu, sc)]
    buf = _d(np.full(PAD + 17 * 16 + PAD, 0x7A7A, np.uint16).view(np.int16))
    for off, ldb in ((2 * PAD, 12), (2 * PAD + 8, 8)):
        rc = _lib().tmog_hip_bf16_pack(Xd.data_ptr(), 17, 24, yd.data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(),
                                       cols[2].data_ptr(), cols[3].data_ptr(), buf.data_ptr() + off, ldb, _st())
        assert rc == -2
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == 0x7A7A).all()


# ================================================================================================ col_bf16_exact
@pytest.mark.parametrize("name,n,d,pad", O.BF16_EXACT_CASES)
def test_col_bf16_exact(name, n, d, pad):
    """No rows, rows below the 4 waves, around the 1024-row chunk and in three chunks; columns around the 64-column
    tile; a row-strided view; one inexact value at the first row, the last row and a row of each residue mod 4; exact
    columns holding -0.0, infinities and a subnormal. The entry zeroes its output: it is handed garbage."""
    X, exact = O.bf16_exact_data(n, d)
    want = O.col_bf16_exact(X)
    assert ((want == 0) == exact).all()
    Xd = _strided(X, pad, np.float32(1.0000001)) if n else _d(np.zeros((1, d + pad), np.float32))[:, :d]
    bodies = []
    for _ in range(2):
        buf = _d(np.full(PAD + d + PAD, 0x5A5A5A5A, np.int32))
        rc = _lib().tmog_hip_col_bf16_exact(Xd.data_ptr(), n, d, Xd.stride(0), buf.data_ptr() + 4 * PAD, _st())
        torch.cuda.synchronize()
        assert rc == 0
        raw = buf.cpu().numpy()
        assert (raw[:PAD] == 0x5A5A5A5A).all() and (raw[PAD + d:] == 0x5A5A5A5A).all()
        bodies.append(raw[PAD:PAD + d].view(np.uint32))
    assert np.array_equal(bodies[0], want) and np.array_equal(bodies[1], want)
    if n:
        assert np.array_equal(ST.bf16_exact_columns(Xd).cpu().numpy(), exact)
