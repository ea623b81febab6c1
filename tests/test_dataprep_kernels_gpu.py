"""Kernel-level oracle tests of the data-preparation kernels: ``vectorize_numeric_kernel``, ``onehot_pivot_kernel``,
``gather_rows_cols_kernel``, ``masked_colsum_kernel`` (``ops/csrc/hip/vector_kernels.hip``) and ``rff_summary_kernel``,
``rff_summary_fold_kernel``, ``rff_hist_kernel`` (``ops/csrc/hip/rff_kernels.hip``) against tests/dataprep_oracle.py,
which tests/test_dataprep_oracle.py validates against the host torch paths on the same case tables. Each case is named
after the path it forces and is the smallest shape that reaches it. Semantics go through the Python wrappers; the
write-guard and chunking cases go through the direct C entry points with sentinel-filled buffers."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import dataprep_oracle as O
from transmogrifai_amd.data.columns import NumericColumn
from transmogrifai_amd.features import types as T
from transmogrifai_amd.ops import rff as R
from transmogrifai_amd.ops import vector as V

pytestmark = pytest.mark.gpu

SENT = np.float32(-1.5e30)
PAD = 64


def _loaded():
    from transmogrifai_amd.ops import _native
    return _native.hip_loaded()


def _lib():
    from transmogrifai_amd.ops import _native
    return _native.hip()


def _st():
    from transmogrifai_amd.ops import _native
    return _native.stream()


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptrs(tensors):
    """Device array of device pointers (0 for None)."""
    return _d(np.array([0 if t is None else t.data_ptr() for t in tensors], np.int64))


def _sentinel(count):
    return _d(np.full(PAD + count + PAD, SENT, np.float32))


def _body(buf, count):
    """The ``count`` floats between the pads of a sentinel buffer, after checking that both pads are untouched."""
    got = buf.cpu().numpy()
    assert (got[:PAD] == SENT).all() and (got[PAD + count:] == SENT).all()
    return got[PAD:PAD + count]


# ============================================================================================= vectorize_numeric
@pytest.mark.parametrize("F", O.VECTORIZE_F)
@pytest.mark.parametrize("n", O.VECTORIZE_N)
def test_vectorize_tile_edges(n, F):
    """64-row x 32-column tiles: rows and columns one short of, on and one past a tile, and more than one tile each
    way; both ``track`` settings; an all-valid and an all-null column; bitwise. Then the same through the direct entry
    into a sentinel buffer whose rows are ``W = F * per + 5`` wide: the 5 padding columns, and the floats before row 0
    and after row n - 1, keep the sentinel."""
    vals, valid, fills = O.vectorize_case(n, F)
    dv, dk = [_d(v) for v in vals], [_d(k) for k in valid]
    cols = [NumericColumn(T.Real, v, k) for v, k in zip(dv, dk)]
    bytes_ = [k.to(torch.uint8) for k in dk]
    vp, kp, df = _ptrs(dv), _ptrs(bytes_), _d(fills)
    for track in (0, 1):
        want = O.bits(O.vectorize(vals, valid, fills, bool(track)))
        got = V.fill_and_track(cols, [float(f) for f in fills], bool(track), torch.float32)
        assert np.array_equal(O.bits(got.cpu().numpy()), want)
        used = F * (2 if track else 1)
        W = used + 5
        buf = _sentinel(n * W)
        rc = _lib().tmog_hip_vectorize_numeric(vp.data_ptr(), kp.data_ptr(), df.data_ptr(), n, F, None, None, None,
                                               buf.data_ptr() + 4 * PAD, W, track, _st())
        torch.cuda.synchronize()
        assert rc == 0
        body = _body(buf, n * W).reshape(n, W)
        assert (body[:, used:] == SENT).all()
        assert np.array_equal(O.bits(body[:, :used]), want)
    assert _loaded()


# ================================================================================================== onehot_pivot
def _onehot_direct(codes, n, W, fill):
    dc = [_d(c) for c in codes]
    dl = [_d(lut) for lut in O.ONEHOT_LUTS]
    ln = _d(np.array([len(lut) for lut in O.ONEHOT_LUTS], np.int32))
    off = _d(np.array(O.ONEHOT_OFFS, np.int64))
    cp, lp = _ptrs(dc), _ptrs(dl)
    buf = _d(np.full(PAD + n * W + PAD, fill, np.float32))
    rc = _lib().tmog_hip_onehot_pivot(cp.data_ptr(), lp.data_ptr(), ln.data_ptr(), off.data_ptr(), len(dc), n,
                                      buf.data_ptr() + 4 * PAD, W, _st())
    torch.cuda.synchronize()
    assert rc == 0
    got = buf.cpu().numpy()
    assert (got[:PAD] == fill).all() and (got[PAD + n * W:] == fill).all()
    return got[PAD:PAD + n * W].reshape(n, W)


@pytest.mark.parametrize("n", O.ONEHOT_N)
def test_onehot_block_edges_and_other_codes(n):
    """256 rows per block: one row, one short of a block, a block, a block and a row. Three columns: a lut of length
    1, luts with -1 slots; codes -1, ln-2, ln-1, ln+3 and other negatives. Equal to the oracle through the wrapper.
    Then the direct entry on a sentinel-filled matrix 3 columns wider than used: the kernel stores 1.0 at the hits and
    nothing else, so every other element, the padding columns included, keeps the sentinel."""
    codes = O.onehot_case(n)
    want = O.onehot(codes, O.ONEHOT_LUTS, O.ONEHOT_OFFS, n, O.ONEHOT_W)
    out = torch.zeros(n, O.ONEHOT_W, device="cuda")
    V.onehot_pivot(out, [_d(c) for c in codes], list(O.ONEHOT_LUTS), list(O.ONEHOT_OFFS))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    W = O.ONEHOT_W + 3
    body = _onehot_direct(codes, n, W, SENT)
    wide = np.full((n, W), SENT, np.float32)
    wide[:, :O.ONEHOT_W][want == 1.0] = 1.0
    assert np.array_equal(body, wide)
    assert _loaded()


# ============================================================================================== gather_rows_cols
@pytest.mark.parametrize("listed", [False, True], ids=["allrows", "rowlist"])
@pytest.mark.parametrize("k", O.GATHER_K)
@pytest.mark.parametrize("m", O.GATHER_M)
def test_gather_tile_edges(m, k, listed):
    """32-row x 64-column tiles, rows and columns around one tile and past two; all rows or a non-monotone row list
    with duplicates, row 0 and row n - 1; blocks of several widths, a [n, 1] block, a column slice with a row stride
    larger than its width, a reversed column index list with repeats; bitwise. Then the direct entry into a buffer with
    sentinel floats before row 0 and after row m - 1."""
    blocks, rows, n = O.gather_case(m, k, listed)
    want = O.bits(O.gather(blocks, rows, n))
    tb = []
    for mat, ci in blocks:
        if mat.base is not None:                   # the column slice of a wider matrix: slice the device copy likewise
            root = mat.base
            lo = (mat.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // 4
            t = _d(root)[:, lo:lo + mat.shape[1]]
            assert t.stride(0) == root.shape[1] == 29 and t.shape[1] == 20
        else:
            t = _d(mat)
        assert np.array_equal(O.bits(t.cpu().numpy()), O.bits(mat))
        tb.append((t, None if ci is None else torch.from_numpy(ci)))
    drows = _d(rows)
    got = V.gather_rows_cols(tb, drows, n)
    torch.cuda.synchronize()
    assert got.shape == (m, k) and np.array_equal(O.bits(got.cpu().numpy()), want)
    # the direct entry: per output column, the address of its first row and its row stride (in floats)
    base, ld = [], []
    for t, ci in tb:
        for j in (range(t.shape[1]) if ci is None else ci.tolist()):
            base.append(t.data_ptr() + 4 * j)
            ld.append(t.stride(0))
    assert len(base) == k
    bp, lp = _d(np.array(base, np.int64)), _d(np.array(ld, np.int64))
    buf = _sentinel(m * k)
    rc = _lib().tmog_hip_gather_rows_cols(bp.data_ptr(), lp.data_ptr(), None if drows is None else drows.data_ptr(),
                                          m, k, buf.data_ptr() + 4 * PAD, _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(O.bits(_body(buf, m * k).reshape(m, k)), want)
    assert _loaded()


# ================================================================================================= masked_colsum
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
@pytest.mark.parametrize("n", O.COLSUM_N)
def test_masked_colsum_chunks(n, integer):
    """Rows around the 1024-row thread step; ``rows_per_chunk`` in {n, 1024, 1000, 257}: one chunk, several chunks, a
    last chunk of one row (n = 1025 and 2049 at 1024). fp32 and fp64 columns; a null validity pointer, an all-false and
    a mixed mask; NaN and infinities in the masked-out slots. Counts always equal the oracle; integer-valued data: every
    per-chunk sum equals it; real-valued data: the column sum (chunks added in order) is within ``n 2^-53 sum |x|`` of
    the exact sum, the bound of any order of fp64 additions. The partials buffer is written exactly."""
    vals, valid = O.colsum_case(n, integer)
    dv = [_d(v) for v in vals]
    dk = [None if k is None else _d(k.astype(np.uint8)) for k in valid]
    vp, kp = _ptrs(dv), _ptrs(dk)
    dt = _d(np.array([1 if v.dtype == np.float64 else 0 for v in vals], np.int32))
    C = len(vals)
    for rpc in O.colsum_chunkings(n):
        chunks = -(-n // rpc)
        buf = _d(np.full(PAD + C * chunks * 2 + PAD, -7.25, np.float64))
        rc = _lib().tmog_hip_masked_colsum(vp.data_ptr(), kp.data_ptr(), dt.data_ptr(), C, n, rpc,
                                           buf.data_ptr() + 8 * PAD, _st())
        torch.cuda.synchronize()
        assert rc == 0
        got = buf.cpu().numpy()
        assert (got[:PAD] == -7.25).all() and (got[PAD + C * chunks * 2:] == -7.25).all()
        got = got[PAD:PAD + C * chunks * 2].reshape(C, chunks, 2)
        ref = O.masked_sums(vals, valid, n, rpc)
        assert np.array_equal(got[:, :, 1], ref[:, :, 1]), rpc
        if integer:
            assert np.array_equal(got[:, :, 0], ref[:, :, 0]), rpc
            continue
        for c, (v, ok) in enumerate(zip(vals, valid)):
            xs = [float(x) for r, x in enumerate(v) if ok is None or ok[r]]
            total = 0.0
            for s in got[c, :, 0]:
                total += float(s)
            bound = n * O.U * O.exact_sum([abs(x) for x in xs])
            assert abs(Fraction(total) - O.exact_sum(xs)) <= bound, (rpc, c)
    assert _loaded()


def test_column_means_all_null_column_is_zero():
    """Through the wrapper: the all-false column (NaN and infinities in every slot) has mean 0.0; the others equal
    sum / count of the oracle (integer data)."""
    n = 1025
    vals, valid = O.colsum_case(n, True)
    ref = O.masked_sums(vals, valid, n, n)[:, 0]
    got = V.column_means([NumericColumn(T.Real, _d(v), _d(k)) for v, k in zip(vals, valid)])
    assert got[2] == 0.0 and ref[2, 1] == 0
    assert got == [float(s / k) if k else 0.0 for s, k in ref]
    assert _loaded()


# =================================================================================================== rff_summary
def _summary(vals, valid, label):
    got = R.numeric_summary([_d(v) for v in vals], [_d(k) for k in valid], _d(label))
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("n,F,integer", O.SUMMARY_CASES)
def test_rff_summary_shapes_dtypes_masks(n, F, integer):
    """n below a workgroup, around it and across chunks (2049 rows, 3 columns: 3 chunks of 683 rows); F across the
    128-wide fold block; fp32, fp64, int64, uint8 and bool columns; null pointer, mixed and all-null masks; label
    absent, fp32, fp64, int64 or bool. count, nulls, min, max equal the oracle (the all-null column: +inf / -inf);
    integer data in |x| <= 30: the five sums are equal; real data: within ``(n + 3) 2^-53 sum |x|^k``."""
    vals, valid, label = O.summary_case(n, F, integer)
    got = _summary(vals, valid, label)
    ref = O.summary(vals, valid, label)
    assert np.array_equal(got[:, :4], ref[:, :4])
    if F >= 3:
        assert ref[2, :4].tolist() == [0, n, np.inf, -np.inf]
    if integer:
        assert np.array_equal(got[:, 4:], ref[:, 4:])
    else:
        bound = O.summary(vals, valid, label, bounds=True)
        for f in range(F):
            for s in range(4, O.NSTAT):
                assert abs(Fraction(got[f, s]) - Fraction(ref[f, s])) <= bound[f][s], (f, s, got[f, s], ref[f, s])
    assert _loaded()


@pytest.mark.parametrize("n,F", O.SUMMARY_NAN_SHAPES)
def test_rff_summary_nan_among_valid_values_propagates(n, F):
    """A valid NaN in the last wave of the last chunk reaches min and max (and the sums) through the wave, block and
    chunk folds, as on the host path; a masked-out NaN (third column) does not."""
    vals, valid = O.summary_nan_case(n, F)
    got = _summary(vals, valid, None)
    ref = O.summary(vals, valid)
    assert np.isnan(ref[:2, 2:8]).all()
    assert np.array_equal(got[:, :4], ref[:, :4], equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert _loaded()


# ====================================================================================================== rff_hist
@pytest.mark.parametrize("gid", list(O.hist_groups()))
def test_rff_hist_split_edges(gid):
    """Every column of a group of the oracle's histogram table in one launch, exact integer equality: every reference
    split with its two neighbours, min, max, a value below min and one above the last split, NaN, null rows; fp64,
    fp32, int64, uint8 and bool columns; the three integer fixtures on which a fused split moves the maximum; a
    degenerate column (2 buckets) between regular ones; the empty summary; training bounds on scoring values; bins 3 to
    16384 (the LDS limit); and 2049 rows x 3 columns, where 3 workgroups add into one column's bins."""
    bins, cols = O.hist_groups()[gid]
    got = R.numeric_hist([_d(c["values"]) for c in cols], [_d(c["valid"]) for c in cols],
                         torch.tensor([c["lo"] for c in cols], dtype=torch.float64),
                         torch.tensor([c["hi"] for c in cols], dtype=torch.float64), bins)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = O.hist_group_counts(gid)
    assert got.shape == want.shape
    bad = {c["name"]: np.flatnonzero(g != w)[:8].tolist() for c, g, w in zip(cols, got, want)
           if not np.array_equal(g, w)}
    assert not bad
    assert _loaded()
