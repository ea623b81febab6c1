"""Kernel-level oracle tests of the kernels behind the multi-class linear and MLP learners: ``csr_spmm_kernel``,
``csc_spmm_t_kernel``, ``seg_reduce_kernel``, ``softmax_epilogue_kernel``, ``colsum_kernel``
(``ops/csrc/hip/sparse_kernels.hip``), ``mlp_bias_sigmoid_kernel``, ``mlp_sigmoid_backprop_kernel``
(``ops/csrc/hip/mlp_kernels.hip``), ``mnl_epilogue_kernel`` and ``mnl_bf16_kernel`` (``ops/csrc/hip/mnl_kernels.hip``)
against tests/multiclass_oracle.py, which tests/test_multiclass_oracle.py validates against the host torch paths on the same
case tables. Each case is named after the path it forces and is the smallest shape that reaches it. Semantics go through
the Python wrappers; write guards and grid shapes go through the direct C entry points with sentinel-padded buffers.

Bounds are derived, not measured (``u = 2^-24``): integer-valued inputs are exact in fp32 and compared bitwise; real inputs
within the accumulation bounds of ``multiclass_oracle.mm_bound`` / ``tmm_bound``; softmax and sigmoid results within
``8 e32`` of the fp64 value (the oracle's docstring) plus one ``u`` for the product with the row weight."""
import numpy as np
import pytest
import torch

import multiclass_oracle as O
from transmogrifai_amd.models.mlp import _bias_sigmoid_, _sigmoid_backprop_
from transmogrifai_amd.ops import linear as LK

pytestmark = pytest.mark.gpu

PAD = 64
SENT32 = np.float32(-1.5e30)
SENT64 = np.float64(-7.25e200)
SENT16 = np.int16(0x7FC1)                 # a bf16 NaN pattern
U, U64 = O.U, O.U64


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


def _p(t):
    return None if t is None else t.data_ptr()


class Guarded:
    """A device buffer of ``count`` elements between two sentinel pads; ``body()`` checks the pads and returns the
    elements."""

    def __init__(self, count, fill, init=None):
        self.fill, self.count = fill, count
        host = np.full(PAD + count + PAD, fill, np.asarray(fill).dtype)
        if init is not None:
            host[PAD:PAD + count] = np.asarray(init, host.dtype).reshape(-1)
        self.t = _d(host)
        self.ptr = self.t.data_ptr() + PAD * host.itemsize

    def body(self):
        got = self.t.cpu().numpy()
        assert (got[:PAD] == self.fill).all() and (got[PAD + self.count:] == self.fill).all(), "pad overwritten"
        return got[PAD:PAD + self.count]


def _sync(rc):
    torch.cuda.synchronize()
    assert rc == 0


# ================================================================================================ sparse products
def _cid(C):
    if C <= 256:
        return f"C{C}-CU{-(-C // 64)}"
    return f"C{C}-chunk256_then_CU{-(-(C - 256) // 64)}_strided_output"


def _check_products(D, S, X, C, integer):
    """``mm``, ``tmm``, ``tmm(square)`` of the device design ``D`` against the oracle design ``S``: integer data bitwise,
    real data within the derived bounds; ``tmm`` twice: bit-equal."""
    V, R = O.operands(X, C, integer)
    M = D.mm(_d(V)).cpu().numpy()
    G = D.tmm(_d(R))
    Gq = D.tmm(_d(R), square=True).cpu().numpy()
    assert torch.equal(G, D.tmm(_d(R))), "tmm is not deterministic"
    G = G.cpu().numpy()
    assert M.dtype == np.float32 and G.dtype == np.float64 and M.shape == (S.N, C) and G.shape == (S.d, C)
    refM, bM = O.mm_bound(S, V)
    refG, bG = O.tmm_bound(S, R, False)
    refQ, bQ = O.tmm_bound(S, R, True)
    # the dense block taken as given: torch's fp32 GEMM of the same block, called as mm / tmm call it. The dense rows of
    # tmm are that product widened; mm is that product plus the CSR row, one more rounding (u |result|) for the addition
    if len(S.idx_d):
        dV, dR = _d(V), _d(R)
        Md = (D.Xd @ dV.index_select(0, D.idx_d)).cpu().numpy().astype(np.float64)
        ref_s, b_s = O.mm_sparse_part(S, V)
        assert (np.abs(M - (Md + ref_s)) <= b_s + U * np.abs(Md + ref_s)).all()
        assert np.array_equal(M[S.row_nnz == 0].astype(np.float64), Md[S.row_nnz == 0])      # nothing added: unchanged
        assert np.array_equal(G[S.idx_d], (D.Xd.t() @ dR).cpu().numpy().astype(np.float64))
        assert np.array_equal(Gq[S.idx_d], ((D.Xd * D.Xd).t() @ dR).cpu().numpy().astype(np.float64))
    if integer:
        assert np.array_equal(M.astype(np.float64), refM)
        assert np.array_equal(G, refG)
        assert np.array_equal(Gq, refQ)
    else:
        assert (np.abs(M - refM) <= bM).all(), float((np.abs(M - refM) - bM).max())
        assert (np.abs(G - refG) <= bG).all(), float((np.abs(G - refG) - bG).max())
        assert (np.abs(Gq - refQ) <= bQ).all(), float((np.abs(Gq - refQ) - bQ).max())


@pytest.mark.parametrize("integer", [True, False], ids=["integer_bitwise", "real_bounded"])
@pytest.mark.parametrize("C", O.SPMM_C, ids=_cid)
def test_sparse_products_multi_segment_columns_and_row_batches(C, integer, monkeypatch):
    """Segments of 70: sparse columns of 0, 1, 1 (full), 2 (last of one pair), 2 (both full) and 5 (last of one pair)
    segments; CSR rows of 0, 1, 7, 8, 9, 63, 64, 65 and 130 pairs (the tail loop alone, one exact unroll, unroll + tail,
    a full 64-batch, a second and a third batch); every column-chunk variant and its edges; above 256 columns the second
    launch writes a column slice of the wider output."""
    monkeypatch.setattr(LK, "_SEG_NNZ", O.SEG_SMALL)
    X = O.design("segs70", integer)
    S = O.Sparse(X, O.SEG_SMALL)
    D = LK.SparseDesign(_d(X))
    assert D.n_seg == S.n_seg and S.segments_of(S.ds - 1) == 5 and S.row_nnz[8] == 130
    _check_products(D, S, X, C, integer)
    assert _loaded()


@pytest.mark.parametrize("integer", [True, False], ids=["integer_bitwise", "real_bounded"])
def test_sparse_products_real_segment_length_two_segments(integer):
    """``_SEG_NNZ`` = 4096 as shipped: 20000 rows, one column at ~24 % (below ``DENSE_FRAC``): 2 segments."""
    X = O.design("seg4096_two_segments", integer)
    S = O.Sparse(X, LK._SEG_NNZ)
    D = LK.SparseDesign(_d(X))
    assert LK._SEG_NNZ == 4096 and D.n_seg == S.n_seg and S.segments_of(0) == 2
    _check_products(D, S, X, 5, integer)
    assert _loaded()


@pytest.mark.parametrize("integer", [True, False], ids=["integer_bitwise", "real_bounded"])
@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("name", O.DESIGNS_SMALL)
def test_sparse_products_degenerate_designs(name, C, integer, monkeypatch):
    """One row (every sparse column empty: no segment at all), 5 rows (a workgroup's waves 1..3 partly idle), no dense
    column, no sparse column; an all-zero sparse column and an empty row among the others."""
    monkeypatch.setattr(LK, "_SEG_NNZ", O.SEG_SMALL)
    X = O.design(name, integer)
    S = O.Sparse(X, O.SEG_SMALL)
    D = LK.SparseDesign(_d(X))
    assert D.n_seg == S.n_seg and D.ds == S.ds
    _check_products(D, S, X, C, integer)
    assert _loaded()


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("C", [1, 65, 193])
def test_csr_spmm_direct_writes_only_its_columns(C, accumulate):
    """The direct entry on the oracle's own CSR arrays, output rows ``ldm = C + 3`` wide in a sentinel buffer: nothing
    outside ``[row][0..C)`` changes; ``accumulate`` adds to what is there, otherwise overwrites. Integer data: bitwise."""
    X = O.design("segs70", True)
    S = O.Sparse(X, O.SEG_SMALL)
    V, _ = O.operands(X, C, True)
    Vs = np.ascontiguousarray(V[S.idx_s])
    ldm = C + 3
    start = np.full((S.N, ldm), SENT32, np.float32)
    init = np.random.default_rng(C).integers(-3, 4, (S.N, C)).astype(np.float32)
    if accumulate:
        start[:, :C] = init
    buf = Guarded(S.N * ldm, SENT32, start)
    rp, col, val, dV = _d(S.row_ptr), _d(S.col), _d(S.val), _d(Vs)
    _sync(_lib().tmog_hip_csr_spmm(_p(rp), _p(col), _p(val), S.N, _p(dV), C, buf.ptr, ldm, accumulate, _st()))
    got = buf.body().reshape(S.N, ldm)
    assert (got[:, C:] == SENT32).all()
    want = O.xv(S.Xs, Vs)[0] + (init if accumulate else 0)
    assert np.array_equal(got[:, :C].astype(np.float64), want)
    assert _loaded()


@pytest.mark.parametrize("C", [1, 129])
def test_csc_spmm_t_direct_segment_partials_in_order(C):
    """The direct entry on the oracle's own segmented CSC, R rows ``ldr = C + 5`` wide with NaN in the padding columns:
    every segment's partial row equals the sum of exactly its pairs (a mis-ordered or mis-cut segment shows here), G
    their sum per column; the pads around ``partial`` and ``G`` keep the sentinel. Integer data: bitwise."""
    X = O.design("segs70", True)
    S = O.Sparse(X, O.SEG_SMALL)
    _, R = O.operands(X, C, True)
    ldr = C + 5
    Rw = np.full((S.N, ldr), np.nan, np.float32)
    Rw[:, :C] = R
    part, G = Guarded(S.n_seg * C, SENT32), Guarded(S.ds * C, SENT64)
    sb, row, val, cs, dR = _d(S.seg_begin), _d(S.csc_row), _d(S.csc_val), _d(S.col_seg), _d(Rw)
    _sync(_lib().tmog_hip_csc_spmm_t(_p(sb), _p(row), _p(val), S.n_seg, _p(cs), S.ds, _p(dR), C, ldr, part.ptr, G.ptr,
                                     _st()))
    want = np.stack([(S.csc_val[a:b, None].astype(np.float64) * R[S.csc_row[a:b]]).sum(0)
                     for a, b in zip(S.seg_begin[:-1], S.seg_begin[1:])])
    assert np.array_equal(part.body().reshape(S.n_seg, C).astype(np.float64), want)
    assert np.array_equal(G.body().reshape(S.ds, C), O.xtr(S.Xs, R)[0])
    assert _loaded()


def test_csc_spmm_t_direct_no_segments_gives_zeros():
    """``n_seg = 0`` with ``ds > 0`` (every sparse column empty): G is all zeros, not what the buffer held."""
    ds, C = 5, 7
    G, part = Guarded(ds * C, SENT64), Guarded(C, SENT32)
    sb, cs = _d(np.zeros(1, np.int64)), _d(np.zeros(ds + 1, np.int64))
    row, val, dR = _d(np.zeros(1, np.int32)), _d(np.ones(1, np.float32)), _d(np.ones((3, C), np.float32))
    _sync(_lib().tmog_hip_csc_spmm_t(_p(sb), _p(row), _p(val), 0, _p(cs), ds, _p(dR), C, C, part.ptr, G.ptr, _st()))
    assert (G.body() == 0).all() and (part.body() == SENT32).all()
    assert _loaded()


# ======================================================================================================== colsum
@pytest.mark.parametrize("N,nblk", O.COLSUM_SHAPES,
                         ids=["below_boundary", "on_boundary", "past_boundary_empty_last_block", "more_blocks_than_rows",
                              "one_row", "three_real_slices"])
@pytest.mark.parametrize("C", O.COLSUM_C)
def test_colsum_blocks_and_thread_stride(C, N, nblk):
    """Per-block fp64 column sums: rows below, on and past ``nblk * rows_per_blk``; blocks without rows write zeros; C
    across the 256-thread stride. The sum of the partials is within ``N 2^-52 sum |x|`` of the exact sum."""
    A = O.colsum_case(N, C)
    part = Guarded(nblk * C, SENT64)
    dA = _d(A)
    _sync(_lib().tmog_hip_colsum(_p(dA), N, C, nblk, part.ptr, _st()))
    got = part.body().reshape(nblk, C)
    rpb = -(-N // nblk)
    for b in range(nblk):
        if b * rpb >= N:
            assert (got[b] == 0).all(), b
    exact, ab = O.exact_colsum(A)
    assert (np.abs(got.sum(0) - exact) <= N * U64 * ab).all()
    assert _loaded()


# ======================================================================================================= softmax
def _softmax_expect(M, bias, y, W, P, K, kind="softmax"):
    m32 = O.margins_f32(M, bias, P, K)
    loss, R, lse = O.softmax_loss_residual(m32, y, W)
    ep, el = O.softmax_e32(m32, y)
    Wd = W.astype(np.float64)
    tolL = O.allow_e32(kind + "_loss", el) * Wd * np.maximum(1.0, np.abs(lse)) + U * np.abs(loss)
    tolR = O.allow_e32(kind + "_p", ep) * Wd[:, :, None] + U * np.abs(R)
    return loss, R, tolL, tolR


@pytest.mark.parametrize("margins", O.SOFTMAX_MARGINS)
@pytest.mark.parametrize("N", O.SOFTMAX_N)
@pytest.mark.parametrize("P,K", O.SOFTMAX_PK, ids=O.SOFTMAX_PK_IDS)
def test_softmax_epilogue_against_oracle(P, K, N, margins):
    """K = 1 and 2, K above 16, P * K up to 240; rows around a 256-thread block; ordinary and saturated margins (one class
    ahead by 120, all equal, +-1e4 under a bias of the opposite sign); weights 0, 1 and non-integers; labels -1 and K on a
    few rows (loss 0, no one-hot term). Direct entry: W rows ``ldw = P + 3`` wide with NaN padding, Lw and M in sentinel
    buffers; ``grad = 0`` leaves M bit-unchanged. Wrapper: f and rsum as sums, R bit-equal to the direct run."""
    M, bias, y, W = O.softmax_case(P, K, N, margins)
    C = P * K
    loss, R, tolL, tolR = _softmax_expect(M, bias, y, W, P, K)
    ldw = P + 3
    Ww = np.full((N, ldw), np.nan, np.float32)
    Ww[:, :P] = W
    db, dy, dW = _d(bias), _d(y), _d(Ww)
    Mb, Lw = Guarded(N * C, SENT32, M), Guarded(N * P, SENT32)
    _sync(_lib().tmog_hip_softmax_epilogue(Mb.ptr, N, P, K, _p(db), _p(dy), _p(dW), ldw, Lw.ptr, 0, _st()))
    assert np.array_equal(O.bits(Mb.body()), O.bits(M.reshape(-1))), "grad = 0 changed M"
    L0 = Lw.body().reshape(N, P).copy()
    assert (np.abs(L0 - loss) <= tolL).all(), float((np.abs(L0 - loss) - tolL).max())
    _sync(_lib().tmog_hip_softmax_epilogue(Mb.ptr, N, P, K, _p(db), _p(dy), _p(dW), ldw, Lw.ptr, 1, _st()))
    Rg = Mb.body().reshape(N, P, K).copy()
    assert np.array_equal(O.bits(Lw.body().reshape(N, P)), O.bits(L0))
    assert (np.abs(Rg - R) <= tolR).all(), float((np.abs(Rg - R) - tolR).max())
    bad = (y < 0) | (y >= K)
    assert (L0[bad] == 0).all()
    # the wrapper: sums
    dM = _d(M)
    f, rs = LK.softmax_objective(dM, dy, _d(W), db, P, K, True)
    torch.cuda.synchronize()
    assert np.array_equal(O.bits(dM.cpu().numpy()), O.bits(Rg.reshape(N, C)))
    f, rs = f.cpu().numpy(), rs.cpu().numpy()
    assert (np.abs(f - loss.sum(0)) <= tolL.sum(0) + N * U64 * np.abs(loss).sum(0)).all()
    Rf, tf = R.reshape(N, C), tolR.reshape(N, C)
    assert (np.abs(rs - Rf.sum(0)) <= tf.sum(0) + N * U64 * np.abs(Rf).sum(0)).all()
    dM = _d(M)
    f0, rs0 = LK.softmax_objective(dM, dy, _d(W), db, P, K, False)
    assert rs0 is None and np.array_equal(f0.cpu().numpy(), f) and np.array_equal(O.bits(dM.cpu().numpy()), O.bits(M))
    assert _loaded()


def test_softmax_epilogue_grid_stride():
    """``N * P = 65536 * 256 + 777`` with P = 1, K = 2: the grid is capped at 65536 blocks, so 777 threads take a second
    element. The rows tile a 4099-row pattern: every period of the output must be bit-equal to the first, and the first
    and the last rows are checked against the oracle."""
    P, K, N, L = 1, 2, O.GRID_STRIDE_TOTAL, O.GRID_PERIOD
    M, bias, y, W = O.softmax_case(P, K, L, "ordinary")
    loss, R, tolL, tolR = _softmax_expect(M, bias, y, W, P, K)
    idx = torch.arange(N, device="cuda") % L
    dM, dy, dW, db = _d(M)[idx].contiguous(), _d(y)[idx].contiguous(), _d(W)[idx].contiguous(), _d(bias)
    Lw = torch.full((N, P), float(SENT32), device="cuda")
    _sync(_lib().tmog_hip_softmax_epilogue(_p(dM), N, P, K, _p(db), _p(dy), _p(dW), P, _p(Lw), 1, _st()))
    assert torch.equal(dM, dM[:L][idx]) and torch.equal(Lw, Lw[:L][idx])
    Rg, Lg = dM[:L].cpu().numpy().reshape(L, P, K), Lw[:L].cpu().numpy()
    assert (np.abs(Rg - R) <= tolR).all() and (np.abs(Lg - loss) <= tolL).all()
    tail = (np.arange(N - 777, N) % L)
    assert (np.abs(dM[N - 777:].cpu().numpy().reshape(777, P, K) - R[tail]) <= tolR[tail]).all()
    assert _loaded()


# ================================================================================================== mnl_epilogue
def _bf16_dev(count):
    return Guarded(count, SENT16)


def _hi_lo(body, N, C):
    h = O.bf16_from_bits(body.view(np.uint16).reshape(N, 2 * C))
    return h[:, :C], h[:, C:]


def _check_split(hi, lo, R, tolR):
    """``[hi | lo]`` of a residual: the sum is the fp32 residual to ``2^-17`` relative (both roundings to nearest), hi is
    the bf16 rounding of it to within one bf16 ulp, lo is at most half an ulp of hi."""
    s = hi.astype(np.float64) + lo.astype(np.float64)
    tol = tolR + 2.0 ** -17 * np.abs(R)
    assert (np.abs(s - R) <= tol).all(), float((np.abs(s - R) - tol).max())
    assert (np.abs(lo) <= 2.0 ** -8 * np.abs(hi) + 2.0 ** -126).all(), "lo is not the small part"
    assert (np.abs(hi - O.bf16_round((hi + lo).astype(np.float32))) <= O.bf16_ulp(hi)).all()


@pytest.mark.parametrize("blocks", ["empty_last_blocks", "one_block_every_pass"])
@pytest.mark.parametrize("N", O.MNL_N)
@pytest.mark.parametrize("K", O.MNL_K)
@pytest.mark.parametrize("P", O.MNL_P, ids=["P1", "P32", "P100_inactive_threads", "P256_one_row_per_pass"])
def test_mnl_epilogue_against_oracle(P, K, N, blocks):
    """P = 1 (256 rows per pass), 32 (8 rows), 100 (2 rows, 56 inactive threads), 256 (one row per pass); K = 1, 2, 16; the
    identity weight map (null) and a many-to-one map; W rows two wider than the columns used. Block counts: one that
    leaves the last block(s) without rows (their partial rows are zero; at N = 257 the blocks hold 12 rows, so the row
    loop repeats only from P = 32 up), and a single block, whose row loop takes every pass (at P = 1 and N = 257 a second
    pass of one row). ``hi + lo`` against the oracle's R, the split itself, f and r partials as sums; ``grad = 0`` leaves
    a sentinel-filled R2 untouched and gives the same partials."""
    M2, bias, y, wid, wmp = O.mnl_case(P, K, N)
    C = P * K
    m32 = O.mnl_margins_f32(M2, bias, P, K)
    ep, el = O.softmax_e32(m32, y)
    nblk = O.empty_tail_blocks(N) if blocks == "empty_last_blocks" else 1
    rpb = -(-N // nblk)
    assert (nblk - 1) * rpb >= N or nblk == 1
    dM2, db, dy = _d(M2), _d(bias), _d(y)
    for W, wmap in (wid, wmp):
        w = (W[:, :P] if wmap is None else W[:, wmap]).astype(np.float64)
        loss, R, lse = O.softmax_loss_residual(m32, y, w)
        tolL = O.allow_e32("mnl_loss", el) * w * np.maximum(1.0, np.abs(lse)) + U * np.abs(loss)
        tolR = (O.allow_e32("mnl_p", ep) * w[:, :, None] + U * np.abs(R)).reshape(N, C)
        R = R.reshape(N, C)
        dW, dm = _d(W), _d(wmap)
        out = {}
        for grad in (1, 0):
            R2, fp, rp = _bf16_dev(N * 2 * C), Guarded(nblk * P, SENT64), Guarded(nblk * C, SENT64)
            _sync(_lib().tmog_hip_mnl_epilogue(_p(dM2), N, P, K, _p(db), _p(dy), _p(dW), W.shape[1], _p(dm), grad,
                                               R2.ptr, fp.ptr, rp.ptr, nblk, _st()))
            out[grad] = (R2.body(), fp.body().reshape(nblk, P), rp.body().reshape(nblk, C))
        body, fpart, rpart = out[1]
        assert (out[0][0] == SENT16).all(), "grad = 0 wrote R2"
        assert np.array_equal(out[0][1], fpart) and np.array_equal(out[0][2], rpart)
        for b in range(nblk):
            if b * rpb >= N:
                assert (fpart[b] == 0).all() and (rpart[b] == 0).all(), b
        assert (np.abs(fpart.sum(0) - loss.sum(0)) <= tolL.sum(0) + N * U64 * np.abs(loss).sum(0)).all()
        assert (np.abs(rpart.sum(0) - R.sum(0)) <= tolR.sum(0) + N * U64 * np.abs(R).sum(0)).all()
        hi, lo = _hi_lo(body, N, C)
        _check_split(hi, lo, R, tolR)
    assert _loaded()


# ====================================================================================================== mnl_bf16
def _run_mnl_bf16(X, Vhi, Vlo, bias, y, W, wcol, K, pc, N, dpad, nblk, extra, grad):
    npad, NC = X.shape[0], K * 32
    ldx = dpad + extra
    Xw = np.full((npad, ldx), 0x7FC0, np.uint16)              # NaN in the padding columns of a wider row
    Xw[:, :dpad] = O.bf16_bits(X)
    Vt = np.concatenate([O.bf16_bits(Vhi), O.bf16_bits(Vlo)], 0)
    dX, dV = _d(Xw.view(np.int16)), _d(Vt.view(np.int16))
    db, dy, dW, dwc = _d(bias), _d(y), _d(W), _d(wcol)
    R2, fp, rp = _bf16_dev(npad * 2 * NC), Guarded(nblk * 8 * 32, SENT64), Guarded(nblk * 8 * NC, SENT64)
    _sync(_lib().tmog_hip_mnl_bf16(_p(dX), ldx, N, dpad, _p(dy), _p(dW), W.shape[1], _p(dwc), pc, K, _p(dV), _p(db),
                                   grad, R2.ptr, fp.ptr, rp.ptr, nblk, _st()))
    return R2.body().reshape(npad, 2 * NC), fp.body().reshape(nblk * 8, 32), rp.body().reshape(nblk * 8, NC)


def _mnl_bf16_expect(X, Vhi, Vlo, bias, y, W, wcol, K, pc, N, dpad):
    m, mabs = O.mnl_bf16_reference(X, Vhi, Vlo, bias, N, K)                   # [N, 32, K]
    w = np.where(np.arange(32)[None, :] < pc, W[:, wcol].astype(np.float64), 0.0)
    loss, R, lse = O.softmax_loss_residual(m, y, w)
    ep, el = O.softmax_e32(m.astype(np.float32), y)
    dm = (2 * dpad + 2) * U * mabs.max(2)                                      # fp32 accumulation of the margins
    tolL = w * (2 * dm + O.allow_e32("bf16_loss", el) * np.maximum(1.0, np.abs(lse))) + U * np.abs(loss)
    tolR = w[:, :, None] * (2 * dm[:, :, None] + O.allow_e32("bf16_p", ep)) + U * np.abs(R)
    return loss, R, tolL, tolR, (ep, el), w, lse


def _problem_major(a, N, K):
    """``[N, K * 32]`` class-major columns -> ``[N, 32, K]``."""
    return a.reshape(N, K, 32).transpose(0, 2, 1)


@pytest.mark.parametrize("integer", [False, True], ids=["real", "integer_exact_margins"])
@pytest.mark.parametrize("cid,K,pc,N,dpad,nblk,extra", O.MNL_BF16_CASES, ids=[c[0] for c in O.MNL_BF16_CASES])
def test_mnl_bf16_against_oracle(cid, K, pc, N, dpad, nblk, extra, integer):
    """K = 2, 3, 6; pc = 1, 31, 32 (the padding problems hold non-zero coefficients and must add exactly 0 to f and r);
    N below, on and past a 32-row tile and 300; one, two and three 64-feature chunks; one block walking 19 tiles in 3
    rounds with dead waves in the last; 4 blocks for 2 tiles (waves with no tile); rows wider than ``dpad``. Reference:
    fp64 on the bf16 X and on ``V_hi + V_lo`` as passed; margin error ``(2 dpad + 2) u sum |x| |v|``, carried into the
    loss and the probabilities by a factor 2. Rows past N of R2 keep the sentinel."""
    X, Vhi, Vlo, bias, y, W, wcol = O.mnl_bf16_case(K, pc, N, dpad, integer)
    NC = K * 32
    loss, R, tolL, tolR, _, _, _ = _mnl_bf16_expect(X, Vhi, Vlo, bias, y, W, wcol, K, pc, N, dpad)
    R2, fp, rp = _run_mnl_bf16(X, Vhi, Vlo, bias, y, W, wcol, K, pc, N, dpad, nblk, extra, 1)
    R0, fp0, rp0 = _run_mnl_bf16(X, Vhi, Vlo, bias, y, W, wcol, K, pc, N, dpad, nblk, extra, 0)
    assert (R0 == SENT16).all(), "the value-only launch wrote R2"
    assert (R2[N:] == SENT16).all(), "rows past N written"
    for fq, rq in ((fp, rp), (fp0, rp0)):
        f, r = fq.sum(0), _problem_major(rq.sum(0)[None], 1, K)[0]               # [32], [32, K]
        assert (f[pc:] == 0).all() and (r[pc:] == 0).all(), "a padding problem contributes"
        assert (np.abs(f - loss.sum(0)) <= tolL.sum(0) + N * U64 * np.abs(loss).sum(0)).all()
        assert (np.abs(r - R.sum(0)) <= tolR.sum(0) + N * U64 * np.abs(R).sum(0)).all()
    h = O.bf16_from_bits(R2[:N].view(np.uint16))
    hi, lo = _problem_major(h[:, :NC], N, K), _problem_major(h[:, NC:], N, K)
    _check_split(hi, lo, R, tolR)
    assert (hi[:, pc:] == 0).all() and (lo[:, pc:] == 0).all()
    assert _loaded()


@pytest.mark.parametrize("K", [2, 3, 6])
def test_mnl_bf16_agrees_with_mnl_epilogue_on_exact_margins(K):
    """Integer X and V_hi, V_lo = 0: the margins are exact in fp32 whatever the order. ``mnl_epilogue_kernel`` fed the
    same margins must agree with the fused kernel to the transcendental allowance alone (plus the two bf16 splits)."""
    pc, N, dpad = 32, 300, 128
    X, Vhi, Vlo, bias, y, W, wcol = O.mnl_bf16_case(K, pc, N, dpad, True)
    NC = K * 32
    _, R, _, _, (ep, el), w, lse = _mnl_bf16_expect(X, Vhi, Vlo, bias, y, W, wcol, K, pc, N, dpad)
    R2, fp, rp = _run_mnl_bf16(X, Vhi, Vlo, bias, y, W, wcol, K, pc, N, dpad, 2, 0, 1)
    m = (X[:N].astype(np.float64) @ Vhi.astype(np.float64).T)                   # exact integers, class-major columns
    assert np.array_equal(m, m.astype(np.float32)) and np.abs(m).max() < 2 ** 20
    Mp = _problem_major(m, N, K).reshape(N, NC).astype(np.float32)
    M2 = np.concatenate([Mp, np.zeros_like(Mp)], 1)
    bp = bias.reshape(K, 32).T.reshape(-1).copy()
    E2, ef, er = _bf16_dev(N * 2 * NC), Guarded(3 * 32, SENT64), Guarded(3 * NC, SENT64)
    dM2, db, dy, dW, dwc = _d(M2), _d(bp), _d(y), _d(W), _d(wcol)
    _sync(_lib().tmog_hip_mnl_epilogue(_p(dM2), N, 32, K, _p(db), _p(dy), _p(dW), W.shape[1], _p(dwc), 1, E2.ptr,
                                       ef.ptr, er.ptr, 3, _st()))
    aL = O.allow_e32("bf16_loss", el) * w * np.maximum(1.0, np.abs(lse))
    aR = O.allow_e32("bf16_p", ep) * w[:, :, None]
    f_e, r_e = ef.body().reshape(3, 32).sum(0), er.body().reshape(3, 32, K).sum(0)
    f_f, r_f = fp.sum(0), _problem_major(rp.sum(0)[None], 1, K)[0]
    assert (np.abs(f_e - f_f) <= aL.sum(0)).all() and (np.abs(r_e - r_f) <= aR.sum(0)).all()
    he, le = _hi_lo(E2.body(), N, NC)
    s_e = (he.astype(np.float64) + le).reshape(N, 32, K)
    h = O.bf16_from_bits(R2[:N].view(np.uint16))
    s_f = _problem_major(h[:, :NC].astype(np.float64) + h[:, NC:], N, K)
    assert (np.abs(s_e - s_f) <= aR + 2 * 2.0 ** -17 * np.abs(R)).all()
    assert _loaded()


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused_kernel", "gemm_then_epilogue"])
@pytest.mark.parametrize("K", [2, 3])
def test_mnl_objective_bf16_wrapper(K, fused, monkeypatch):
    """``mnl_objective_bf16`` end to end on an integer-valued (bf16-exact, unshifted) design: f, rsum and G against the
    fp64 objective of ``V_hi + V_lo``; G's bound adds the library GEMM over ``[R_hi | R_lo]`` in 16 row chunks."""
    monkeypatch.setenv("TMOG_MNL_FUSED_BF16", fused)
    N, d, P = 300, 70, 3
    rng = np.random.default_rng(K)
    X = rng.integers(-2, 3, (N, d)).astype(np.float32)
    V = (rng.standard_normal((d, P * K)) * 0.2).astype(np.float32)
    bias = rng.standard_normal(P * K).astype(np.float32)
    y = O._labels(rng, N, K, out_of_range=False)
    W = O._weights(rng, (N, P))
    D = LK.Bf16Design.of(_d(X), pad=False)
    assert not D.shifted and D.dpad == 128
    f, rs, G = LK.mnl_objective_bf16(D, _d(V), _d(y), _d(W), _d(bias), P, K, True)
    f0, rs0, G0 = LK.mnl_objective_bf16(D, _d(V), _d(y), _d(W), _d(bias), P, K, False)
    torch.cuda.synchronize()
    assert G0 is None
    f, rs, G, f0 = f.cpu().numpy(), rs.cpu().numpy(), G.cpu().numpy(), f0.cpu().numpy()
    Vhi, Vlo = O.bf16_split(V)
    Vs = Vhi.astype(np.float64) + Vlo
    m = (X.astype(np.float64) @ Vs + bias).reshape(N, P, K)
    mabs = (np.abs(X).astype(np.float64) @ np.abs(Vs) + np.abs(bias)).reshape(N, P, K)
    w = W.astype(np.float64)
    loss, R, lse = O.softmax_loss_residual(m, y, w)
    ep, el = O.softmax_e32(m.astype(np.float32), y)
    dm = (2 * D.dpad + 2) * U * mabs.max(2)
    tolL = w * (2 * dm + O.allow_e32("bf16_loss", el) * np.maximum(1.0, np.abs(lse))) + U * np.abs(loss)
    tolR = (w[:, :, None] * (2 * dm[:, :, None] + O.allow_e32("bf16_p", ep)) + U * np.abs(R)).reshape(N, P * K)
    R = R.reshape(N, P * K)
    assert (np.abs(f - loss.sum(0)) <= tolL.sum(0) + N * U64 * np.abs(loss).sum(0)).all()
    assert (np.abs(f0 - loss.sum(0)) <= tolL.sum(0) + N * U64 * np.abs(loss).sum(0)).all()
    assert (np.abs(rs - R.sum(0)) <= tolR.sum(0) + N * U64 * np.abs(R).sum(0)).all()
    refG, absG = O.xtr(X, R)
    rows = D.Xb.shape[0] // 16
    tolG = np.abs(X).astype(np.float64).T @ (tolR + 2.0 ** -17 * np.abs(R)) + (rows + 2) * U * absG
    assert (np.abs(G - refG) <= tolG).all(), float((np.abs(G - refG) - tolG).max())
    assert _loaded()


# =========================================================================================================== mlp
@pytest.mark.parametrize("N", O.MLP_N)
@pytest.mark.parametrize("B", O.MLP_B, ids=["B1", "B7", "B256", "B257_thread_stride", "B600_thread_stride"])
@pytest.mark.parametrize("P", O.MLP_P)
def test_mlp_bias_sigmoid_against_oracle(P, B, N):
    """In place in a sentinel-padded buffer; the wrapper gives the same bits."""
    Z, b = O.sigmoid_case(P, N, B)
    ref, e32 = O.bias_sigmoid(Z, b)
    buf, db = Guarded(Z.size, SENT32, Z), _d(b)
    _sync(_lib().tmog_hip_mlp_bias_sigmoid(buf.ptr, P, N, B, _p(db), _st()))
    got = buf.body().reshape(P, N, B)
    assert (np.abs(got - ref) <= O.allow_e32("sigmoid", e32)).all(), float(np.abs(got - ref).max())
    assert (got >= 0).all() and (got <= 1).all()
    wrapped = _bias_sigmoid_(_d(Z), db)
    torch.cuda.synchronize()
    assert np.array_equal(O.bits(wrapped.cpu().numpy()), O.bits(got))
    assert _loaded()


def test_mlp_bias_sigmoid_saturation():
    """z = 0, -0, +-20, +-87, +-89, +-100, +-1e4 (``__expf`` overflows from about 88.7): finite, in [0, 1], monotone."""
    z = np.array(O.SIGMOID_Z, np.float32)
    Z = np.repeat(z[None, :, None], 3, 2).copy()                      # P = 1, N = 12, B = 3
    b = np.zeros((1, 3), np.float32)
    ref, e32 = O.bias_sigmoid(Z, b)
    got = _bias_sigmoid_(_d(Z), _d(b)).cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    assert (np.diff(got[0], axis=0) >= 0).all(), got[0, :, 0]
    assert (np.abs(got - ref) <= O.allow_e32("sigmoid", e32)).all()
    assert got[0, 5, 0] == got[0, 6, 0]
    assert _loaded()


def test_mlp_bias_sigmoid_grid_stride():
    """``P * N * B = 65536 * 256 + 777`` (N = 172969, B = 97): 777 threads take a second element. The flat input tiles a
    pattern of 43 rows, so every period of the output equals the first, which is checked against the oracle."""
    P, N, B = O.MLP_GRID_PNB
    assert P * N * B == O.GRID_STRIDE_TOTAL
    rows = 43
    Zp, b = O.sigmoid_case(1, rows, B)
    ref, e32 = O.bias_sigmoid(Zp, b)
    L = rows * B
    idx = torch.arange(P * N * B, device="cuda") % L
    dZ, db = _d(Zp.reshape(-1))[idx].contiguous(), _d(b)
    _sync(_lib().tmog_hip_mlp_bias_sigmoid(_p(dZ), P, N, B, _p(db), _st()))
    assert torch.equal(dZ, dZ[:L][idx])
    assert (np.abs(dZ[:L].cpu().numpy() - ref.reshape(-1)) <= O.allow_e32("sigmoid", e32)).all()
    assert _loaded()


@pytest.mark.parametrize("N", O.MLP_N, ids=["N1", "N2047", "N2048_wrapper_one_block", "N2049_wrapper_two_blocks",
                                            "N5000"])
@pytest.mark.parametrize("B", O.MLP_B, ids=["B1", "B7", "B256", "B257_thread_stride", "B600_thread_stride"])
@pytest.mark.parametrize("P", O.MLP_P)
def test_mlp_sigmoid_backprop_against_oracle(P, B, N):
    """nblk = 1, 3 and one that leaves the last block(s) without rows (a row slice that ends before N, zero partials):
    the written D is within ``4 u |d a (1 - a)|`` of the oracle (three roundings), the partials sum to the fp64 sum of the
    kernel's own D within ``N 2^-52 sum |d|``, A is bit-unchanged, the pads around D and ``part`` keep the sentinel."""
    D, A = O.backprop_case(P, N, B)
    want, _ = O.sigmoid_backprop(D, A)
    tol = 4 * U * np.abs(want) + 2.0 ** -149
    dA = _d(A)
    first = None
    for nblk in O.mlp_nblks(N):
        buf, part = Guarded(D.size, SENT32, D), Guarded(P * nblk * B, SENT64)
        _sync(_lib().tmog_hip_mlp_sigmoid_backprop(buf.ptr, _p(dA), P, N, B, nblk, part.ptr, _st()))
        got = buf.body().reshape(P, N, B)
        assert (np.abs(got - want) <= tol).all(), nblk
        parts = part.body().reshape(P, nblk, B)
        rpb = -(-N // nblk)
        for blk in range(nblk):
            if blk * rpb >= N:
                assert (parts[:, blk] == 0).all(), (nblk, blk)
        own = got.astype(np.float64)
        assert (np.abs(parts.sum(1) - own.sum(1)) <= N * U64 * np.abs(own).sum(1)).all(), nblk
        if first is None:
            first = got.copy()
        assert np.array_equal(O.bits(got), O.bits(first)), nblk
    assert np.array_equal(O.bits(dA.cpu().numpy()), O.bits(A)), "A changed"
    dD = _d(D)
    sums = _sigmoid_backprop_(dD, dA).cpu().numpy()
    assert np.array_equal(O.bits(dD.cpu().numpy()), O.bits(first))
    own = first.astype(np.float64)
    assert (np.abs(sums - own.sum(1)) <= N * U64 * np.abs(own).sum(1)).all()
    assert _loaded()
