"""Plain oracle of the kernels behind the multi-class linear and MLP learners: ``csr_spmm_kernel``, ``csc_spmm_t_kernel``,
``seg_reduce_kernel``, ``softmax_epilogue_kernel``, ``colsum_kernel`` (``ops/csrc/hip/sparse_kernels.hip``),
``mlp_bias_sigmoid_kernel``, ``mlp_sigmoid_backprop_kernel`` (``ops/csrc/hip/mlp_kernels.hip``), ``mnl_epilogue_kernel`` and
``mnl_bf16_kernel`` (``ops/csrc/hip/mnl_kernels.hip``). numpy and the standard library only: nothing of the project, no torch.
One fp64 function per operation, written from its definition, and the *case tables* that
tests/test_multiclass_kernels_gpu.py runs on the device and tests/test_multiclass_oracle.py runs on the host torch paths,
so both sides are judged on the same inputs.

Out-of-range labels. The three device epilogues (``softmax_epilogue_kernel``, ``mnl_epilogue_kernel``,
``mnl_bf16_kernel``) document one rule for a label outside ``[0, K)``: the row's loss is 0 and its residual has no
one-hot term, ``R = w softmax``. ``softmax_loss_residual`` follows that rule. The host path of ``MLPObjective._output``
clamps the label instead; it is not changed, because ``OpMultilayerPerceptronClassifier.fit_batch`` cannot pass such a
label: it takes ``K = max(y) + 1`` and refuses ``layers[-1] < K``, so every label it hands on is below ``layers[-1]``
(and the label column of a classifier is a non-negative class index). The host multinomial path one-hot encodes the label
and raises on one out of range. The host comparisons of tests/test_multiclass_oracle.py therefore use in-range labels.

Tolerances of the fast intrinsics. ``__expf``, ``__logf`` and the hardware reciprocal have no stated bound in this
project, so the tests do not take one from the kernels' output either. For every softmax / sigmoid case the oracle
evaluates the kernel's formula twice on the case's own fp32 inputs: in fp64, and in numpy ``float32`` arithmetic with
``float32`` ``exp`` / ``log`` (every operation rounded once, in the kernel's order). ``e32`` is the largest difference of the
two at unit weight: for probabilities and sigmoids as it is, for the loss divided by ``max(1, |lse|)``. A device result may
differ from the fp64 value by ``8 e32`` (a few ulp per intrinsic beyond correctly rounded ones), times ``w`` for R and times
``w max(1, |lse|)`` for the loss, plus the accumulation terms derived in the tests. ``E32`` below records, per kernel, the
largest ``e32`` over the kernel's case table as measured on the host (numpy ``float32`` ``exp`` / ``log``);
``allow_e32`` caps each case's own figure with it, so a platform whose ``float32`` functions are worse cannot widen a test.
tests/test_multiclass_oracle.py checks that every case's ``e32`` is at or below its entry.

    kernel                     quantity              measured maximum   E32 (ceiling)
    softmax_epilogue_kernel    softmax probability   3.60e-07           4.5e-07
    softmax_epilogue_kernel    loss / max(1, |lse|)  3.73e-07           4.7e-07
    mnl_epilogue_kernel        softmax probability   3.60e-07           4.5e-07
    mnl_epilogue_kernel        loss / max(1, |lse|)  4.00e-07           5.0e-07
    mnl_bf16_kernel            softmax probability   2.20e-07           2.8e-07
    mnl_bf16_kernel            loss / max(1, |lse|)  6.12e-07           7.7e-07
    mlp_bias_sigmoid_kernel    sigmoid               9.67e-08           1.3e-07

The ceilings are the measured maxima plus a quarter, rounded up to two digits: room for another host's ``float32``
``exp`` / ``log`` being an ulp off this one's, not for the device. The figures are a few fp32 ulp of 1.0 (``2^-23 =
1.19e-7``): a probability is a product of a rounded exponential and a rounded reciprocal of a sum of up to 20 rounded
terms; the loss is a difference of two rounded numbers of the size of ``lse``.
"""
import math

import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32
U64 = 2.0 ** -52          # the fp64 bound used for fixed-order fp64 sums: n * U64 * sum |x|
F32, F64 = np.float32, np.float64

E32 = {
    "softmax_p": 4.5e-7, "softmax_loss": 4.7e-7,
    "mnl_p": 4.5e-7, "mnl_loss": 5.0e-7,
    "bf16_p": 2.8e-7, "bf16_loss": 7.7e-7,
    "sigmoid": 1.3e-7,
}


def allow_e32(kind, e32):
    """The transcendental allowance of one case: 8 x its own e32, capped by the table."""
    return 8.0 * min(float(e32), E32[kind])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ======================================================================================================== bf16
def bf16_round(a):
    """fp32 -> nearest bf16 (ties to even), returned as fp32."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(a))


def bf16_bits(a):
    """The 16-bit patterns of bf16-exact fp32 values."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not (b & 0xFFFF).any()
    return (b >> 16).astype(np.uint16).reshape(np.shape(a))


def bf16_from_bits(h):
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(h))


def bf16_split(r):
    """``hi = bf16(r)``, ``lo = bf16(r - hi)`` (the subtraction in fp32, exact here), both as fp32."""
    r = np.asarray(r, np.float32)
    hi = bf16_round(r)
    lo = bf16_round((r - hi).astype(np.float32))
    return hi, lo


def bf16_ulp(a):
    """Spacing of bf16 numbers at |a| (8 significand bits)."""
    a = np.abs(np.asarray(a, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, 2.0 ** (e - 7), 2.0 ** -133)


# ================================================================================================= sparse design
class Sparse:
    """CSR + segmented CSC of the sparse columns and the dense/sparse column split of a dense matrix, built with plain
    numpy scans: a column is dense when more than ``dense_frac`` of the rows are non-zero; CSR pairs in row then column
    order; CSC pairs in column then row order, every column's run cut into segments of at most ``seg`` pairs, listed
    in order (``seg_begin`` has one more entry, the pair count; ``col_seg[j]`` is column j's first segment)."""

    def __init__(self, X, seg, dense_frac=0.25):
        X = np.asarray(X, np.float32)
        N, d = X.shape
        self.X, self.N, self.d, self.seg = X, N, d, seg
        nz = (X != 0).sum(0) if N else np.zeros(d, np.int64)
        dense = nz > dense_frac * max(N, 1)
        self.idx_d = np.flatnonzero(dense).astype(np.int64)
        self.idx_s = np.flatnonzero(~dense).astype(np.int64)
        Xs = X[:, self.idx_s]
        self.Xs, self.Xd = Xs, X[:, self.idx_d]
        self.ds = len(self.idx_s)
        r, c = np.nonzero(Xs)                                   # row-major scan
        self.row_nnz = np.bincount(r, minlength=N).astype(np.int64)
        self.row_ptr = np.concatenate([[0], np.cumsum(self.row_nnz)]).astype(np.int64)
        self.col = c.astype(np.int32)
        self.val = Xs[r, c].astype(np.float32)
        self.nnz = len(r)
        c2, r2 = np.nonzero(Xs.T)                               # column-major scan
        self.csc_row = r2.astype(np.int32)
        self.csc_val = Xs[r2, c2].astype(np.float32)
        self.col_cnt = np.bincount(c2, minlength=self.ds).astype(np.int64)
        seg_begin, col_seg, at = [], [0], 0
        for j in range(self.ds):
            for a in range(0, int(self.col_cnt[j]), seg):
                seg_begin.append(at + a)
            at += int(self.col_cnt[j])
            col_seg.append(len(seg_begin))
        self.n_seg = len(seg_begin)
        self.seg_begin = np.asarray(seg_begin + [self.nnz], np.int64)
        self.col_seg = np.asarray(col_seg, np.int64)

    def segments_of(self, j):
        return int(self.col_seg[j + 1] - self.col_seg[j])


def xv(X, V):
    """``X V`` and ``|X| |V|`` in fp64."""
    X, V = np.asarray(X, F64), np.asarray(V, F64)
    return X @ V, np.abs(X) @ np.abs(V)


def xtr(X, R, square=False):
    """``X^T R`` (``(X o X)^T R`` with ``square``) and its absolute-value twin in fp64."""
    X, R = np.asarray(X, F64), np.asarray(R, F64)
    if square:
        X = X * X
    return X.T @ R, np.abs(X).T @ np.abs(R)


SPMM_C = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300)
ROW_NNZ = (0, 1, 7, 8, 9, 63, 64, 65, 130)        # rows 0..8 of the segs70 design
SEG_SMALL = 70
# sparse column -> non-zero count of the special columns of the segs70 design (segments at SEG_SMALL = 70):
# 0 (no segment), 1, 70 (one full segment), 71 (2 segments, the last of 1 pair), 140 (2 full segments),
# 281 (5 segments, the last of 1 pair)
SPECIAL_COL_NNZ = (0, 1, 70, 71, 140, 281)


def _fill(rng, shape, integer):
    if integer:
        return rng.choice(np.array([-2, -1, 1, 2], np.float32), shape)
    v = rng.standard_normal(shape).astype(np.float32) * 1.5
    v[v == 0] = 1.0
    return v


def design(name, integer):
    """The dense fp32 design matrices of the sparse-product cases, by the path they force."""
    rng = np.random.default_rng(sum(map(ord, name)) * 2 + int(integer))
    if name == "segs70":
        # N = 1200; columns: 3 dense, then 134 plain sparse columns, then the 6 special columns. Rows 0..8 hold exactly
        # ROW_NNZ sparse non-zeros (in the plain columns); the other rows ~2 % of the plain columns.
        N, nd, npl = 1200, 3, 134
        X = np.zeros((N, nd + npl + len(SPECIAL_COL_NNZ)), np.float32)
        X[:, :nd] = _fill(rng, (N, nd), integer)
        for r, k in enumerate(ROW_NNZ):
            cols = np.arange(k) if k >= 130 else np.sort(rng.choice(npl, k, replace=False))
            X[r, nd + cols] = _fill(rng, k, integer)
        rest = rng.random((N - len(ROW_NNZ), npl)) < 0.02
        X[len(ROW_NNZ):, nd:nd + npl][rest] = _fill(rng, int(rest.sum()), integer)
        for s, k in enumerate(SPECIAL_COL_NNZ):
            rows = len(ROW_NNZ) + np.sort(rng.choice(N - len(ROW_NNZ), k, replace=False))
            X[rows, nd + npl + s] = _fill(rng, k, integer)
        return X
    if name == "seg4096_two_segments":
        # the real segment length: N = 20000, one column at ~24 % density (below DENSE_FRAC): 2 segments of 4096 + rest
        N = 20000
        X = np.zeros((N, 8), np.float32)
        X[:, :2] = _fill(rng, (N, 2), integer)
        hit = rng.random(N) < 0.24
        X[hit, 2] = _fill(rng, int(hit.sum()), integer)
        for j in range(3, 8):
            hit = rng.random(N) < 0.01 * j
            X[hit, j] = _fill(rng, int(hit.sum()), integer)
        return X
    if name == "n1":                       # one row: its non-zero columns are dense, the zero columns sparse and empty
        X = np.zeros((1, 6), np.float32)
        X[0, [1, 4]] = _fill(rng, 2, integer)
        return X
    if name == "n5":                       # fewer rows than a workgroup's 4 waves + 1: single non-zeros stay sparse
        X = np.zeros((5, 9), np.float32)
        X[:, 0] = _fill(rng, 5, integer)
        for j in range(1, 8):
            X[(3 * j) % 5, j] = _fill(rng, 1, integer)[0]
        return X                           # column 8 all zero
    if name == "no_dense":
        N = 300
        X = np.zeros((N, 40), np.float32)
        hit = rng.random((N, 40)) < 0.05
        X[hit] = _fill(rng, int(hit.sum()), integer)
        X[:, 17] = 0                       # an all-zero sparse column between others
        X[7, :] = 0                        # an empty row
        return X
    if name == "no_sparse":
        return _fill(rng, (130, 5), integer)
    raise KeyError(name)


DESIGNS_SMALL = ("n1", "n5", "no_dense", "no_sparse")


def operands(X, C, integer, seed=0):
    """``V [d, C]`` and ``R [N, C]`` in fp32: {-1, 0, 1} or normal."""
    rng = np.random.default_rng(1000 + 7 * C + seed)
    N, d = X.shape
    if integer:
        return (rng.integers(-1, 2, (d, C)).astype(np.float32), rng.integers(-1, 2, (N, C)).astype(np.float32))
    return rng.standard_normal((d, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)


def mm_bound(S, V):
    """Reference and bound of ``SparseDesign.mm``: the dense block's fp32 GEMM (``nd`` products in any order), the CSR
    row's ``nnz_row`` fused or unfused multiply-adds in order, one addition of the two:
    ``|err| <= (nnz_row + 2) u (|Xs| |Vs|) + (nd + 2) u (|Xd| |Vd|)``."""
    V = np.asarray(V, np.float32)
    ref_s, abs_s = xv(S.Xs, V[S.idx_s])
    ref_d, abs_d = xv(S.Xd, V[S.idx_d])
    bound = (S.row_nnz[:, None] + 2) * U * abs_s + (len(S.idx_d) + 2) * U * abs_d
    return ref_s + ref_d, bound


def mm_sparse_part(S, V):
    """The CSR product alone, ``Xs Vs`` in fp64, and ``(nnz_row + 2) u (|Xs| |Vs|)``: what ``csr_spmm_kernel`` adds to the
    dense block's own fp32 GEMM, for the comparison that takes that GEMM as given."""
    V = np.asarray(V, np.float32)
    ref_s, abs_s = xv(S.Xs, V[S.idx_s])
    return ref_s, (S.row_nnz[:, None] + 2) * U * abs_s


def tmm_bound(S, R, square):
    """Reference ``[d, C]`` and bound of ``SparseDesign.tmm``: sparse column j: fp32 partials of at most
    ``min(cnt_j, seg)`` terms, added across segments in fp64; dense column: an fp32 GEMM over N terms. ``square`` rounds
    each squared value once more (one more u)."""
    R = np.asarray(R, np.float32)
    ref, ab = xtr(S.X, R, square)
    terms = np.empty(S.d, F64)
    terms[S.idx_s] = np.minimum(S.col_cnt, S.seg)
    terms[S.idx_d] = S.N
    return ref, (terms[:, None] + 2 + (1 if square else 0)) * U * ab


# ======================================================================================================== colsum
COLSUM_C = (1, 255, 256, 257, 700)
# (N, nblk): rows_per_blk = ceil(N / nblk); below, on and past nblk * rows_per_blk; nblk > N (empty blocks); one
# larger N so that a block's sum is a real accumulation
COLSUM_SHAPES = ((7, 4), (8, 4), (9, 4), (3, 8), (1, 1), (1000, 3))


def colsum_case(N, C):
    rng = np.random.default_rng(N * 1000 + C)
    return (rng.standard_normal((N, C)) * np.exp(rng.standard_normal((N, C)) * 3)).astype(np.float32)


def exact_colsum(A):
    A = np.asarray(A, F64)
    return np.array([math.fsum(A[:, j]) for j in range(A.shape[1])]), np.abs(A).sum(0)


# ======================================================================================================= softmax
def softmax_loss_residual(m, y, w):
    """fp64. ``m [N, P, K]`` margins with bias, ``y [N]``, ``w [N, P]``: loss ``w (lse - m_y)``, ``R = w (softmax -
    onehot(y))``, ``lse``; a label outside [0, K): loss 0, no one-hot term."""
    m = np.asarray(m, F64)
    N, P, K = m.shape
    mx = m.max(2, keepdims=True)
    e = np.exp(m - mx)
    se = e.sum(2, keepdims=True)
    lse = (mx + np.log(se))[:, :, 0]
    p = e / se
    yi = np.asarray(y).astype(np.int64)
    ok = (yi >= 0) & (yi < K)
    my = np.where(ok[:, None], np.take_along_axis(m, np.clip(yi, 0, K - 1)[:, None, None].repeat(P, 1), 2)[:, :, 0], lse)
    oh = np.zeros((N, 1, K))
    oh[np.flatnonzero(ok), 0, yi[ok]] = 1.0
    w = np.asarray(w, F64)
    return w * (lse - my), w[:, :, None] * (p - oh), lse


def softmax_f32(m32):
    """The kernels' formula in numpy float32 on fp32 margins (bias already added, once rounded, as the kernels do):
    ``p = exp(m - max) * (1 / sum)``, ``lse = max + log(sum)``, terms added in class order."""
    m32 = np.asarray(m32, F32)
    mx = m32.max(2, keepdims=True)
    e = np.exp((m32 - mx).astype(F32)).astype(F32)
    se = np.zeros(m32.shape[:2] + (1,), F32)
    for k in range(m32.shape[2]):
        se = (se + e[:, :, k:k + 1]).astype(F32)
    inv = (F32(1) / se).astype(F32)
    return (e * inv).astype(F32), (mx + np.log(se).astype(F32)).astype(F32)[:, :, 0]


def softmax_e32(m32, y):
    """``(e32 of the probabilities, e32 of the unit-weight loss / max(1, |lse|))`` of a case: float32 against fp64
    evaluation on the same fp32 margins."""
    m32 = np.asarray(m32, F32)
    N, P, K = m32.shape
    p32, lse32 = softmax_f32(m32)
    loss64, R64, lse64 = softmax_loss_residual(m32, y, np.ones((N, P)))
    yi = np.asarray(y).astype(np.int64)
    ok = (yi >= 0) & (yi < K)
    my32 = np.take_along_axis(m32, np.clip(yi, 0, K - 1)[:, None, None].repeat(P, 1), 2)[:, :, 0]
    loss32 = np.where(ok[:, None], (lse32 - my32).astype(F32), F32(0))
    oh = np.zeros((N, 1, K))
    oh[np.flatnonzero(ok), 0, yi[ok]] = 1.0
    ep = float(np.abs(p32.astype(F64) - (R64 + oh)).max())
    el = float((np.abs(loss32.astype(F64) - loss64) / np.maximum(1.0, np.abs(lse64))).max())
    return ep, el


SOFTMAX_PK = ((1, 1), (1, 2), (3, 3), (7, 16), (40, 6), (5, 20))
SOFTMAX_PK_IDS = ("P1-K1_single_class", "P1-K2_two_classes", "P3-K3", "P7-K16", "P40-K6_240_columns", "P5-K20_K_above_16")
SOFTMAX_N = (1, 255, 257)
SOFTMAX_MARGINS = ("ordinary", "saturated")
GRID_STRIDE_TOTAL = 65536 * 256 + 777          # one element more than a full grid of 65536 blocks covers in one step
GRID_PERIOD = 4099                              # the grid-stride cases tile a pattern of this (prime) length


def _weights(rng, shape):
    """Row weights: zeros, ones and non-integers."""
    w = rng.random(shape).astype(np.float32) * 2.5
    pick = rng.random(shape)
    w[pick < 0.2] = 0.0
    w[pick > 0.85] = 1.0
    return w


def _labels(rng, N, K, out_of_range=True):
    y = rng.integers(0, K, N).astype(np.float32)
    if out_of_range:
        y[3::11] = -1.0
        y[5::13] = float(K)
    return y


def softmax_case(P, K, N, margins, out_of_range=True):
    """``M [N, P*K]`` (no bias), ``bias [P*K]``, ``y [N]``, ``W [N, P]`` in fp32. ``ordinary``: margins of sigma ~2, bias
    ~1. ``saturated``: rows in turn hold one class ahead of equal others by 120, all classes equal (at 0, 50 and -3e4),
    and margins of +-1e4 under a bias of the opposite sign (sum of sigma ~2)."""
    rng = np.random.default_rng(P * 100003 + K * 1009 + N * 7 + len(margins))
    C = P * K
    bias = rng.standard_normal(C).astype(np.float32)
    M = (rng.standard_normal((N, C)) * 2).astype(np.float32)
    if margins == "saturated":
        big = np.where(np.arange(C) % 2 == 0, 1e4, -1e4).astype(np.float32)
        bias = (-big).astype(np.float32)
        M = (M + big[None, :]).astype(np.float32)         # M + bias is the sigma ~2 draw again (rounded to M's grid)
        for r in range(N):
            kind = r % 4
            if kind == 0:                                  # one class ahead by 120
                row = np.zeros((P, K), np.float32)
                row[np.arange(P), rng.integers(0, K, P)] = 120.0
                M[r] = row.reshape(-1) - bias
            elif kind == 1:                                # all classes equal
                M[r] = np.float32((0.0, 50.0, -3e4)[(r // 4) % 3]) - bias
    elif margins != "ordinary":
        raise KeyError(margins)
    return M, bias, _labels(rng, N, K, out_of_range), _weights(rng, (N, P))


def margins_f32(M, bias, P, K):
    """``M + bias`` rounded once to fp32, as the kernels form it, ``[N, P, K]``."""
    return (np.asarray(M, F32) + np.asarray(bias, F32)[None, :]).astype(F32).reshape(len(M), P, K)


# =========================================================================================================== mnl
MNL_P = (1, 32, 100, 256)
MNL_K = (1, 2, 16)
MNL_N = (1, 3, 257)


def empty_tail_blocks(N):
    """The smallest block count whose last block gets no rows: ``(nblk - 1) * ceil(N / nblk) >= N``."""
    nblk = 2
    while (nblk - 1) * (-(-N // nblk)) < N:
        nblk += 1
    return nblk


def mnl_case(P, K, N):
    """``M2 [N, 2C]`` (products with V_hi, then the much smaller ones with V_lo), ``bias [C]``, ``y``, ``W [N, ldw]``
    with ``ldw`` two more than the weight columns used, and the many-to-one ``wmap [P]`` (None: identity)."""
    rng = np.random.default_rng(P * 7919 + K * 131 + N)
    C = P * K
    Mh = (rng.standard_normal((N, C)) * 2).astype(np.float32)
    Ml = (rng.standard_normal((N, C)) * 2e-3).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    y = _labels(rng, N, K)
    nw = max(1, (P + 2) // 3)
    wmap = (np.arange(P) % nw).astype(np.int32)[::-1].copy()
    W_id = _weights(rng, (N, P + 2))
    W_map = _weights(rng, (N, nw + 2))
    return np.concatenate([Mh, Ml], 1), bias, y, (W_id, None), (W_map, wmap)


def mnl_margins_f32(M2, bias, P, K):
    """``(M_hi + M_lo) + bias`` in fp32, the kernel's order."""
    C = P * K
    M2 = np.asarray(M2, F32)
    return ((M2[:, :C] + M2[:, C:]).astype(F32) + np.asarray(bias, F32)[None, :]).astype(F32).reshape(len(M2), P, K)


# (id, K, pc, N, dpad, nblk, ldx - dpad); nblk = ceil(tiles / 8) unless the id says otherwise
MNL_BF16_CASES = (
    ("K2-N1-pc1-dpad64", 2, 1, 1, 64, 1, 0),
    ("K2-N31-pc31-dpad128", 2, 31, 31, 128, 1, 0),
    ("K2-N32-pc32-dpad192", 2, 32, 32, 192, 1, 0),
    ("K2-N33-pc1-dpad128", 2, 1, 33, 128, 1, 0),
    ("K2-N300-pc31-dpad192", 2, 31, 300, 192, 2, 0),
    ("K3-N1-pc32-dpad64", 3, 32, 1, 64, 1, 0),
    ("K3-N31-pc1-dpad192", 3, 1, 31, 192, 1, 0),
    ("K3-N32-pc31-dpad64", 3, 31, 32, 64, 1, 0),
    ("K3-N33-pc32-dpad128", 3, 32, 33, 128, 1, 0),
    ("K3-N300-pc1-dpad64", 3, 1, 300, 64, 2, 0),
    ("K6-N1-pc31-dpad128", 6, 31, 1, 128, 1, 0),
    ("K6-N31-pc32-dpad192", 6, 32, 31, 192, 1, 0),
    ("K6-N32-pc1-dpad128", 6, 1, 32, 128, 1, 0),
    ("K6-N33-pc31-dpad192", 6, 31, 33, 192, 1, 0),
    ("K6-N300-pc32-dpad64", 6, 32, 300, 64, 2, 0),
    ("K2-N600-nblk1-three_rounds_dead_waves", 2, 32, 600, 128, 1, 0),
    ("K3-N40-nblk4-waves_without_tile", 3, 31, 40, 64, 4, 0),
    ("K6-N33-ldx_gt_dpad", 6, 1, 33, 192, 1, 16),
    ("K2-N300-dpad64-single_chunk_ldx_gt_dpad", 2, 31, 300, 64, 2, 8),
)


def mnl_bf16_case(K, pc, N, dpad, integer):
    """Inputs of the fused kernel: ``X [npad, dpad]`` bf16-exact fp32 (rows past N zero), ``Vhi``, ``Vlo`` ``[K*32,
    dpad]`` bf16-exact (class-major rows ``k * 32 + p``; the padding problems p >= pc keep non-zero coefficients: their
    weight, not their margin, must silence them), ``bias [K*32]``, ``y``, ``W [N, ldw]``, ``wcol [32]``."""
    rng = np.random.default_rng(K * 1000003 + pc * 10007 + N * 13 + dpad + int(integer))
    npad = -(-N // 32) * 32
    X = np.zeros((npad, dpad), np.float32)
    if integer:
        X[:N] = rng.integers(-2, 3, (N, dpad)).astype(np.float32)
        Vhi = (rng.integers(-1, 2, (K * 32, dpad)) * (rng.random((K * 32, dpad)) < 0.2)).astype(np.float32)
        Vlo = np.zeros_like(Vhi)
        bias = rng.integers(-2, 3, K * 32).astype(np.float32)
    else:
        X[:N] = bf16_round(rng.standard_normal((N, dpad)).astype(np.float32))
        V = (rng.standard_normal((K * 32, dpad)) * (1.5 / math.sqrt(dpad))).astype(np.float32)
        Vhi, Vlo = bf16_split(V)
        bias = rng.standard_normal(K * 32).astype(np.float32)
    y = _labels(rng, N, K)
    nw = max(1, (pc + 1) // 2)
    W = _weights(rng, (N, nw + 3))
    wcol = np.zeros(32, np.int32)
    wcol[:pc] = (np.arange(pc) * 5) % nw
    wcol[pc:] = wcol[0]
    return X, Vhi, Vlo, bias, y, W, wcol


def mnl_bf16_reference(X, Vhi, Vlo, bias, N, K):
    """fp64 margins ``[N, 32, K]`` of the bf16 X against ``V_hi + V_lo`` exactly as passed, and ``sum |x| |v|``."""
    X = np.asarray(X, F64)[:N]
    m = X @ (np.asarray(Vhi, F64) + np.asarray(Vlo, F64)).T + np.asarray(bias, F64)[None, :]       # [N, K*32]
    a = np.abs(X) @ (np.abs(np.asarray(Vhi, F64)) + np.abs(np.asarray(Vlo, F64))).T + np.abs(np.asarray(bias, F64))
    return m.reshape(N, K, 32).transpose(0, 2, 1), a.reshape(N, K, 32).transpose(0, 2, 1)


# =========================================================================================================== mlp
MLP_P = (1, 3)
MLP_B = (1, 7, 256, 257, 600)
MLP_N = (1, 2047, 2048, 2049, 5000)
SIGMOID_Z = (-1e4, -100.0, -89.0, -87.0, -20.0, -0.0, 0.0, 20.0, 87.0, 89.0, 100.0, 1e4)     # ascending
MLP_GRID_PNB = (1, 172969, 97)                 # P * N * B = GRID_STRIDE_TOTAL = 97 * 172969


def sigmoid(z):
    """fp64 ``1 / (1 + e^-z)`` without overflow."""
    z = np.asarray(z, F64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_f32(z32):
    """The kernel's formula in numpy float32: ``1 / (1 + exp(-z))``."""
    z32 = np.asarray(z32, F32)
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-z32).astype(F32)).astype(F32)).astype(F32)


def sigmoid_case(P, N, B):
    """``Z [P, N, B]``, ``bias [P, B]`` fp32: sigma ~3 pre-activations, bias ~1."""
    rng = np.random.default_rng(P * 1000003 + N * 1009 + B)
    return (rng.standard_normal((P, N, B)) * 3).astype(np.float32), rng.standard_normal((P, B)).astype(np.float32)


def bias_sigmoid(Z, b):
    """``(fp64 sigmoid(z), e32)`` with ``z = Z + b`` rounded once to fp32, as the kernel forms it."""
    z32 = (np.asarray(Z, F32) + np.asarray(b, F32)[:, None, :]).astype(F32)
    ref = sigmoid(z32)
    return ref, float(np.abs(sigmoid_f32(z32).astype(F64) - ref).max())


def backprop_case(P, N, B):
    """``D [P, N, B]`` normal, ``A [P, N, B]`` activations in [0, 1], exact 0 and 1 among them."""
    rng = np.random.default_rng(P * 7 + N * 100003 + B * 11)
    D = rng.standard_normal((P, N, B)).astype(np.float32)
    A = sigmoid(rng.standard_normal((P, N, B)) * 3).astype(np.float32)
    pick = rng.random((P, N, B))
    A[pick < 0.02] = 0.0
    A[pick > 0.98] = 1.0
    return D, A


def sigmoid_backprop(D, A):
    """fp64 ``d a (1 - a)`` and its column sums ``[P, B]``."""
    D, A = np.asarray(D, F64), np.asarray(A, F64)
    out = D * (A * (1.0 - A))
    return out, out.sum(1)


def mlp_nblks(N):
    """Block counts of the back-propagation cases: 1, 3 and one that leaves the last blocks without rows."""
    return (1, 3, empty_tail_blocks(N))
