"""Plain oracle of the column-statistics and Gramian kernels (``ops/csrc/hip/stats_kernels.hip``): numpy and the standard
library only, nothing of the project, no torch. One straightforward function per kernel, written from the operation's
definition, and the *case tables* (shapes and data builders) that tests/test_stats_kernels_gpu.py runs on the device and
tests/test_stats_oracle.py runs on the host paths of ``ops/stats.py``, so that both sides are judged on the same inputs.

Precision. Sums whose terms are small integers or dyadic fractions are added as int64 after scaling by a power of two:
exact and order-free, so a kernel that adds the same terms in fp64 (or in fp32 while every partial sum fits 24 bits) must
give the same bits whatever its order. Real-valued sums are added as ``fractions.Fraction`` (or ``math.fsum`` where every
term is an fp64 value) and rounded once. The column mean and M2 are exact rationals of exact integer sums.

bf16. ``bf16_bits`` rounds the fp32 bit pattern to nearest even at bit 16. ``split3`` is the three-part split of the
packing kernel: ``h = bf16(c)``, ``mid = bf16(c - h)``, ``lo = bf16((c - h) - mid)`` in fp32. The parts sum to ``c``
exactly while ``lo`` is not lost to underflow (``c`` zero or ``|c| >= 2^-100``). A magnitude above the largest finite
bf16 value (about 3.39e38) rounds ``h`` to infinity and the split yields NaN: that input is out of scope here and no
case holds one.

Exactness of the bf16 Gramian cases. ``gram_bf16_kernel`` adds exact products in fp32 over 256-row slices, one
accumulator per pair of packed columns. A block stays exact when all its products are multiples of one unit ``u`` and
256 of them stay under ``2^24 u``. The dyadic columns ``a + b 2^-10`` (``a`` in [-2, 2], ``b`` in [-3, 3]) are therefore
centred on ``mean = +-4``: then ``h = a - mean`` is an integer of magnitude 2 to 6 (``|a - mean| = 1`` would not do:
``1 - 3 2^-10`` lies in the binade below 1, where bf16 rounds it to ``1 - 2^-8``),
``mid = b 2^-10`` and ``lo = 0`` on every row, and the blocks have units 1, 2^-10 and 2^-20 with sums under 2^14, 2^13
and 2^12 units. (Centred on 0, the rows with ``a = 0`` would put ``h = b 2^-10`` into the block of the integers, whose
partial sums near 2^10 cannot hold a 2^-20.) ``gram_lo_case`` adds a 2^-19 term under a ``+-3 2^-11`` middle part so that
``lo`` is non-zero; its units are worked out in its docstring."""
import math
from fractions import Fraction

import numpy as np

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64


def f32_from_bits(words):
    return np.asarray(words, np.uint32).view(F32)


def frac(a):
    """The values of a float array as exact rationals."""
    return [Fraction(float(v)) for v in np.asarray(a).ravel()]


# ========================================================================================================== bf16
def bf16_bits(x):
    """uint16 bf16 pattern of fp32 values: round to nearest, ties to even, on the bit pattern (no NaN handling)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(x):
    """fp32 values rounded to bf16, as fp32."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(F32)


def split3(c):
    """(h, mid, lo) of fp32 ``c``: each part a bf16 value held in fp32; every operation is one fp32 operation."""
    c = np.ascontiguousarray(c, F32)
    h = bf16_round(c)
    mid = bf16_round(c - h)
    lo = bf16_round((c - h) - mid)
    return h, mid, lo


ZERO, ONE, RAW, HI, MID, LO, LABEL = range(7)        # column modes of bf16_pack_kernel


def bf16_pack(X, y, src, mode, mu, sc, ldb, rows):
    """uint16 ``[rows, ldb]``: the bf16 pattern of output column j per its mode; columns past ``len(src)`` and rows
    past ``X``'s are zero."""
    n = X.shape[0]
    out = np.zeros((rows, ldb), np.uint16)
    for j in range(len(src)):
        m, s = int(mode[j]), int(src[j])
        if m == ZERO:
            continue
        if m == ONE:
            v = np.ones(n, F32)
        elif m == RAW:
            v = X[:, s]
        elif m in (HI, MID, LO):
            c = (np.ascontiguousarray(X[:, s], F32) - F32(mu[j])) * F32(sc[j])
            v = split3(c)[m - HI]
        else:
            v = (np.asarray(y) == s).astype(F32)
        out[:n, j] = bf16_bits(v)
    return out


def col_bf16_exact(X):
    """uint32 ``[d]``: OR over the rows of the low 16 bits of each column's fp32 patterns (0: exact in bf16)."""
    b = np.ascontiguousarray(X, F32).view(np.uint32)
    acc = np.zeros(X.shape[1], np.uint32)
    for r in range(X.shape[0]):
        acc |= b[r] & np.uint32(0xFFFF)
    return acc


# ===================================================================================================== col_stats
def _exact_ints(col):
    """(integers M, exponent e) with ``col[r] == M[r] * 2^e`` exactly, for an fp32 column."""
    m, e = np.frexp(np.asarray(col, F64))
    mant = (m * 2.0 ** 24).astype(I64)                      # 24-bit significands: exact
    ex = e.astype(I64) - 24
    live = mant != 0
    e0 = int(ex[live].min()) if live.any() else 0
    return [int(a) << (int(b) - e0) if a else 0 for a, b in zip(mant, ex)], e0


def col_stats(X):
    """dict of fp64 ``[d]`` arrays: mean, m2 (sum of squared deviations from the exact mean), min, max, nnz, and the
    row count; mean and m2 are exact rationals rounded once."""
    n, d = X.shape
    out = {k: np.zeros(d, F64) for k in ("mean", "m2", "min", "max", "nnz")}
    out["count"] = n
    for j in range(d):
        ints, e0 = _exact_ints(X[:, j])
        S, Q = sum(ints), sum(v * v for v in ints)
        scale = Fraction(2) ** e0
        out["mean"][j] = float(Fraction(S, n) * scale)
        out["m2"][j] = float((Q - Fraction(S * S, n)) * scale * scale)
        out["min"][j] = min(float(v) for v in X[:, j])
        out["max"][j] = max(float(v) for v in X[:, j])
        out["nnz"][j] = sum(1 for v in X[:, j] if v != 0)     # -0.0 is not a non-zero
    return out


def col_stats_launch(n, d):
    """(chunks launched, rows per chunk, chunks that hold no row) of the col_stats entry: ~2048 workgroups, at most
    n / 256 + 1 chunks, not recounted after the rows per chunk are rounded up."""
    cblocks = (d + 63) // 64
    chunks = max(1, min((2048 + cblocks - 1) // cblocks, n // 256 + 1))
    rpc = (n + chunks - 1) // chunks
    return chunks, rpc, sum(1 for k in range(chunks) if k * rpc >= n)


COL_KINDS = ("offset1e6", "offset1e4", "constant", "zero", "negative", "negzero", "indicator", "normal")


def col_stats_data(n, d, seed=0):
    """fp32 ``[n, d]``: column j is of kind ``COL_KINDS[j % 8]``."""
    rng = np.random.default_rng(1000 * seed + 7 * n + d)
    X = np.zeros((n, d), F32)
    for j in range(d):
        k = COL_KINDS[j % len(COL_KINDS)]
        if k == "offset1e6":
            X[:, j] = (1e6 + 1e-3 * rng.standard_normal(n)).astype(F32)
        elif k == "offset1e4":                                       # a spread that fp32 resolves
            X[:, j] = (1e4 + 1e-2 * rng.standard_normal(n)).astype(F32)
        elif k == "constant":
            X[:, j] = 5.0
        elif k == "negative":
            X[:, j] = (-1.0 - rng.random(n)).astype(F32)
        elif k == "negzero":
            X[:, j] = rng.integers(0, 2, n).astype(F32) * 0.5
            X[::3, j] = -0.0
        elif k == "indicator":
            X[:, j] = (rng.random(n) < 0.3).astype(F32)
        elif k == "normal":
            X[:, j] = (0.5 + rng.standard_normal(n)).astype(F32)
    return X


# (name, n, d, extra row stride)
COL_STATS_CASES = (
    [(f"rows_{n}", n, 8, 0) for n in (1, 3, 255, 256, 257)]
    + [("rows_2305_ten_chunks_cross_fold_unroll", 2305, 8, 0)]
    + [(f"cols_{d}", 257, d, 0) for d in (1, 63, 64, 65, 130)]
    + [("empty_trailing_chunk", 76800, 3, 0), ("row_strided", 300, 65, 5)])


# ================================================================================================== class_colsum
def class_colsum(X, codes, L):
    """(sums, abs) fp64 ``[P, L, d]``: the exactly rounded sum, and sum of magnitudes, of ``X[r, j]`` over the rows with
    ``codes[p, r] == c``; codes outside [0, L) count nowhere."""
    P, n = codes.shape
    d = X.shape[1]
    out, mag = np.zeros((P, L, d), F64), np.zeros((P, L, d), F64)
    X64 = np.asarray(X, F64)
    for p in range(P):
        for c in range(L):
            rows = X64[codes[p] == c]
            for j in range(d):
                out[p, c, j] = math.fsum(rows[:, j])
                mag[p, c, j] = math.fsum(np.abs(rows[:, j]))
    return out, mag


def ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, shape).astype(F32)


def class_colsum_data(n, d, P, L, real=False):
    rng = np.random.default_rng(11 * n + 3 * d + 101 * P + L)
    X = rng.standard_normal((n, d)).astype(F32) if real else ints(rng, (n, d))
    codes = rng.integers(-1, L, (P, n)).astype(I32)
    if P > 1:
        codes[P - 1] = -1                                # a whole problem without rows
    return X, codes


CLASS_PL = ((1, 1), (1, 2), (3, 4), (8, 8), (64, 1), (1, 64))
# (name, n, d, P, L, real)
CLASS_COLSUM_CASES = (
    [(f"n{n}_d{d}", n, d, 3, 4, False) for n in (1, 3, 257, 1000) for d in (1, 64, 65)]
    + [(f"P{P}_L{L}", 257, 65, P, L, False) for P, L in CLASS_PL if (P, L) != (3, 4)]
    + [("real_valued", 257, 65, 3, 4, True)])


# ============================================================================================== weighted_colsums
def weighted_colsums_exact(X, W):
    """fp64 ``[P, 2, d]`` for integer ``X`` and weights that are multiples of 1/8: int64 sums, exact."""
    Xi = np.asarray(X, F64).astype(I64)
    Wi = (np.asarray(W, F64) * 8).astype(I64)
    assert (Xi == X).all() and (Wi == np.asarray(W, F64) * 8).all()
    s1 = Wi.T @ Xi
    s2 = Wi.T @ (Xi * Xi)
    return np.stack([s1, s2], 1).astype(F64) / 8.0


def weighted_colsums_real(X, W):
    """(sums, abs) fp64 ``[P, 2, d]`` for real data: rational sums rounded once, and the sums of the magnitudes."""
    n, d = X.shape
    P = W.shape[1]
    out, mag = np.zeros((P, 2, d), F64), np.zeros((P, 2, d), F64)
    xs = [frac(X[:, j]) for j in range(d)]
    for p in range(P):
        w = frac(W[:, p])
        for j in range(d):
            t1 = [a * b for a, b in zip(w, xs[j])]
            t2 = [a * b * b for a, b in zip(w, xs[j])]
            out[p, 0, j], out[p, 1, j] = float(sum(t1)), float(sum(t2))
            mag[p, 0, j], mag[p, 1, j] = float(sum(map(abs, t1))), float(sum(map(abs, t2)))
    return out, mag


def eighths(rng, shape, top=16):
    """Weights in {0, 1/8, ..., top/8}, about a fifth of them zero."""
    w = rng.integers(0, top + 1, shape).astype(F64) / 8.0
    w[rng.random(shape) < 0.2] = 0.0
    return w


def weighted_colsums_data(n, d, P):
    rng = np.random.default_rng(13 * n + 5 * d + P)
    return ints(rng, (n, d)), eighths(rng, (n, P)).astype(F32)


# (name, n, d, P)
WEIGHTED_COLSUMS_CASES = (
    [(f"rows_{n}", n, 65, 17) for n in (1, 3, 4095, 4096, 4097, 8193)]
    + [(f"cols_{d}", 4097, d, 1) for d in (1, 64)]
    + [(f"problems_{P}", 3, 64, P) for P in (16, 33)])


# ========================================================================================================= wgram
def _design(X, Y, k):
    """fp64 ``A_k = [X | 1 | y_k]`` (y_k: column k of a 2-d ``Y``, or a shared 1-d ``Y``, or absent)."""
    cols = [np.asarray(X, F64), np.ones((X.shape[0], 1), F64)]
    if Y is not None:
        cols.append(np.asarray(Y[:, k] if Y.ndim == 2 else Y, F64)[:, None])
    return np.concatenate(cols, 1)


def wgram_exact(X, W, Y):
    """fp64 ``[K, D, D]`` for data that are multiples of 2^-10 and weights that are multiples of 1/8: int64, exact."""
    K = W.shape[1]
    out = []
    for k in range(K):
        A = _design(X, Y, k) * 1024.0
        Ai, wi = A.astype(I64), (np.asarray(W[:, k], F64) * 8).astype(I64)
        assert (Ai == A).all() and (wi == W[:, k] * 8).all()
        out.append(((Ai * wi[:, None]).T @ Ai).astype(F64) / 2.0 ** 23)
    return np.stack(out)


def wgram_real(X, W, Y):
    """(G, abs) fp64 ``[K, D, D]`` for real data: rational sums rounded once, and the sums of the magnitudes."""
    K = W.shape[1]
    G, T = [], []
    for k in range(K):
        A = _design(X, Y, k)
        D = A.shape[1]
        cols, w = [frac(A[:, i]) for i in range(D)], frac(W[:, k])
        g, t = np.zeros((D, D), F64), np.zeros((D, D), F64)
        for i in range(D):
            wa = [a * b for a, b in zip(w, cols[i])]
            for j in range(i, D):
                terms = [a * b for a, b in zip(wa, cols[j])]
                g[i, j] = g[j, i] = float(sum(terms))
                t[i, j] = t[j, i] = float(sum(map(abs, terms)))
        G.append(g)
        T.append(t)
    return np.stack(G), np.stack(T)


def dyadic(rng, shape):
    """``a + b 2^-10`` with a in [-2, 2] and b in [-3, 3]."""
    return (rng.integers(-2, 3, shape) + rng.integers(-3, 4, shape) / 1024.0).astype(F32)


def wgram_data(n, d, K, ymode, real=False):
    """X fp32 [n, d], W fp64 [n, K], Y fp64 None / [n] / [n, K]."""
    rng = np.random.default_rng(17 * n + 7 * d + 3 * K + len(ymode))
    yshape = {"none": None, "shared": (n,), "per_weight": (n, K)}[ymode]
    if real:
        X, W = rng.standard_normal((n, d)).astype(F32), rng.random((n, K))
        Y = None if yshape is None else rng.standard_normal(yshape)
    else:
        X, W = dyadic(rng, (n, d)), eighths(rng, (n, K))
        Y = None if yshape is None else dyadic(rng, yshape).astype(F64)
    return X, W, Y


# (name, n, d, K, ymode); D = d + 1 (+ 1 with a response)
WGRAM_CASES = (
    [(f"rows_{n}", n, 5, 5, "per_weight") for n in (1, 15, 16, 17, 257, 600)]
    + [("D2", 17, 1, 1, "none"), ("D63", 17, 62, 1, "none"), ("D64_shared", 17, 62, 4, "shared"),
       ("D65_ones_alone_in_last_tile", 17, 64, 5, "none"), ("D65_response_alone_in_last_tile", 17, 63, 5, "per_weight"),
       ("D66", 17, 64, 4, "per_weight"), ("D129_shared", 17, 127, 1, "shared"), ("D129_K9", 17, 128, 9, "none")])
WGRAM_REAL_CASE = ("real_valued", 257, 5, 5, "per_weight")


# ====================================================================================================== Gramians
def gram_int(A, unit):
    """fp64 ``A^T A`` of a matrix whose entries are multiples of ``unit`` (a power of two): int64, exact."""
    S = np.asarray(A, F64) / unit
    Ai = S.astype(I64)
    assert (Ai == S).all()
    return (Ai.T @ Ai).astype(F64) * (unit * unit)


def onehot(y, L):
    """fp64 ``[n, L]``; a code outside [0, L) counts in no column."""
    return (np.asarray(y)[:, None] == np.arange(L)[None, :]).astype(F64)


def gram_aug(X, mu, y, L):
    """The augmented matrix ``[fp32(X - mu) | onehot(y)]`` in fp64: the centring is the kernel's one fp32 subtraction."""
    C = (np.ascontiguousarray(X, F32) - np.asarray(mu, F32)[None, :]).astype(F64)
    return np.concatenate([C, onehot(y, L)], 1) if L else C


def gram_centered(X, mean, y, L):
    """The augmented matrix ``[X - mean | onehot(y)]`` in fp64 (exact for the dyadic cases)."""
    C = np.asarray(X, F64) - np.asarray(mean, F64)[None, :]
    return np.concatenate([C, onehot(y, L)], 1) if L else C


GRAM_ROWS = (1, 31, 32, 33, 255, 256, 257, 1025)
# (name, n, d, L): D = d + L
GRAM_AUG_CASES = (
    [(f"rows_{n}", n, 5, 3) for n in GRAM_ROWS]
    + [("D1", 33, 1, 0), ("D127", 33, 124, 3), ("D128_label_last_in_tile", 33, 127, 1),
       ("D129_labels_straddle_tile", 33, 126, 3), ("D129_no_labels", 33, 129, 0), ("D257_three_tiles", 33, 254, 3),
       ("D257_two_chunks", 1025, 254, 3)])


def gram_aug_data(n, d, L, real=False):
    """X fp32 [n, d] (quarters in [-3, 3]), integer centres in [-2, 2], codes in [-1, L] (both ends count nowhere).
    |x - mu| <= 5 in quarters: products are multiples of 1/16 and 256 of them stay under 2^24 / 16."""
    rng = np.random.default_rng(19 * n + 7 * d + L)
    if real:
        X, mu = rng.standard_normal((n, d)).astype(F32), (0.1 * rng.standard_normal(d)).astype(F32)
    else:
        X, mu = (rng.integers(-12, 13, (n, d)) / 4.0).astype(F32), rng.integers(-2, 3, d).astype(F32)
    y = rng.integers(-1, L + 2, n).astype(I32)
    return X, mu, y


GRAM_BF16_CASES = (
    [(f"rows_{n}", n, 5, pad) for n in GRAM_ROWS for pad in (0, 8)]
    + [(f"D{D}", 33, D, pad) for D, pad in ((1, 8), (127, 0), (128, 8), (129, 0), (257, 8))]
    + [("D257_two_chunks", 1025, 257, 0)])


def gram_bf16_data(n, D, pad):
    """Small integers (exact in bf16) [n, lda] with lda = tiles * 128 + pad; columns from D on are zero."""
    rng = np.random.default_rng(23 * n + D + pad)
    lda = (D + 127) // 128 * 128 + pad
    A = np.zeros((n, lda), F32)
    A[:, :D] = ints(rng, (n, D))
    return A


def _mix(d, kind):
    """Which columns of a gram_centered case are exact in bf16."""
    return {"all_exact": [True] * d, "none_exact": [False] * d, "interleaved": [j % 2 == 0 for j in range(d)]}[kind]


# (name, n, d, column mix, L)
GRAM_CENTERED_CASES = [(f"{kind}_d{d}_L{L}", 300, d, kind, L)
                       for kind, d in (("all_exact", 6), ("none_exact", 5), ("interleaved", 9), ("all_exact", 1),
                                       ("none_exact", 1))
                       for L in (0, 3)]


def gram_centered_data(n, d, kind, L):
    """X fp32 [n, d]: exact columns are integers in [-3, 3] centred on an integer in [-2, 2]; the others are
    ``a + b 2^-10`` centred on +-4 (the module docstring says why). Codes in [0, L)."""
    rng = np.random.default_rng(29 * n + 11 * d + L + len(kind))
    X, mean = np.zeros((n, d), F32), np.zeros(d, F64)
    for j, ex in enumerate(_mix(d, kind)):
        if ex:
            X[:, j], mean[j] = ints(rng, n), rng.integers(-2, 3)
        else:
            X[:, j], mean[j] = dyadic(rng, n), 4 * (1 if j % 4 < 2 else -1)
            X[0, j] = 1.0 + 3.0 / 1024.0                          # whatever the draw, the column is not exact
    y = rng.integers(0, max(L, 1), n).astype(I32)
    return X, mean, y


def gram_lo_case(n=300, d=4, L=3):
    """Columns ``a + 3 s 2^-11 + e 2^-19`` (a in [-2, 2], s = +-1, e in [-3, 3]) centred on -4, so all three parts are
    non-zero: h = a + 4 in [2, 6] (unit 1), mid = bf16(3 s 2^-11 + e 2^-19) of magnitude at most 1.51 * 2^-10 within
    one binade (unit 2^-17, the bf16 spacing there), lo the rest, of magnitude at most 2^-18 (unit 2^-19). Largest
    256-row block sums in units: h h 36 * 256 < 2^14; h mid 6 * 1.51 * 2^7 * 256 < 2^19; h lo 6 * 2 * 256 < 2^12;
    mid mid (1.51 * 2^7)^2 * 256 < 2^23.2; mid lo 1.51 * 2^7 * 2 * 256 < 2^17; lo lo 4 * 256 = 2^10: all under 2^24, so
    the fp32 sums are exact. Column 0 is an integer (bf16-exact) column centred on 1."""
    rng = np.random.default_rng(31)
    X = (rng.integers(-2, 3, (n, d)) + rng.choice([-3.0, 3.0], (n, d)) / 2.0 ** 11
         + rng.integers(-3, 4, (n, d)) / 2.0 ** 19).astype(F32)
    mean = np.full(d, -4.0)
    X[:, 0], mean[0] = ints(rng, n), 1.0
    return X, mean, rng.integers(0, L, n).astype(I32), L


def gram_real_case(n=300, d=7, L=3):
    """Real-valued columns (one of them an indicator, exact in bf16) and their fp64 mean, which fp32 does not hold."""
    rng = np.random.default_rng(37)
    X = rng.standard_normal((n, d)).astype(F32)
    X[:, 1] = (1e2 + rng.standard_normal(n)).astype(F32)
    X[:, 2] = (rng.random(n) < 0.3).astype(F32)
    mean = np.array([math.fsum(X[:, j]) / n for j in range(d)])
    return X, mean, rng.integers(0, L, n).astype(I32), L


# ===================================================================================================== bf16_pack
PACK_DX = 24                                          # columns of the packing source matrix
# 0, -0.0, an fp32 subnormal, 2^-120, 2^100, the next fp32 after a bf16 value, the one before the next bf16 value, the
# two ties (round down to even, round up to even), and their negatives
PACK_SPECIAL = np.concatenate([
    f32_from_bits([0x00000000, 0x80000000, 0x00012345, 0x80400000]),
    np.array([2.0 ** -120, -2.0 ** -120, 2.0 ** 100, -2.0 ** 100], F32),
    f32_from_bits([0x3F800001, 0x3F80FFFF, 0x3F808000, 0x3F818000, 0xBF800001, 0xBF80FFFF, 0xBF808000, 0xBF818000])])


def pack_source(n):
    """fp32 [n, 24]: random values with the special ones spread over rows and columns."""
    rng = np.random.default_rng(41 + n)
    X = (rng.standard_normal((n, PACK_DX)) * 4).astype(F32)
    for r in range(n):
        for c in range(PACK_DX):
            if (r * 5 + c) % 3 == 0:
                X[r, c] = PACK_SPECIAL[(r * 7 + c) % len(PACK_SPECIAL)]
    return X


_SC = (1.0, 0.25, 1.0 / 3.0)
_MU = (0.0, 1.0, -0.375, 0.1)


def _cols(src, mode):
    k = len(src)
    return (np.array(src, I32), np.array(mode, I32), np.array([_MU[j % 4] for j in range(k)], F32),
            np.array([_SC[j % 3] for j in range(k)], F32))


def _wide(k):
    """k output columns: sources walk the matrix three at a time, modes cycle through all seven."""
    src, mode = [], []
    for j in range(k):
        m = j % 7
        src.append(2 if m == LABEL else (j * 3) % PACK_DX)
        mode.append(m)
    return src, mode


# name -> (n, ldb, rows, src, mode, view): view is how X lies in memory, "aligned" (row stride 24, base on 16 bytes),
# "ld_odd" (row stride 27) or "base_off" (row stride 24, base 4 bytes past a 16-byte boundary)
PACK_CASES = {
    "fast_path_eight_aligned_sources": (17, 8, 17, list(range(8, 16)), [HI, MID, LO, RAW, HI, MID, LO, RAW], "aligned"),
    "consecutive_from_column_5": (17, 8, 17, list(range(5, 13)), [HI, MID, LO, RAW] * 2, "aligned"),
    "row_stride_not_multiple_of_4": (17, 8, 17, list(range(8, 16)), [HI, MID, LO, RAW] * 2, "ld_odd"),
    "base_4_bytes_off_16": (17, 8, 17, list(range(8, 16)), [HI, MID, LO, RAW] * 2, "base_off"),
    "labels_match_nothing": (17, 8, 17, [99, -7, 3, 4, 5, 6, 7, 8], [LABEL, LABEL, HI, MID, LO, RAW, ONE, ZERO],
                             "aligned"),
    "rows_past_n_are_zero": (15, 8, 24, [0, 0, 2, 3, 3, 3, 1, 9], [ZERO, ONE, RAW, HI, MID, LO, LABEL, HI], "aligned"),
    "ldb_512_full": (70, 512, 70) + _wide(512) + ("aligned",),
    "ldb_520_two_column_tiles": (70, 520, 70) + _wide(515) + ("aligned",),
    "ldb_520_fast_groups": (16, 520, 16, [j % 24 for j in range(504)], [HI + (j // 8) % 3 for j in range(504)],
                            "aligned"),
}
for _n in (1, 15, 16, 17, 70):
    PACK_CASES[f"all_seven_modes_rows_{_n}"] = (_n, 8, _n, [0, 0, 2, 3, 3, 3, 1, 9],
                                                [ZERO, ONE, RAW, HI, MID, LO, LABEL, HI], "aligned")


def pack_case(name):
    """(X, y, src, mode, mu, sc, ldb, rows, view) of a packing case; label codes in [-1, 3]."""
    n, ldb, rows, src, mode, view = PACK_CASES[name]
    y = np.random.default_rng(43 + n).integers(-1, 4, n).astype(I32)
    return (pack_source(n), y) + _cols(src, mode) + (ldb, rows, view)


# ================================================================================================ col_bf16_exact
# (name, n, d, extra row stride)
BF16_EXACT_CASES = (
    [(f"rows_{n}", n, 65, 0) for n in (0, 1, 3, 1023, 1024, 1025, 2049)]
    + [(f"cols_{d}", 1025, d, 0) for d in (1, 64)] + [("row_strided", 1025, 65, 3)])


def bf16_exact_data(n, d):
    """fp32 [n, d] of bf16-exact values (small integers, -0.0, inf, a subnormal with its low bits clear), with one
    inexact value in column j at: row 0 (j % 8 == 1), the last row (2), a middle row of residue 0..3 mod 4 (3..6);
    columns with j % 8 in (0, 7) stay exact. Returns (X, expected exactness) -- the expectation by construction."""
    rng = np.random.default_rng(47 * n + d)
    X = ints(rng, (n, d))
    exact = np.ones(d, bool)
    special = f32_from_bits([0x80000000, 0x7F800000, 0x00010000, 0xFF800000])
    for j in range(d):
        if n:
            X[(j * 13) % n, j] = special[j % 4]
        k = j % 8
        row = {1: 0, 2: n - 1}.get(k, n // 2 // 4 * 4 + (k - 3) if 3 <= k <= 6 else None)
        if row is not None and 0 <= row < n:
            X[row, j] = f32_from_bits([0x3F800001 if j % 2 else 0x40008000])[0]
            exact[j] = False
    return X, exact
