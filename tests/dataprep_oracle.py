"""Plain oracle of the data-preparation kernels (``ops/csrc/hip/vector_kernels.hip``, ``ops/csrc/hip/rff_kernels.hip``):
numpy and the standard library only, nothing of the project, no torch. One straightforward function per operation, written
from the operation's definition (row loops, exact rational sums), and the *case tables* that
tests/test_dataprep_kernels_gpu.py runs on the device and tests/test_dataprep_oracle.py runs on the host torch paths, so
that both sides are judged on the same inputs.

Bit patterns: fp32 results that are moved, not computed (``vectorize``, ``gather``), are compared as int32 views, so NaN
payloads, the sign of zero and denormals count. Sums: the oracle adds exactly (``fractions.Fraction``) and rounds once.
Histogram splits: ``mn + step * b`` in Python floats, i.e. a rounded multiply and a rounded add, as
``FeatureDistribution.histValues`` computes them; ``hist(..., fused=True)`` rounds ``mn + step * b`` once instead, which is
what a fused multiply-add does, and exists only to show that the histogram case table tells the two apart."""
import bisect
import functools
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)           # unit roundoff of fp64
F32, F64, I64, U8, BOOL = np.float32, np.float64, np.int64, np.uint8, np.bool_


def bits(a):
    """int32 view of an fp32 array: the comparison key of the moved-not-computed results."""
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _f32_from_bits(words):
    return np.asarray(words, np.uint32).view(np.float32)


# NaN with payloads (quiet, negative quiet, signalling), the infinities, the zeros, the smallest and the largest denormal
SPECIAL_F32 = _f32_from_bits([0x7FC00123, 0xFFC00001, 0x7FA00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                              0x00000001, 0x807FFFFF])
POISON_F32 = _f32_from_bits([0x7FC0DEAD, 0x7F800000, 0xFF800000, 0xFFC0BEEF])      # what null slots hold


def _values_f32(rng, n):
    """Random fp32 values, about a third of them drawn from SPECIAL_F32."""
    v = rng.standard_normal(n).astype(np.float32)
    pick = rng.random(n) < 0.35
    v[pick] = SPECIAL_F32[rng.integers(0, len(SPECIAL_F32), int(pick.sum()))]
    return v


# ===================================================================================================== vectorize
def vectorize(vals, valid, fills, track):
    """``out[r, per*c] = valid ? val : fill[c]``; ``out[r, per*c + 1] = !valid`` when tracking nulls. fp32 [n, F*per]."""
    n, F, per = len(vals[0]), len(vals), 2 if track else 1
    out = np.zeros((n, F * per), np.float32)
    ob = out.view(np.uint32)
    for c in range(F):
        vb = np.ascontiguousarray(vals[c], np.float32).view(np.uint32)
        fb = np.asarray([fills[c]], np.float32).view(np.uint32)[0]
        for r in range(n):
            ob[r, per * c] = vb[r] if valid[c][r] else fb
            if track:
                out[r, per * c + 1] = 0.0 if valid[c][r] else 1.0
    return out


VECTORIZE_N = (1, 63, 64, 65, 129)           # the tile is 64 rows x 32 columns
VECTORIZE_F = (1, 31, 32, 33, 65)
_FILLS = _f32_from_bits([0x3FC00000, 0x80000000, 0x00000003, 0xC2F60000, 0x00000000])     # 1.5, -0.0, denormal, -123, 0


def vectorize_case(n, F):
    """``(vals, valid, fills)``: column ``c`` is all valid when ``c % 7 == 0``, all null when ``c % 7 == 3`` (with one
    column: all null for even ``n``), mixed otherwise; valid values include SPECIAL_F32, null slots hold POISON_F32."""
    rng = np.random.default_rng(1000 * n + F)
    vals, valid = [], []
    for c in range(F):
        ok = rng.random(n) < 0.6
        if c % 7 == 0:
            ok[:] = True
        if c % 7 == 3 or (F == 1 and n % 2 == 0):
            ok[:] = False
        v = _values_f32(rng, n)
        v[~ok] = POISON_F32[rng.integers(0, len(POISON_F32), int((~ok).sum()))]
        vals.append(v)
        valid.append(ok)
    fills = _FILLS[np.arange(F) % len(_FILLS)].copy()
    return vals, valid, fills


# ======================================================================================================== onehot
def onehot(codes, luts, offs, n, W):
    """fp32 [n, W], zero but for 1.0 at ``off[c] + slot`` where ``slot = lut[code]`` for a code in ``[0, ln - 1)`` and
    ``lut[ln - 1]`` for any other code (-1, other negatives, codes >= ln - 1); slot -1 writes nothing."""
    out = np.zeros((n, W), np.float32)
    for code, lut, off in zip(codes, luts, offs):
        ln = len(lut)
        for r in range(n):
            c = int(code[r])
            slot = int(lut[c]) if 0 <= c < ln - 1 else int(lut[ln - 1])
            if slot != -1:
                out[r, off + slot] = 1.0
    return out


ONEHOT_N = (1, 255, 256, 257)                # 256 rows per block, one grid row per column
# ln = 1: only the "other" entry; -1 slots for a dictionary code and for "other"
ONEHOT_LUTS = (np.array([0], np.int32), np.array([2, -1, 0, 1], np.int32), np.array([3, 0, -1, 1, 2, 4, -1], np.int32))
ONEHOT_OFFS = (0, 1, 4)                      # widths 1, 3, 5
ONEHOT_W = 9


def onehot_case(n):
    """Codes of the three ONEHOT_LUTS columns: every row draws from {-1, -5, 0 .. ln-2, ln-1, ln, ln+3}; the first
    rows walk that set in order, so -1, ln-2, ln-1 and ln+3 occur whenever ``n`` allows, and for ``n == 1`` each column
    takes a different one of them."""
    rng = np.random.default_rng(77 + n)
    codes = []
    for j, lut in enumerate(ONEHOT_LUTS):
        ln = len(lut)
        pool = np.array(sorted({-1, -5, ln - 2, ln - 1, ln, ln + 3} | set(range(ln - 1))), np.int32)
        c = pool[rng.integers(0, len(pool), n)]
        lead = np.array([ln + 3, ln - 1, -1, ln - 2], np.int32)
        lead = np.roll(np.concatenate([lead, pool]), -j)[:n]
        c[:len(lead)] = lead
        codes.append(c.astype(np.int32))
    return codes


# ======================================================================================================== gather
def gather(blocks, rows, n):
    """``out[r, j]`` = the value at row ``rows[r]`` (``r`` when ``rows`` is None) of column ``j`` of the concatenation
    of the blocks; a block is ``(matrix [n, w], column index list or None)``. fp32 [m, k]."""
    src = list(range(n)) if rows is None else [int(r) for r in rows]
    cols = []
    for mat, ci in blocks:
        for j in (range(mat.shape[1]) if ci is None else [int(x) for x in ci]):
            cols.append((mat, j))
    out = np.zeros((len(src), len(cols)), np.float32)
    ob = out.view(np.uint32)
    for r, s in enumerate(src):
        for j, (mat, cj) in enumerate(cols):
            ob[r, j] = np.asarray(mat[s, cj], np.float32).reshape(1).view(np.uint32)[0]
    return out


GATHER_M = (1, 31, 32, 33, 65)               # the tile is 32 rows x 64 columns
GATHER_K = (1, 63, 64, 65, 130)
GATHER_SRC_ROWS = 41                         # source rows when a row list is given


def gather_case(m, k, listed):
    """``(blocks, rows, n)`` with ``k`` output columns and ``m`` output rows. ``listed``: ``rows`` is a non-monotone
    list with duplicates that holds row 0 and row n-1 (n = 41 source rows); else ``rows`` is None and n = m.
    k > 1: a [n, 1] block, a 20-column slice of a 29-column matrix (row stride 29), 17 columns of a 9-column matrix
    through a reversed index list with repeats, and a plain block for the rest. k == 1: the [n, 1] block alone, or
    (listed) one column of the 9-column matrix through an index list."""
    rng = np.random.default_rng(10000 * m + 10 * k + int(listed))
    n = GATHER_SRC_ROWS if listed else m
    rows = None
    if listed:
        rows = rng.integers(0, n, m)
        for i, r in enumerate((n - 1, 0, n - 1, 7, 7)[:m]):
            rows[i] = r
        if m == 1:
            rows[0] = n - 1
        rows = rows.astype(np.int64)

    def mat(w):
        return _values_f32(rng, n * w).reshape(n, w).copy()         # owns its data: a slice of it has it as .base
    wide, nine = mat(29), mat(9)
    if k == 1:
        blocks = [(nine, np.array([4], np.int64))] if listed else [(mat(1), None)]
    else:
        idx = np.array([8, 7, 7, 6, 5, 4, 3, 3, 2, 1, 0, 8, 8, 0, 4, 4, 2], np.int64)
        blocks = [(mat(1), None), (wide[:, 5:25], None), (nine, idx), (mat(k - 38), None)]
    return blocks, rows, n


# =================================================================================================== masked sums
def exact_sum(xs):
    """The sum of finite floats as a Fraction."""
    return sum((Fraction(float(x)) for x in xs), Fraction(0))


def masked_sums(vals, valid, n, rows_per_chunk):
    """fp64 [C, chunks, 2]: per column and chunk of ``rows_per_chunk`` rows, the (sum, count) of the valid values
    (``valid[c]`` None = all valid); the sum is exact, rounded once."""
    chunks = -(-n // rows_per_chunk)
    out = np.zeros((len(vals), chunks, 2), np.float64)
    for c, (v, ok) in enumerate(zip(vals, valid)):
        for k in range(chunks):
            r0, r1 = k * rows_per_chunk, min(n, (k + 1) * rows_per_chunk)
            xs = [v[r] for r in range(r0, r1) if ok is None or ok[r]]
            out[c, k] = (float(exact_sum(xs)), float(len(xs)))
    return out


COLSUM_N = (1, 255, 1023, 1024, 1025, 2049)  # 1024 rows per thread step


def colsum_chunkings(n):
    return sorted({n, 1024, 1000, 257})


def colsum_case(n, integer):
    """``(vals, valid)`` of six columns: fp32 mixed mask, fp64 no mask, fp32 all-false mask, fp64 mixed mask, fp32 no
    mask, fp64 all-true mask. Masked-out slots hold NaN or an infinity. ``integer``: values are integers in [-30, 30]
    (every partial sum exact in any order); else reals spread over six decades."""
    rng = np.random.default_rng(5 * n + int(integer))
    dts = (F32, F64, F32, F64, F32, F64)
    masks = ("mixed", None, "none", "mixed", None, "all")
    vals, valid = [], []
    for dt, mk in zip(dts, masks):
        if integer:
            v = rng.integers(-30, 31, n).astype(dt)
        else:
            v = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dt)
        ok = None if mk is None else (rng.random(n) < 0.5 if mk == "mixed" else np.full(n, mk == "all"))
        if ok is not None:
            v[~ok] = np.array([np.nan, np.inf, -np.inf], dt)[rng.integers(0, 3, int((~ok).sum()))]
        vals.append(v)
        valid.append(ok)
    return vals, valid


# ======================================================================================================= summary
NSTAT = 9        # count, nulls, min, max, sum x, sum x^2, sum x^3, sum x^4, sum of the label over the null rows


def _nan_min(xs):
    return float("nan") if any(x != x for x in xs) else min(xs, default=float("inf"))


def _nan_max(xs):
    return float("nan") if any(x != x for x in xs) else max(xs, default=float("-inf"))


def _round(fr_or_nan):
    return fr_or_nan if isinstance(fr_or_nan, float) else float(fr_or_nan)


def _power_sum(xs, k, absolute=False):
    """Exact ``sum x^k`` (``sum |x|^k``) as a Fraction; NaN (float) when a value is not finite."""
    if not all(math.isfinite(x) for x in xs):
        return float("nan")
    return sum(((abs(Fraction(x)) if absolute else Fraction(x)) ** k for x in xs), Fraction(0))


def summary(vals, valid, label=None, bounds=False):
    """fp64 [F, 9] per column: count and nulls; min and max of the valid values (an empty column: +inf / -inf; a NaN
    among them: NaN); the exact sums of x, x^2, x^3, x^4 rounded once; the sum of ``label`` over the null rows.
    ``bounds=True``: instead, [F, 9] Fractions, the error a device sum may show against the rounded oracle,
    ``(n + 3) 2^-53 sum |x|^k`` for the five sums (``n`` for the order of the n - 1 additions, 3 for the up to two
    roundings of forming x^k and the oracle's own), 0 for the other statistics."""
    n = len(vals[0])
    out = []
    for v, ok in zip(vals, valid):
        good = [ok is None or bool(ok[r]) for r in range(n)]
        xs = [float(v[r]) for r in range(n) if good[r]]
        ls = [] if label is None else [float(label[r]) for r in range(n) if not good[r]]
        if bounds:
            out.append([Fraction(0)] * 4 + [(n + 3) * U * _power_sum(xs, k, True) for k in (1, 2, 3, 4)] +
                       [(n + 3) * U * _power_sum(ls, 1, True)])
        else:
            out.append([float(len(xs)), float(n - len(xs)), _nan_min(xs), _nan_max(xs)] +
                       [_round(_power_sum(xs, k)) for k in (1, 2, 3, 4)] + [_round(_power_sum(ls, 1))])
    return out if bounds else np.array(out, np.float64).reshape(len(vals), NSTAT)


_SUMMARY_DTYPES = (F32, F64, I64, U8, BOOL)
_LABEL_DTYPES = (None, F32, F64, I64, BOOL)
# n below / across the 256-thread block and the 1024-row chunking (n = 2049, F = 3: 3 chunks of 683 rows); F across
# the 128-wide block of the fold kernel
SUMMARY_SHAPES = ((1, 1), (255, 3), (257, 130), (1023, 1), (2049, 3))
SUMMARY_CASES = tuple((n, F, integer) for n, F in SUMMARY_SHAPES for integer in (True, False))


def summary_case(n, F, integer):
    """``(vals, valid, label)``. Column ``c``: dtype cycles fp32, fp64, int64, uint8, bool (starting at a per-case
    offset), the mask cycles none / mixed / all-null (a single column: none for n = 1, mixed else). Float columns hold
    integers in [-30, 30] (``integer``) or reals; int64 holds [-30, 30], uint8 [0, 30]. Null slots of float columns
    hold NaN. The label dtype cycles through absent, fp32, fp64, int64, bool over SUMMARY_CASES; a float label is
    integer-valued when ``integer``."""
    i = SUMMARY_CASES.index((n, F, integer))
    rng = np.random.default_rng(900 + i)
    vals, valid = [], []
    first = (n > 1) if F == 1 else SUMMARY_SHAPES.index((n, F))       # single columns are fp32 (n = 1) and fp64
    for c in range(F):
        dt = _SUMMARY_DTYPES[(c + first) % 5]
        mk =("none", "mixed", "null")[c % 3] if F > 1 else ("none" if n == 1 else "mixed")
        if dt in (F32, F64):
            v = rng.integers(-30, 31, n).astype(dt) if integer else (rng.standard_normal(n) * 7.0).astype(dt)
        elif dt is I64:
            v = rng.integers(-30, 31, n).astype(dt)
        elif dt is U8:
            v = rng.integers(0, 31, n).astype(dt)
        else:
            v = rng.random(n) < 0.4
        ok = None if mk == "none" else (rng.random(n) < 0.7 if mk == "mixed" else np.zeros(n, bool))
        if ok is not None and dt in (F32, F64):
            v[~ok] = np.nan
        vals.append(v)
        valid.append(ok)
    ldt = _LABEL_DTYPES[i % 5]
    if ldt is None:
        label = None
    elif ldt is BOOL:
        label = rng.random(n) < 0.5
    elif ldt is I64 or integer:
        label = rng.integers(-3, 4, n).astype(ldt)
    else:
        label = rng.standard_normal(n).astype(ldt)
    return vals, valid, label


SUMMARY_NAN_SHAPES = ((257, 2), (2049, 3))


def summary_nan_case(n, F):
    """fp64 / fp32 columns with one NaN among the valid values, at a row of the last wave of the last chunk (it has
    to survive the wave, block and chunk folds); the last column of F = 3 has its NaN masked out instead."""
    rng = np.random.default_rng(40 + n)
    vals, valid = [], []
    for c in range(F):
        v = rng.standard_normal(n).astype((F64, F32)[c % 2])
        ok = rng.random(n) < 0.8
        ok[n - 3] = c < 2
        v[n - 3] = np.nan
        vals.append(v)
        valid.append(ok)
    return vals, valid


# ========================================================================================================== hist
def hist_splits(mn, mx, bins, fused=False):
    """The ``bins`` splits ``mn + step * b``, ``step = (mx - mn) / (bins - 2)``: a rounded product, then a rounded sum;
    ``fused``: the exact ``mn + step * b`` rounded once. Needs bins >= 3 (with bins == 2 the reference's own step is a
    division by zero; that case is left alone)."""
    assert bins >= 3
    step = (mx - mn) / (bins - 2.0)
    if fused:
        return [float(Fraction(mn) + Fraction(step) * b) for b in range(bins)]
    return [mn + step * b for b in range(bins)]


def hist_bucket(x, splits):
    """The last i with ``split[i] <= x`` when ``split[0] <= x < split[bins-1]``; anything else, NaN included: bins-1."""
    if splits[0] <= x < splits[-1]:
        return bisect.bisect_right(splits, x) - 1
    return len(splits) - 1


def hist(values, valid, mn, mx, bins, fused=False):
    """Counts [bins] (Python ints) of the valid values. ``!(mn < mx)``: [count(x == mx), count(x != mx), 0, ...]."""
    xs = [float(x) for r, x in enumerate(values) if valid is None or valid[r]]
    out = [0] * bins
    if not mn < mx:
        out[0] = sum(1 for x in xs if x == mx)
        out[1] = len(xs) - out[0]
        return out
    splits = hist_splits(mn, mx, bins, fused)
    for x in xs:
        out[hist_bucket(x, splits)] += 1
    return out


HIST_BINS = (3, 10, 12, 100, 101, 16384)
INTEGER_FIXTURES = ((100, -3.0, 6.0), (100, -3.0, 15.0), (100, -2.0, 7.0))      # (bins, min, max)
FIXTURE_MOVERS = {(100, -3.0, 6.0): (6.0,), (100, -3.0, 15.0): (6.0, 15.0), (100, -2.0, 7.0): (7.0,)}


def _edge_values(mn, mx, bins, dtype, rng):
    """The values a column of the histogram table holds: every split with its two neighbours, min, max, one value
    below min and one above the last split, NaN; in fp32, the fp32 roundings of the splits with their fp32 neighbours
    (where a split is representable that is the split itself); in int64, the integers around every split. Shuffled."""
    sp = np.array(hist_splits(mn, mx, bins), np.float64)
    step = (mx - mn) / (bins - 2.0)
    ends = [mn, mx, mn - 1.5 * step, sp[-1] + step]
    if dtype is F64:
        v = np.concatenate([sp, np.nextafter(sp, -np.inf), np.nextafter(sp, np.inf), ends, [np.nan]])
    elif dtype is F32:
        s32 = sp.astype(np.float32)
        v = np.concatenate([s32, np.nextafter(s32, np.float32(-np.inf)), np.nextafter(s32, np.float32(np.inf)),
                            np.array(ends, np.float32), np.array([np.nan], np.float32)])
    else:
        v = np.concatenate([np.floor(sp), np.ceil(sp), np.floor(ends), np.ceil(ends)]).astype(np.int64)
    v = v.astype(dtype)
    rng.shuffle(v)
    return v


def _column(name, values, lo, hi, rng=None, valid=None):
    values = np.asarray(values)
    if valid is None and rng is not None:         # some null rows, holding values that would count if they leaked
        valid = rng.random(len(values)) < 0.9
    return {"name": name, "values": values, "valid": valid, "lo": float(lo), "hi": float(hi)}


def _hist_group(bins):
    rng = np.random.default_rng(31 * bins)
    cols = []
    n_real = 2 if bins == 16384 else 8
    for i in range(n_real):
        mn = float(rng.standard_normal() * 10.0 ** rng.integers(-2, 3))
        mx = mn + float(abs(rng.standard_normal()) + 0.01) * 10.0 ** rng.integers(-1, 3)
        dt = F32 if i % 4 == 3 else F64
        cols.append(_column(f"real{i}-{dt.__name__}", _edge_values(mn, mx, bins, dt, rng), mn, mx, rng))
    # degenerate min == max beside regular columns (2 buckets in a row of `bins`): == max, != max, NaN
    cols.insert(1, _column("degenerate", np.array([2.5, 2.5, 3.0, np.nan, -2.5, 2.5, np.inf]), 2.5, 2.5))
    # fp32 values that sit exactly on splits: step 1/4, every split representable in fp32
    q_hi = -1.0 + 0.25 * (bins - 2)
    cols.append(_column("quarters-f32", _edge_values(-1.0, q_hi, bins, F32, rng), -1.0, q_hi, rng))
    # the empty summary (+inf, -inf): everything lands in bin 1
    cols.append(_column("empty-summary", np.array([0.0, -1.0, np.inf, np.nan, 1e300]), np.inf, -np.inf))
    # scoring use: lo / hi of another (training) column, values fall outside on both sides
    x = rng.standard_normal(300) * 3.0
    cols.append(_column("scoring-f64", x, -1.0, 2.0, rng))
    cols.append(_column("scoring-f32", x.astype(np.float32), -0.5, 0.75, rng))
    for b, mn, mx in INTEGER_FIXTURES:
        if b != bins:
            continue
        ints = np.arange(mn - 2, mx + 3)
        tag = f"int[{mn:g},{mx:g}]"
        cols.append(_column(tag + "-f64", np.concatenate([ints, _edge_values(mn, mx, bins, F64, rng)]), mn, mx, rng))
        cols.append(_column(tag + "-f32", np.concatenate([ints.astype(np.float32),
                                                          _edge_values(mn, mx, bins, F32, rng)]), mn, mx, rng))
        cols.append(_column(tag + "-i64", ints.astype(np.int64), mn, mx))
    i_mn, i_mx = -7.0, 40.0
    cols.append(_column("int64-edges", _edge_values(i_mn, i_mx, bins, I64, rng), i_mn, i_mx, rng))
    cols.append(_column("bool", rng.random(200) < 0.3, 0.0, 1.0, rng))
    cols.append(_column("bool-degenerate", rng.random(50) < 0.5, 1.0, 1.0))
    cols.append(_column("uint8", rng.integers(0, 9, 100).astype(np.uint8), 0.0, 8.0, rng))
    return _pad(cols)


def _pad(cols):
    """All columns of a group run in one call: pad to the longest with null rows (which hold the column's first value)."""
    n = max(len(c["values"]) for c in cols)
    for c in cols:
        k = n - len(c["values"])
        ok = np.ones(len(c["values"]), bool) if c["valid"] is None else c["valid"]
        if k:
            c["values"] = np.concatenate([c["values"], np.repeat(c["values"][:1], k)])
            ok = np.concatenate([ok, np.zeros(k, bool)])
            c["valid"] = ok
    return cols


def _merge_group():
    """n = 2049, F = 3 (3 chunks of 683 rows per column merge through the global atomics): a regular fp64 column, a
    degenerate one in the middle, an unmasked fp32 one with training bounds."""
    rng = np.random.default_rng(2049)
    a = rng.standard_normal(2049)
    b = rng.integers(0, 3, 2049).astype(np.float64)
    c = (rng.standard_normal(2049) * 2).astype(np.float32)
    return [_column("regular", a, a.min(), a.max(), rng), _column("degenerate", b, 1.0, 1.0, rng),
            _column("scoring-f32-nomask", c, -1.0, 1.5)]


_GROUPS = {}


def hist_groups():
    """``{id: (bins, [column, ...])}``, built once. A column is a dict: name, values (typed array), valid (bool array or
    None), lo, hi. All columns of a group have the same length and run in one call."""
    if not _GROUPS:
        for bins in HIST_BINS:
            _GROUPS[f"bins{bins}"] = (bins, _hist_group(bins))
        _GROUPS["merge-n2049-F3"] = (12, _merge_group())
    return _GROUPS


@functools.lru_cache(maxsize=None)
def hist_group_counts(group_id, fused=False):
    """int64 [F, bins], read-only: the oracle histogram of every column of a group (computed once per process)."""
    bins, cols = hist_groups()[group_id]
    out = np.array([hist(c["values"], c["valid"], c["lo"], c["hi"], bins, fused) for c in cols], np.int64)
    out.setflags(write=False)
    return out
