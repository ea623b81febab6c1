"""NumPy oracle of the staged evaluation of a boosted forest (``models/tree_engine.py forest_staged_eval``), written from
its contract: stage ``s`` is the trees ``stage_off[s]..stage_off[s + 1]``, tree ``t`` adds ``weight[t] * leaf value`` to
column ``tree_col[t]`` of the rows' fp64 margins, and after every stage a metric of the margins is taken. No native code:
the leaf every row reaches comes from ``forest_predict_oracle.reach`` (int64), the margins are float64 sums in tree
order, the logarithmic terms are evaluated in ``numpy.longdouble`` so that the oracle's own rounding is far below the
bound it grants.

*Exact* regime (:func:`case`): the forests of ``forest_predict_oracle`` (leaf values multiples of 1/16 in [-4, 4], weights
multiples of 1/4 in (0, 2], at most 80 trees), base margins multiples of 1/64 in [-8, 8], labels 0/1, multiples of 1/4
(regression) or class ids. Every staged margin is then a multiple of 1/64 below 2^10, so the margins, ``(m - y)^2``,
``|m - y|`` and their sums, the error counts and the AuPR count tables are exact whatever the summation order: compared
with equality. The logloss / mlogloss sums are compared within ``(n + 16) 2^-52 sum |term|``: n - 1 additions and a few
ulp of exp / log1p per term."""
import numpy as np

import forest_predict_oracle as FO
from transmogrifai_amd.models.tree_engine import Forest

LD = np.longdouble
BINS = 1 << 16
EXACT = ("error", "aucpr", "rmse", "mse", "mae", "merror")        # raw results compared with equality
BINARY, REGRESSION, MULTI = ("logloss", "error", "aucpr"), ("rmse", "mse", "mae"), ("mlogloss", "merror")


def staged_margins(forest, X, rows, stage_off, tree_col, K, weights, base):
    """float64 ``[S, n, K]``: the margins after every stage (``base``: a scalar or one per column)."""
    rows = np.arange(np.asarray(X).shape[0]) if rows is None else np.asarray(rows, np.int64)
    so = np.asarray(stage_off, np.int64)
    S = len(so) - 1
    m = np.zeros((len(rows), K)) + np.asarray(base, np.float64)
    out = np.zeros((S, len(rows), K))
    w = np.ones(forest.n_trees) if weights is None else np.asarray(weights, np.float64)
    col = np.zeros(forest.n_trees, np.int64) if tree_col is None else np.asarray(tree_col, np.int64)
    node = FO.reach(forest, X, rows, np.arange(so[0], so[-1])) if len(rows) and so[-1] > so[0] else None
    for s in range(S):
        for t in range(so[s], so[s + 1] if node is not None else so[s]):    # tree order, as the predictors add
            m[:, col[t]] += w[t] * forest.value[node[:, t - so[0]], 0].astype(np.float64)
        out[s] = m
    return out


def logloss_terms(m, y, scale):
    sm = LD(scale) * m.astype(LD)
    return np.log1p(np.exp(-np.abs(sm))) + (np.maximum(sm, 0) - y.astype(LD) * sm)


def mlogloss_terms(m, label):
    K = m.shape[1]
    m = m.astype(LD)
    r = np.arange(len(m))
    a = np.argmax(m, 1)                                          # first maximal class
    e = np.exp(m - m[r, a][:, None])
    e[r, a] = 0
    return (m[r, a] - m[r, np.clip(label, 0, K - 1)]) + np.log1p(e.sum(1))


def aupr_bin(pr, bins=BINS):
    """The score bin of ``boost_epilogue_kernel``: fp32 clamp and product, truncated."""
    sc = np.clip(pr.astype(np.float32), np.float32(0), np.float32(1))
    return (sc * np.float32(bins - 1)).astype(np.int64)


def aupr_slots(m, y, scale, bins=BINS):
    """``(slot, insensitive)``: each row's index into the ``[2, bins]`` table (bins in descending score order), and
    whether moving the probability by +-4 ulp leaves every row's bin unchanged."""
    pr = 1.0 / (1.0 + np.exp(-(scale * m)))
    b = aupr_bin(pr, bins)
    lo, hi = pr.copy(), pr.copy()
    for _ in range(4):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    same = bool(np.array_equal(aupr_bin(lo, bins), b) and np.array_equal(aupr_bin(hi, bins), b))
    return (y > 0.5).astype(np.int64) * bins + (bins - 1 - b), same


def raw(margins, y, metric, scale=1.0, bins=BINS):
    """What a predictor accumulates per stage, from ``margins`` ``[S, n, K]`` and the rows' labels ``y`` ``[n]``:
    ``(raw, bound)``. ``raw`` is float64 ``[S]`` sums, int64 ``[S]`` counts or int64 ``[S, 2, bins]`` tables; ``bound`` is the
    per-stage tolerance of a floating sum (0 where the result is exact)."""
    S, n, K = margins.shape
    y = np.asarray(y, np.float64)
    zero = np.zeros(S)
    if metric == "aucpr":
        out = np.zeros((S, 2 * bins), np.int64)
        for s in range(S):
            slot, same = aupr_slots(margins[s, :, 0], y, scale, bins)
            assert same, "a probability sits within 4 ulp of a bin edge: the case cannot judge a predictor"
            np.add.at(out[s], slot, 1)
        return out.reshape(S, 2, bins), zero
    if metric == "error":
        return ((scale * margins[:, :, 0] > 0) != (y > 0.5)[None, :]).sum(1).astype(np.int64), zero
    if metric == "merror":
        return (np.argmax(margins, 2) != y.astype(np.int64)[None, :]).sum(1).astype(np.int64), zero
    if metric in ("rmse", "mse"):
        return ((margins[:, :, 0] - y[None, :]) ** 2).sum(1), zero
    if metric == "mae":
        return np.abs(margins[:, :, 0] - y[None, :]).sum(1), zero
    if metric == "logloss":
        t = np.stack([logloss_terms(margins[s, :, 0], y, scale) for s in range(S)]) if S else np.zeros((0, n), LD)
    elif metric == "mlogloss":
        t = np.stack([mlogloss_terms(margins[s], y.astype(np.int64)) for s in range(S)]) if S else np.zeros((0, n), LD)
    else:
        raise ValueError(metric)
    return t.sum(1).astype(np.float64), ((n + 16) * 2.0 ** -52 * np.abs(t).sum(1)).astype(np.float64)


def finish(r, n, metric):
    """The metric as the user reads it, from the raw sums / counts (``aucpr`` is finished by
    ``evaluators.metrics.binned_aupr_from_counts``, which this oracle does not restate)."""
    v = np.asarray(r, np.float64) / max(n, 1)
    return np.sqrt(v) if metric == "rmse" else v


def assert_raw(got, want, bound, metric):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    if metric in EXACT:
        np.testing.assert_array_equal(got.astype(want.dtype), want)
        return
    err = np.abs(got - want)
    assert (err <= bound).all(), f"stage sums past the bound: worst err / bound {np.max(err / np.maximum(bound, 1e-300))}"


# ------------------------------------------------------------------------------------------------ cases
def case(seed, metric, *, n, F, K=1, stages=(1,), missing=False, row_list=False, shape="random", B=32):
    """One exact-regime input: a dict with the forest, the binned rows ``X`` (uint8 ``[N, F]``), ``rows`` (None or int64
    ids, shuffled, with rows of ``X`` left out), labels ``y`` (float32 ``[N]``), ``stage_off``, ``tree_col``, ``weights``,
    ``base`` and the call's ``K`` / ``metric`` / ``scale``. ``stages``: trees per stage (zeros allowed). ``shape``:
    ``random`` trees, ``leaf`` (every other tree a single leaf) or ``chain`` (the first tree a 40-deep spine, F
    permitting)."""
    rng = np.random.default_rng(seed)
    stages = list(stages)
    T = int(sum(stages))
    assert T <= FO.EXACT_MAX_TREES and (K == 1 or metric in MULTI)
    N = n + 9 if row_list else n
    mb = B - 1 if missing else -1
    depth = min(40, F)
    X = FO.random_bins(rng, N, F, B, mb)
    if shape == "chain" and N:
        X = FO.chain_rows(rng, depth, F, B, N, hi=B - 2 if missing else None)
        if missing:
            X = np.where(rng.random(X.shape) < 0.1, mb, X).astype(np.uint8)
    parts = []
    if T:
        if shape == "chain":
            parts.append(FO.chain_tree(rng, depth, F, B, 1, missing_bin=mb))
        if T - len(parts):
            nt = T - len(parts)
            parts.append(FO.random_forest(rng, nt, F, B, 1, budget=rng.integers(3, 16, nt).tolist(),
                                          single_leaf=range(0, nt, 2) if shape == "leaf" else (), missing_bin=mb,
                                          X=X if N else None))
        forest = Forest.concat(parts)
    else:
        forest = Forest(np.zeros(1, np.int64), np.zeros((0, 4), np.int32), np.zeros(0, np.uint8),
                        np.zeros((0, 1), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32),
                        np.zeros(0, np.int32), mb)
    rows = rng.permutation(N)[:n].astype(np.int64) if row_list else None
    if metric in BINARY:
        y = rng.integers(0, 2, N)
    elif metric in REGRESSION:
        y = rng.integers(-32, 33, N) / 4.0
    else:
        y = rng.integers(0, K + 1, N)            # K itself occurs: mlogloss clamps it, merror counts it as wrong
    base = rng.integers(-512, 513, K if metric in MULTI else 1) / 64.0
    return {"forest": forest, "X": X, "rows": rows, "y": y.astype(np.float32),
            "stage_off": np.concatenate([[0], np.cumsum(stages)]).astype(np.int64),
            "tree_col": rng.integers(0, K, T).astype(np.int32), "weights": FO.exact_weights(rng, T) if T else
            np.zeros(0, np.float32), "base": base if metric in MULTI else float(base[0]), "K": K, "metric": metric,
            "scale": 2.0 if (metric in BINARY and seed % 2) else 1.0}


def expect(c):
    """``(margins [S, n, K], raw, bound)`` of a :func:`case`."""
    rows = np.arange(len(c["X"])) if c["rows"] is None else c["rows"]
    m = staged_margins(c["forest"], c["X"], rows, c["stage_off"], c["tree_col"], c["K"], c["weights"], c["base"])
    assert np.array_equal(m * 64, np.rint(m * 64)) and (np.abs(m).max() if m.size else 0) < 2 ** 10
    r, b = raw(m, c["y"][rows], c["metric"], c["scale"])
    return m, r, b
