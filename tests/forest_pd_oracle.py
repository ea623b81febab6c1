"""Brute-force NumPy oracle of ``tree_engine.forest_partial_dependence`` and the shared cases of its tests.

Independent of the host twin and the kernel: for every requested column and every grid bin the oracle copies the
binned rows, overwrites the column with the bin and sums ``forest_predict_oracle.walk`` per tree (weights taken as
fp32, ``tree_out`` / ``n_out`` honoured). No path logic at all.

Tolerance (:func:`tolerance`): an ICE entry is the base (at most T contributions) plus a prefix sum of differences
(at most T more that have not cancelled), each rounded to the fixed-point quantum with an error <= 1 / (2 scale):
bounded here by ``2 T / scale``; the oracle sums T fp64 terms of magnitude <= S, the twin's exact integers stand
for up to 3 S: ``4 T 2^-52 S``. A sum over n rows gets n times that, at the sum's scale ``scale / 2^ceil(log2 n)``."""
import functools

import numpy as np

import forest_loco_oracle as L
import forest_predict_oracle as P
from transmogrifai_amd.models import tree_engine as te
from transmogrifai_amd.models.tree_engine import Forest

B = L.B


def ice(forest, Xb, cols, n_grid, rows=None, tree_weight=None, tree_out=None, n_out=None):
    """float64 ``[n, Q, NB, C]`` as ``forest_partial_dependence(..., ice=True)`` defines it."""
    T, K = forest.n_trees, forest.K
    w = np.ones(T) if tree_weight is None else np.asarray(tree_weight, np.float32).astype(np.float64)
    tout = np.zeros(T, np.int64) if tree_out is None else np.asarray(tree_out, np.int64)
    C = int(n_out) if n_out is not None else (int(tout.max()) if T else 0) + K
    X = np.asarray(Xb)
    X = X if rows is None else X[np.asarray(rows, np.int64)]
    n, NB = X.shape[0], int(n_grid)
    out = np.zeros((n, len(cols), NB, C))
    for q, c in enumerate(cols):
        Xp = np.repeat(X[None], NB, 0)                      # [NB, n, F]
        Xp[:, :, c] = np.arange(NB, dtype=X.dtype)[:, None]
        Xp = Xp.reshape(NB * n, -1)
        for t in range(T):
            s = P.walk(forest, Xp, None, [t], w).reshape(NB, n, K)
            out[:, q, :, tout[t]:tout[t] + K] += s.transpose(1, 0, 2)
    return out


def sum_scale(forest, n, tree_weight=None, tree_out=None):
    return te.forest_loco_plan(forest, tree_weight, tree_out).scale / 2.0 ** max(0, (n - 1).bit_length())


def tolerance(forest, tree_weight=None, tree_out=None, n_sum=None):
    """Of an ICE entry, or with ``n_sum`` of an entry of the sum over that many rows."""
    S = L.magnitude(forest, tree_weight)
    T = forest.n_trees
    if n_sum is None:
        return 2 * T / te.forest_loco_plan(forest, tree_weight, tree_out).scale + 4 * T * 2.0 ** -52 * S
    return n_sum * (2 * T / sum_scale(forest, n_sum, tree_weight, tree_out) + 4 * T * 2.0 ** -52 * S)


# ------------------------------------------------------------------------------------------------------ cases
def _one_row_one_col():
    rng = np.random.default_rng(31)
    f, X, cols = L._forest(rng, 1, 1, 40, 1, -1, 7)
    return f, X[:1], [int(cols[0])], B, {}


def _single_leaf_only():
    rng = np.random.default_rng(32)
    f = P.random_forest(rng, 2, 8, B, 1, single_leaf=(0, 1))
    return f, P.random_bins(rng, 67, 8, B), [0, 3], B, {}


def _k3_missing_rows_dup():
    rng = np.random.default_rng(33)
    f, X, cols = L._forest(rng, 9, 3, 40, 5, B - 1, 31, single_leaf=(4,),
                           values=lambda n, k: P.rounded_values(rng, n, k))
    rows = np.concatenate([rng.permutation(67)[:40], [5, 5]])
    return f, X, [int(c) for c in cols], B, dict(rows=rows, tree_weight=P.rounded_weights(rng, 9))


def _tree_out_n3():
    rng = np.random.default_rng(34)
    f, X, cols = L._forest(rng, 9, 1, 40, 37, -1, 41, values=lambda n, k: P.rounded_values(rng, n, k))
    return f, X, [int(c) for c in cols[::7]], B, dict(tree_weight=P.exact_weights(rng, 9), tree_out=np.arange(9) % 3,
                                                       n_out=3)


def _q37_unsplit():
    """37 requested columns of which seven are split on by no tree; three output columns."""
    rng = np.random.default_rng(35)
    f, X, cols = L._forest(rng, 9, 1, 40, 30, B - 1, 41, values=lambda n, k: P.rounded_values(rng, n, k))
    never = np.setdiff1d(np.arange(40), cols)
    want = rng.permutation(np.concatenate([cols, never[:7]]))
    assert want.size == 37
    return f, X, [int(c) for c in want], B, dict(tree_weight=P.rounded_weights(rng, 9), tree_out=np.arange(9) % 3,
                                                 n_out=3)


def _chain12_missing():
    rng = np.random.default_rng(36)
    f = P.chain_tree(rng, 12, 40, B, 1, missing_bin=B - 1)
    X = P.chain_rows(rng, 12, 40, B, 67, hi=B - 2)
    X = np.where(rng.random(X.shape) < 0.15, B - 1, X).astype(np.uint8)
    assert set(f.default_left[f.nodes[:, 2] >= 0]) == {0, 1}
    return f, X, [0, 3, 4, 11, 39], B, {}


def _mixed_depths_k3():
    rng = np.random.default_rng(37)
    X = P.random_bins(rng, 67, 40, B)
    parts = [P.random_forest(rng, 1, 40, B, 3, single_leaf=(0,)), P.chain_tree(rng, 12, 40, B, 3),
             P.random_forest(rng, 7, 40, B, 3, budget=21, X=X)]
    f = Forest.concat(parts)
    P.check_forest(f, 40, B)
    cols = [int(c) for c in L.used_columns(f)[:9]]
    return f, X, cols, B, dict(tree_weight=P.rounded_weights(rng, 9))


def _grid_rows(F=2):
    """Every bin of column 0 and of column 1 once (the other column at bin 7)."""
    X = np.full((2 * B, F), 7, np.uint8)
    X[:B, 0] = np.arange(B)
    X[B:, 1] = np.arange(B)
    return X


def _repeat_unreachable():
    """Column 0 twice on one path: root (0 <= 10) -> node 1 (0 <= 20). Node 1's right leaf (value 64) cannot be
    reached; the curve of column 0 has the two steps [0, 10] -> 1 and [11, 31] -> 4."""
    f = L._hand([(0, 10, 1, 2), (0, 20, 3, 4), (0, 0, -1, -1), (0, 0, -1, -1), (0, 0, -1, -1)], [0, 0, 4, 1, 64])
    return f, _grid_rows(), [0, 1], B, {}


def _split_edges():
    """Splits at bin 0, at the last ordinary bin (31: everything goes left) and at the one before it."""
    f = L._hand([(0, 0, 1, 2), (1, 31, 3, 4), (1, 30, 5, 6)] + [(0, 0, -1, -1)] * 4, [0, 0, 0, 1, 2, 3, 5])
    return f, _grid_rows(), [0, 1], B, {}


def _split_edges_missing():
    """The same with a missing bin: the last ordinary bin is 30, bin 31 follows the default directions (right)."""
    f = L._hand([(0, 0, 1, 2), (1, 30, 3, 4), (1, 29, 5, 6)] + [(0, 0, -1, -1)] * 4, [0, 0, 0, 1, 2, 3, 5], B - 1)
    return f, _grid_rows(), [0, 1], B, {}


def _equal_sides():
    """A split whose two leaves hold the same value: a flat curve made of two emitted steps that cancel."""
    f = L._hand([(0, 10, 1, 2), (0, 0, -1, -1), (1, 5, 3, 4), (0, 0, -1, -1), (0, 0, -1, -1)], [0, 2, 0, 2, 2])
    return f, _grid_rows(), [0, 1], B, {}


_BUILD = {"one_row_one_col": _one_row_one_col, "single_leaf_only": _single_leaf_only,
          "k3_missing_rows_dup": _k3_missing_rows_dup, "tree_out_n3": _tree_out_n3, "q37_unsplit": _q37_unsplit,
          "chain12_missing": _chain12_missing, "mixed_depths_k3": _mixed_depths_k3,
          "repeat_unreachable": _repeat_unreachable, "split_edges": _split_edges,
          "split_edges_missing": _split_edges_missing, "equal_sides": _equal_sides}
CASES = list(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    """``(forest, Xb, cols, n_grid, kwargs of forest_partial_dependence, oracle ICE)``, built once and shared; do
    not modify."""
    forest, Xb, cols, n_grid, kw = _BUILD[name]()
    P.check_forest(forest, Xb.shape[1], B)
    return forest, np.ascontiguousarray(Xb, np.uint8), cols, n_grid, kw, ice(forest, Xb, cols, n_grid, **kw)
