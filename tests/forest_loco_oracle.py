"""Brute-force NumPy oracle of ``tree_engine.forest_loco`` and the shared cases of its tests.

Independent of the host twin and the kernel: for every candidate (a used column, or a column group) the oracle copies
the binned rows, overwrites the candidate's columns with their zero bins, walks every tree again with the vectorised
fp64 walk of ``forest_predict_oracle`` and subtracts the unperturbed sum. No path logic at all.

Tolerance (:func:`tolerance`): the twin rounds each of at most T contributions of a slot to the fixed-point quantum
(error <= 1 / (2 scale) each, bounded here by ``T / scale``) and the oracle sums T fp64 terms of magnitude <= S
(``T 2^-52 S``). A slot in which no tree changes is exactly 0.0 in both."""
import functools

import numpy as np

import forest_predict_oracle as P
from transmogrifai_amd.models import tree_engine as te
from transmogrifai_amd.models.tree_engine import Forest

B = 32


def used_columns(forest):
    return np.unique(forest.nodes[forest.nodes[:, 2] >= 0, 0]).astype(np.int64)


def loco(forest, Xb, zero_bins, rows=None, groups=None, tree_weight=None, tree_out=None, n_out=None):
    """float64 ``[n, U + G + 1, C]`` as ``forest_loco`` defines it, and the used columns."""
    T, K = forest.n_trees, forest.K
    w = np.ones(T) if tree_weight is None else np.asarray(tree_weight, np.float32).astype(np.float64)
    tout = np.zeros(T, np.int64) if tree_out is None else np.asarray(tree_out, np.int64)
    C = int(n_out) if n_out is not None else (int(tout.max()) if T else 0) + K
    X = np.asarray(Xb)
    X = X if rows is None else X[np.asarray(rows, np.int64)]
    zb = np.asarray(zero_bins, np.uint8)
    used = used_columns(forest)
    value = forest.value.astype(np.float64)

    def sums(Xm):
        node = P.reach(forest, Xm, None, np.arange(T))
        out = np.zeros((Xm.shape[0], C))
        for t in range(T):
            out[:, tout[t]:tout[t] + K] += w[t] * value[node[:, t]]
        return out

    base = sums(X)
    cands = [[int(c)] for c in used] + [[int(c) for c in g] for g in (groups or [])]
    out = np.zeros((X.shape[0], len(cands) + 1, C))
    for s, cols in enumerate(cands):
        Xp = X.copy()
        Xp[:, cols] = zb[cols]
        out[:, s] = sums(Xp) - base
    out[:, -1] = base
    return out, used


def magnitude(forest, tree_weight=None):
    """S = sum_t |w_t| max_node |value_t| with the weights as fp32."""
    w = np.ones(forest.n_trees) if tree_weight is None else np.asarray(tree_weight, np.float32).astype(np.float64)
    return float(sum(abs(w[t]) * np.abs(forest.value[int(forest.tree_off[t]):int(forest.tree_off[t + 1])]).max()
                     for t in range(forest.n_trees)))


def tolerance(forest, tree_weight=None, tree_out=None):
    S = magnitude(forest, tree_weight)
    scale = te.forest_loco_plan(forest, tree_weight, tree_out).scale
    T = forest.n_trees
    return T / scale + T * 2.0 ** -52 * S


# ------------------------------------------------------------------------------------------------------ cases
def _spread(rng, forest, U, F):
    """Relabel the split columns so that exactly ``U`` distinct ones occur, spread over ``[0, F)``: the first U
    internal nodes take each once, the others a random one of them."""
    cols = np.sort(rng.choice(F, U, replace=False))
    internal = np.nonzero(forest.nodes[:, 2] >= 0)[0]
    assert internal.size >= U, "not enough splits for the wanted number of used columns"
    pick = np.concatenate([rng.permutation(U), rng.integers(0, U, internal.size - U)])
    forest.nodes[internal, 0] = cols[pick]
    assert used_columns(forest).size == U
    return cols


def _forest(rng, T, K, F, U, missing_bin, budget, single_leaf=(), values=None):
    X = P.random_bins(rng, 67, F, B, missing_bin)
    f = P.random_forest(rng, T, F, B, K, budget=budget, single_leaf=single_leaf, missing_bin=missing_bin, X=X,
                        values=values)
    cols = _spread(rng, f, U, F)
    P.check_forest(f, F, B)
    return f, X, cols


def _zero_bins(rng, F, missing_bin, some_missing=False):
    zb = rng.integers(0, B - 1, F).astype(np.uint8)
    if some_missing and missing_bin >= 0:
        zb[rng.random(F) < 0.2] = missing_bin          # a model whose missing value is 0
    return zb


def _one_row_u1():
    rng = np.random.default_rng(11)
    f, X, _ = _forest(rng, 1, 1, 40, 1, -1, 7)
    return f, X[:1], _zero_bins(rng, 40, -1), {}


def _single_leaf_only():
    rng = np.random.default_rng(12)
    f = P.random_forest(rng, 1, 8, B, 1, single_leaf=(0,))
    return f, P.random_bins(rng, 67, 8, B), _zero_bins(rng, 8, -1), {}


def _u5_t9_k3_missing():
    rng = np.random.default_rng(13)
    f, X, _ = _forest(rng, 9, 3, 40, 5, B - 1, 31, single_leaf=(4,),
                      values=lambda n, k: P.rounded_values(rng, n, k))
    rows = np.concatenate([rng.permutation(67)[:40], [5, 5]])
    return f, X, _zero_bins(rng, 40, B - 1, True), dict(rows=rows, tree_weight=P.rounded_weights(rng, 9))


def _u37_t9_tree_out_groups():
    rng = np.random.default_rng(14)
    f, X, cols = _forest(rng, 9, 1, 40, 37, -1, 41, values=lambda n, k: P.rounded_values(rng, n, k))
    never = np.setdiff1d(np.arange(40), cols)
    # group 0: a node's column and its child's column (they follow each other on a path); group 1 holds a column
    # no tree splits on
    nd = f.nodes
    parent = next(k for k in range(len(nd)) if nd[k, 2] >= 0 and nd[nd[k, 2], 2] >= 0
                  and nd[nd[k, 2], 0] != nd[k, 0])
    g0 = [int(nd[parent, 0]), int(nd[nd[parent, 2], 0])]
    g1 = [int(c) for c in cols if int(c) not in g0][:2] + [int(never[0])]
    return f, X, _zero_bins(rng, 40, -1), dict(groups=[np.asarray(g0), np.asarray(g1)],
                                               tree_weight=P.exact_weights(rng, 9), tree_out=np.arange(9) % 3,
                                               n_out=3)


def _u37_t1():
    rng = np.random.default_rng(15)
    f, X, _ = _forest(rng, 1, 1, 40, 37, B - 1, 91)
    return f, X, _zero_bins(rng, 40, B - 1), dict(tree_weight=np.asarray([0.375], np.float32))


def _chain12_groups():
    """Depth-12 spine over columns 0..11; group 0 = three columns that follow one another on the spine, group 1 = a
    spine column and column 39, which no tree splits on. Missing cells with both default directions."""
    rng = np.random.default_rng(16)
    f = P.chain_tree(rng, 12, 40, B, 1, missing_bin=B - 1)
    X = P.chain_rows(rng, 12, 40, B, 67, hi=B - 2)
    X = np.where(rng.random(X.shape) < 0.15, B - 1, X).astype(np.uint8)
    assert set(f.default_left[f.nodes[:, 2] >= 0]) == {0, 1}
    return f, X, _zero_bins(rng, 40, B - 1, True), dict(groups=[np.asarray([3, 4, 5]), np.asarray([7, 39])])


def _mixed_depths_k3():
    """A single leaf, a depth-12 spine and random trees in one forest of T = 9, three values per leaf."""
    rng = np.random.default_rng(17)
    X = P.random_bins(rng, 67, 40, B)
    parts = [P.random_forest(rng, 1, 40, B, 3, single_leaf=(0,)), P.chain_tree(rng, 12, 40, B, 3),
             P.random_forest(rng, 7, 40, B, 3, budget=21, X=X)]
    f = Forest.concat(parts)
    P.check_forest(f, 40, B)
    return f, X, _zero_bins(rng, 40, -1), dict(tree_weight=P.rounded_weights(rng, 9),
                                               groups=[np.asarray([0, 1, 2]), np.asarray([20, 21])])


def _hand(nodes, values, missing_bin=-1):
    n = len(nodes)
    nd = np.asarray(nodes, np.int32)
    return Forest(np.asarray([0, n], np.int64), nd, np.zeros(n, np.uint8), np.asarray(values, np.float32).reshape(n, 1),
                  np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(1, np.int32), missing_bin)


def _repeat_feature():
    """Column 0 twice on one path, both nodes flip: root (0 <= 10) -> node 1 (0 <= 5) -> leaf 3. With column 0 at
    its zero bin 20 the row goes root -> leaf 2: the delta is value[2] - value[3] = 3, once; counting the second
    flipped node too would add value[4] - value[3]."""
    f = _hand([(0, 10, 1, 2), (0, 5, 3, 4), (0, 0, -1, -1), (0, 0, -1, -1), (0, 0, -1, -1)], [0, 0, 4, 1, 2])
    return f, np.asarray([[3, 0]], np.uint8), np.asarray([20, 0], np.uint8), {}


def _group_back():
    """Two members of one group on one path. Alone, column 0 moves the row from leaf 3 to leaf 5 (+2) and column 1
    to leaf 4 (+1); together they lead to leaf 6, which holds the original leaf's value: the group's delta is
    exactly 0. (A perturbed walk cannot end in the very leaf it left -- its first flipped node turns the other
    way -- so "back to the original leaf" is a leaf of the same value.)"""
    f = _hand([(0, 10, 1, 2), (1, 10, 3, 4), (1, 10, 5, 6)] + [(0, 0, -1, -1)] * 4, [0, 0, 0, 1, 2, 3, 1])
    return f, np.asarray([[3, 3]], np.uint8), np.asarray([20, 20], np.uint8), dict(groups=[np.asarray([0, 1])])


_BUILD = {"one_row_u1": _one_row_u1, "single_leaf_only": _single_leaf_only, "u5_t9_k3_missing": _u5_t9_k3_missing,
          "u37_t9_tree_out_groups": _u37_t9_tree_out_groups, "u37_t1": _u37_t1, "chain12_groups": _chain12_groups,
          "mixed_depths_k3": _mixed_depths_k3, "repeat_feature": _repeat_feature, "group_back": _group_back}
CASES = list(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    """``(forest, Xb, zero_bins, kwargs of forest_loco, oracle output)``, built once and shared; do not modify."""
    forest, Xb, zb, kw = _BUILD[name]()
    want, _ = loco(forest, Xb, zb, **kw)
    return forest, np.ascontiguousarray(Xb, np.uint8), zb, kw, want
