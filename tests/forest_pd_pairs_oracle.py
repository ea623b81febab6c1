"""Brute-force NumPy oracle of ``tree_engine.forest_partial_dependence_pairs`` and the shared cases of its tests.

Independent of the host twin and the kernel: for every pair and every cell ``(i, j)`` of the grid the oracle copies
the binned rows, overwrites the pair's two columns with the bins and sums ``forest_predict_oracle.walk`` per tree
(weights taken as fp32, ``tree_out`` / ``n_out`` honoured, a tree without nodes skipped). No path logic at all.
:func:`cells` does the same for a list of cells only, for spot checks on wide grids.

Tolerance: ``forest_pd_oracle.tolerance`` as it stands. A cell of a surface gets at most one rounded delta per tree
on top of the base, the same count as a point of a 1-D curve, so the same bound holds."""
import functools
import itertools

import numpy as np

import forest_loco_oracle as L
import forest_pd_oracle as O
import forest_predict_oracle as P
from transmogrifai_amd.models.tree_engine import Forest

B = L.B


def tolerance(forest, tree_weight=None, tree_out=None, n_sum=None):
    """``forest_pd_oracle.tolerance`` of the forest's trees that have nodes (a tree without nodes adds nothing to the
    result, and that function takes the largest value of every tree)."""
    off = np.asarray(forest.tree_off, np.int64)
    live = off[1:] > off[:-1]
    if live.all():
        return O.tolerance(forest, tree_weight, tree_out, n_sum)
    f = Forest(np.concatenate([off[:1], off[1:][live]]), forest.nodes, forest.default_left, forest.value, forest.gain,
               forest.cover, forest.tree_model[live], forest.missing_bin)
    return O.tolerance(f, None if tree_weight is None else np.asarray(tree_weight)[live],
                       None if tree_out is None else np.asarray(tree_out)[live], n_sum)


def _setup(forest, Xb, rows, tree_weight, tree_out, n_out):
    T, K = forest.n_trees, forest.K
    w = np.ones(T) if tree_weight is None else np.asarray(tree_weight, np.float32).astype(np.float64)
    tout = np.zeros(T, np.int64) if tree_out is None else np.asarray(tree_out, np.int64)
    C = int(n_out) if n_out is not None else (int(tout.max()) if T else 0) + K
    X = np.asarray(Xb)
    X = X if rows is None else X[np.asarray(rows, np.int64)]
    live = [t for t in range(T) if forest.tree_off[t + 1] > forest.tree_off[t]]
    return w, tout, C, X, live, K


def cells(forest, Xb, pair, at, rows=None, tree_weight=None, tree_out=None, n_out=None):
    """float64 ``[n, len(at), C]``: the surface of the pair ``(a, b)`` at the cells ``at`` (a list of ``(i, j)``)."""
    w, tout, C, X, live, K = _setup(forest, Xb, rows, tree_weight, tree_out, n_out)
    at = np.asarray(at, np.int64).reshape(-1, 2)
    n, m = X.shape[0], at.shape[0]
    Xp = np.repeat(X[None], m, 0)                               # [m, n, F]
    Xp[:, :, pair[0]] = at[:, 0].astype(X.dtype)[:, None]
    Xp[:, :, pair[1]] = at[:, 1].astype(X.dtype)[:, None]
    Xp = Xp.reshape(m * n, -1)
    out = np.zeros((n, m, C))
    for t in live:
        s = P.walk(forest, Xp, None, [t], w).reshape(m, n, K)
        out[:, :, tout[t]:tout[t] + K] += s.transpose(1, 0, 2)
    return out


def ice2(forest, Xb, pairs, n_grid, rows=None, tree_weight=None, tree_out=None, n_out=None):
    """float64 ``[n, Pn, NB, NB, C]`` as ``forest_partial_dependence_pairs(..., ice=True)`` defines it."""
    NB = int(n_grid)
    grid = [(i, j) for i in range(NB) for j in range(NB)]
    per = [cells(forest, Xb, p, grid, rows, tree_weight, tree_out, n_out) for p in pairs]
    n, C = per[0].shape[0], per[0].shape[2]
    return np.stack([s.reshape(n, NB, NB, C) for s in per], 1)


# ------------------------------------------------------------------------------------------------------ cases
def _hand(nodes, values, default_left=None, missing_bin=-1):
    f = L._hand(nodes, values, missing_bin)
    if default_left is not None:
        f.default_left[:] = np.asarray(default_left, np.uint8)
    return f


def _ordered(cols, k):
    return [p for p in itertools.permutations([int(c) for c in cols], 2)][:k]


def _unsplit_mixed():
    """Two never-split columns; a split and a never-split column in both orders; two split columns in both orders."""
    f, X, cols, _, kw = O._BUILD["q37_unsplit"]()
    used = set(L.used_columns(f).tolist())
    never = [c for c in cols if c not in used]
    split = [c for c in cols if c in used]
    pairs = [(never[0], never[1]), (split[0], never[0]), (never[0], split[0]), (split[1], split[2]),
             (split[2], split[1]), (split[0], split[3])]
    return f, X, pairs, B, kw


def _k3_missing_rows_dup():
    f, X, cols, _, kw = O._BUILD["k3_missing_rows_dup"]()
    return f, X, _ordered(cols, 6), B, kw


def _tree_out_n3():
    f, X, cols, _, kw = O._BUILD["tree_out_n3"]()
    return f, X, _ordered(cols[:3], 6), B, kw


def _chain12_missing():
    """The spine tests column d at depth d: (0, 3) has a above b, (3, 0) b above a; 39 is never split on."""
    f, X, _, _, kw = O._BUILD["chain12_missing"]()
    return f, X, [(0, 3), (3, 0), (4, 11), (11, 39), (39, 0), (3, 4)], B, kw


def _mixed_depths_k3():
    f, X, cols, _, kw = O._BUILD["mixed_depths_k3"]()
    return f, X, _ordered(cols[:4], 6), B, kw


def _single_leaf_and_empty():
    """Two single-leaf trees with a tree of no nodes between them."""
    f, X, _, _, kw = O._BUILD["single_leaf_only"]()
    g = Forest(np.asarray([0, 1, 1, 2], np.int64), f.nodes, f.default_left, f.value, f.gain, f.cover,
               np.zeros(3, np.int32), f.missing_bin)
    return g, X, [(0, 3), (3, 0)], B, kw


def _product_rows(step=5):
    """Rows on a product grid of columns 0 and 1 (every ``step``-th bin and the last), column 2 at bin 7."""
    v = sorted(set(range(0, B, step)) | {B - 1})
    X = np.asarray([(i, j, 7) for i in v for j in v], np.uint8)
    assert X.shape[0] <= 67
    return X


def _repeat_aba():
    """A path a, b, a: root (0 <= 10) -> node 1 (1 <= 15) -> node 3 (0 <= 20). Node 3's right leaf (value 64)
    cannot be reached: column 0 is at most 10 there."""
    f = _hand([(0, 10, 1, 2), (1, 15, 3, 4), (0, 0, -1, -1), (0, 20, 5, 6), (0, 0, -1, -1), (0, 0, -1, -1),
               (0, 0, -1, -1)], [0, 0, 4, 0, 2, 1, 64])
    return f, _product_rows(), [(0, 1), (1, 0), (0, 2)], B, {}


def _edge_trees(last, missing_bin):
    """Two trees whose splits sit at bin 0 and at the last ordinary bin ``last``, with the default directions both
    ways on both columns, so that the grid's last line, last column and corner differ from their neighbours."""
    leaves = [(0, 0, -1, -1)] * 4
    t1 = _hand([(0, 0, 1, 2), (1, last, 3, 4), (1, 0, 5, 6)] + leaves, [0, 0, 0, 1, 2, 3, 5], [1, 0, 1, 0, 0, 0, 0],
               missing_bin)
    t2 = _hand([(1, last - 1, 1, 2), (0, last, 3, 4), (0, 0, 5, 6)] + leaves, [0, 0, 0, 7, 11, 13, 17],
               [0, 1, 0, 0, 0, 0, 0], missing_bin)
    return Forest.concat([t1, t2])


def _split_edges():
    return _edge_trees(B - 1, -1), _product_rows(), [(0, 1), (1, 0)], B, {}


def _split_edges_missing():
    X = _product_rows()
    return _edge_trees(B - 2, B - 1), X, [(0, 1), (1, 0), (2, 1)], B, {}


def _equal_sides():
    f, X, _, _, kw = O._BUILD["equal_sides"]()
    return f, X, [(0, 1), (1, 0)], B, kw


def _one_row_one_pair():
    rng = np.random.default_rng(51)
    f, X, cols = L._forest(rng, 1, 1, 40, 2, -1, 7)
    return f, X[:1], [(int(cols[0]), int(cols[1]))], B, {}


_BUILD = {"unsplit_mixed": _unsplit_mixed, "k3_missing_rows_dup": _k3_missing_rows_dup, "tree_out_n3": _tree_out_n3,
          "chain12_missing": _chain12_missing, "mixed_depths_k3": _mixed_depths_k3,
          "single_leaf_and_empty": _single_leaf_and_empty, "repeat_aba": _repeat_aba, "split_edges": _split_edges,
          "split_edges_missing": _split_edges_missing, "equal_sides": _equal_sides,
          "one_row_one_pair": _one_row_one_pair}
CASES = list(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    """``(forest, Xb, pairs, n_grid, kwargs of forest_partial_dependence_pairs, oracle surfaces)``, built once and
    shared; do not modify."""
    forest, Xb, pairs, n_grid, kw = _BUILD[name]()
    assert Xb.shape[0] <= 67 and len(pairs) <= 6
    if name != "single_leaf_and_empty":                 # check_forest asks every tree for a root
        P.check_forest(forest, Xb.shape[1], B)
    Xb = np.ascontiguousarray(Xb, np.uint8)
    return forest, Xb, [tuple(p) for p in pairs], n_grid, kw, ice2(forest, Xb, pairs, n_grid, **kw)
