"""NumPy oracle of forest prediction, written from the data contract of ``models/tree_engine.py`` ``Forest`` (nodes are
``(feat, bin, left, right)`` with global child indices, ``left < 0`` marks a leaf, trees are BFS ordered, ``default_left``
per node, ``missing_bin`` per forest, values ``[n, K]``) and the routing rule ``goes_left`` of ``common/tree_rules.hpp``.
No native code: forests are built by hand (no grower), the walk is a vectorised level-by-level descent in int64 /
float64. tests/test_forest_predict_oracle.py checks it against the host twin, which entitles it to judge the HIP
kernels in tests/test_forest_predict_kernels_gpu.py.

Two value regimes. *Exact*: leaf values are multiples of 1/16 in [-4, 4] and tree weights multiples of 1/4 in (0, 2],
so every product is a multiple of 1/64 of magnitude <= 8 and every partial sum over T <= 80 trees, in any order, a
multiple of 1/64 below 2^10: 16 significant bits, exact in fp32, so predictor and oracle agree bit for bit whatever the
summation order or use of fma. *Rounded*: arbitrary fp32 values and weights; a predictor that rounds each product and
each of its T - 1 additions once (unit roundoff 2^-24) is within ``(T + 2) 2^-24 sum_t |w_t v_t|`` of the exact sum,
the bound tests/test_tree_shap.py uses, here evaluated per row and output by :func:`bound`."""
import numpy as np

from transmogrifai_amd.models.tree_engine import Forest

EXACT_MAX_TREES = 80


def goes_left(bins, split_bin, default_left, missing_bin):
    """A row whose bin is the missing bin (when there is one) follows the node's default; any other goes left when
    ``bin <= split_bin``."""
    bins = np.asarray(bins, np.int64)
    natural = bins <= np.asarray(split_bin, np.int64)
    if missing_bin < 0:
        return natural
    return np.where(bins == missing_bin, np.asarray(default_left) != 0, natural)


def variant_stop(forest, max_depth, min_gain):
    """``stop(node_ids, depth)`` of the pruned variant ``(max_depth, min_gain)`` (``prune_forest``): a node ends the
    walk when it is a grown leaf, lies at ``depth >= max_depth`` or has a stored fp32 gain below ``float32(min_gain)``."""
    mg = np.float32(min_gain)

    def stop(node_ids, depth):
        return (forest.nodes[node_ids, 2] < 0) | (depth >= max_depth) | (forest.gain[node_ids] < mg)
    return stop


def reach(forest, X, rows, trees, stop=None):
    """int64 ``[len(rows), len(trees)]``: the node at which each row's walk of each tree ends."""
    X = np.asarray(X)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows, np.int64)
    trees = np.asarray(trees, np.int64).reshape(-1)
    nd = forest.nodes.astype(np.int64)
    node = np.broadcast_to(forest.tree_off[:-1][trees].astype(np.int64), (len(rows), len(trees))).copy()
    if node.size == 0:
        return node
    if stop is None:
        def stop(ids, depth):
            return nd[ids, 2] < 0
    live = np.ones(node.shape, bool)
    depth = 0
    while True:
        live &= ~stop(node, depth)
        if not live.any():
            return node
        r, t = np.nonzero(live)
        k = node[r, t]
        assert (nd[k, 2] >= 0).all(), "the stop rule must stop at grown leaves"
        left = goes_left(X[rows[r], nd[k, 0]], nd[k, 1], forest.default_left[k], forest.missing_bin)
        node[r, t] = np.where(left, nd[k, 2], nd[k, 3])
        depth += 1


def _weights(forest, trees, weights):
    w = np.ones(forest.n_trees) if weights is None else np.asarray(weights, np.float64)
    return w[np.asarray(trees, np.int64).reshape(-1)]


def walk(forest, X, rows, trees, weights=None, stop=None):
    """float64 ``[len(rows), K]``: the weighted sum over ``trees`` (indices into the forest; ``weights`` is indexed
    by tree index as ``forest_predict``'s ``tree_weight`` is) of the value of the node where each row's walk ends."""
    node = reach(forest, X, rows, trees, stop)
    v = forest.value.astype(np.float64)[node]                       # [R, T, K]
    return (v * _weights(forest, trees, weights)[None, :, None]).sum(1)


def bound(forest, X, rows, trees, weights=None, stop=None):
    """Per row and output, the fp32 summation bound ``(T + 2) 2^-24 sum_t |w_t v_t|`` of the rounded regime."""
    node = reach(forest, X, rows, trees, stop)
    v = np.abs(forest.value.astype(np.float64)[node] * _weights(forest, trees, weights)[None, :, None])
    return (node.shape[1] + 2) * 2.0 ** -24 * v.sum(1)


def assert_matches(got, forest, X, rows, trees, weights=None, stop=None, exact=True):
    """``got`` (float32 ``[len(rows), K]``) against :func:`walk`: equal in the exact regime, within :func:`bound` in
    the rounded one."""
    want = walk(forest, X, rows, trees, weights, stop)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    if exact:
        np.testing.assert_array_equal(got.astype(np.float64), want)
        return
    err = np.abs(got.astype(np.float64) - want)
    lim = bound(forest, X, rows, trees, weights, stop)
    bad = err > lim
    assert not bad.any(), f"{int(bad.sum())} outputs past the bound, worst err / bound {(err[bad] / lim[bad]).max()}"


# ------------------------------------------------------------------------------------------------ generators
def exact_values(rng, n, K):
    v = (rng.integers(-64, 65, (n, K)) / 16.0).astype(np.float32)
    assert np.array_equal(v * 16, np.rint(v * 16)) and np.abs(v).max() <= 4
    return v


def exact_weights(rng, T):
    """Multiples of 1/4 in (0, 2]; with :func:`exact_values` any sum of at most ``EXACT_MAX_TREES`` products is a
    multiple of 1/64 below 2^10, hence exact in fp32 (asserted)."""
    assert T <= EXACT_MAX_TREES and EXACT_MAX_TREES * 4 * 2 < 2 ** 10
    w = (rng.integers(1, 9, T) / 4.0).astype(np.float32)
    assert np.array_equal(w * 4, np.rint(w * 4)) and w.min() > 0 and w.max() <= 2
    return w


def rounded_values(rng, n, K):
    return (rng.standard_normal((n, K)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)


def rounded_weights(rng, T):
    return (rng.standard_normal(T) * 1.5).astype(np.float32)


def check_forest(f, F, B):
    """Every index a predictor follows is in range: no input built here can send a kernel out of bounds."""
    T = f.n_trees
    off = np.asarray(f.tree_off, np.int64)
    n = len(f.nodes)
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 1).all()
    assert f.nodes.dtype == np.int32 and f.nodes.shape == (n, 4) and f.value.dtype == np.float32
    assert f.value.shape[0] == n and f.default_left.shape == (n,) and f.gain.shape == (n,) and len(f.tree_model) == T
    assert f.missing_bin < B
    tree = np.repeat(np.arange(T), np.diff(off))
    internal = f.nodes[:, 2] >= 0
    assert (f.nodes[~internal, 3] < 0).all()
    nd = f.nodes[internal].astype(np.int64)
    assert (nd[:, 0] >= 0).all() and (nd[:, 0] < F).all() and (nd[:, 1] >= 0).all() and (nd[:, 1] < B).all()
    me = np.nonzero(internal)[0]
    for c in (nd[:, 2], nd[:, 3]):
        assert (c > me).all() and (c < off[tree[me] + 1]).all()         # BFS: children after the parent, in the tree
    kids = np.sort(np.concatenate([nd[:, 2], nd[:, 3]]))
    assert np.array_equal(kids, np.setdiff1d(np.arange(n), off[:-1]))    # every non-root node has exactly one parent


def _assemble(parts, K, values, missing_bin, tree_model):
    """``parts``: per tree (feat, bin, left, right, default_left, gain) with tree-local children -> Forest."""
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in parts])
    nodes = np.zeros((int(off[-1]), 4), np.int32)
    dl = np.zeros(int(off[-1]), np.uint8)
    gain = np.zeros(int(off[-1]), np.float32)
    for t, (feat, sbin, left, right, d, g) in enumerate(parts):
        a, b = int(off[t]), int(off[t + 1])
        leaf = np.asarray(left) < 0
        nodes[a:b, 0] = np.where(leaf, 0, feat)
        nodes[a:b, 1] = np.where(leaf, 0, sbin)
        nodes[a:b, 2] = np.where(leaf, -1, np.asarray(left) + a)
        nodes[a:b, 3] = np.where(leaf, -1, np.asarray(right) + a)
        dl[a:b] = np.where(leaf, 0, d)
        gain[a:b] = np.where(leaf, 0, g)
    value = np.ascontiguousarray(values(int(off[-1]), K), np.float32)
    tm = np.zeros(len(parts), np.int32) if tree_model is None else np.asarray(tree_model, np.int32)
    return Forest(off, nodes, dl, value, gain, np.ones(int(off[-1]), np.float32), tm, missing_bin)


def _random_tree(rng, n_split, F, B, X):
    """A tree of ``n_split`` splits (``2 n_split + 1`` nodes) grown by splitting a random leaf each time, renumbered in
    BFS order. Half the split bins are the bin of a random row of ``X`` in the split column, so rows sit on the
    ``bin == split_bin`` edge; the rest are uniform in [0, B)."""
    kids = {0: None}
    leaves = [0]
    nxt = 1
    for _ in range(n_split):
        k = leaves.pop(int(rng.integers(len(leaves))))
        kids[k] = (nxt, nxt + 1)
        kids[nxt] = kids[nxt + 1] = None
        leaves += [nxt, nxt + 1]
        nxt += 2
    order, new = [0], {0: 0}
    for k in order:                                     # BFS
        if kids[k] is not None:
            for c in kids[k]:
                new[c] = len(order)
                order.append(c)
    n = len(order)
    left = np.array([-1 if kids[k] is None else new[kids[k][0]] for k in order], np.int64)
    right = np.array([-1 if kids[k] is None else new[kids[k][1]] for k in order], np.int64)
    feat = rng.integers(0, F, n)
    sbin = rng.integers(0, B, n)
    if X is not None and len(X):
        hit = rng.random(n) < 0.5
        sbin = np.where(hit, X[rng.integers(0, len(X), n), feat], sbin)
    gain = (rng.random(n) * 0.98 + 0.01).astype(np.float32)
    return feat, sbin, left, right, rng.integers(0, 2, n), gain


def random_forest(rng, T, F, B, K, *, budget=9, single_leaf=(), missing_bin=-1, X=None, values=None,
                  tree_model=None):
    """``T`` hand-built trees over ``F`` columns of bins in [0, B). ``budget`` (an int or one per tree) is the node
    budget of a tree: it gets ``(budget - 1) // 2`` splits whatever depth that gives; trees listed in ``single_leaf``
    are one leaf. ``values(n, K)`` makes the node values (every node has one, as the grower records them): default
    :func:`exact_values`. Internal gains are distinct-ish fp32 in (0, 1); ``default_left`` takes both values."""
    budget = [budget] * T if np.isscalar(budget) else list(budget)
    assert len(budget) == T
    parts = [_random_tree(rng, 0 if t in single_leaf else (int(budget[t]) - 1) // 2, F, B, X) for t in range(T)]
    f = _assemble(parts, K, values or (lambda n, k: exact_values(rng, n, k)), missing_bin, tree_model)
    check_forest(f, F, B)
    assert all(f.tree_off[t + 1] - f.tree_off[t] <= max(1, budget[t]) for t in range(T))
    return f


def chain_tree(rng, depth, F, B, K, *, missing_bin=-1, values=None):
    """One tree that is a spine of ``depth`` splits (depth <= 40) with one leaf off each spine node: the spine goes on
    to the left child at even depths and to the right child at odd ones; spine node ``d`` splits column ``d`` at bin
    ``B // 2 - 1``. ``2 depth + 1`` nodes. :func:`chain_rows` makes rows that leave the spine at every depth."""
    assert 1 <= depth <= 40 and F >= depth and B >= 2
    n = 2 * depth + 1
    feat, sbin = np.zeros(n, np.int64), np.full(n, B // 2 - 1, np.int64)
    left, right = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    k = 0                                              # BFS: level d >= 1 holds nodes 2d - 1 (left) and 2d (right)
    for d in range(depth):
        feat[k] = d
        left[k], right[k] = 2 * d + 1, 2 * d + 2
        k = left[k] if d % 2 == 0 else right[k]
    gain = (rng.random(n) * 0.98 + 0.01).astype(np.float32)
    f = _assemble([(feat, sbin, left, right, rng.integers(0, 2, n), gain)], K,
                  values or (lambda m, k_: exact_values(rng, m, k_)), missing_bin, None)
    check_forest(f, F, B)
    return f


def chain_rows(rng, depth, F, B, n, hi=None):
    """uint8 ``[n, F]`` rows for :func:`chain_tree`: row ``i`` follows the spine for ``i % (depth + 1)`` steps and then
    leaves it (or reaches the bottom); bins equal to the split bin occur. ``hi``: largest bin drawn (default B - 1)."""
    hi = B - 1 if hi is None else hi
    s = B // 2 - 1
    X = rng.integers(0, hi + 1, (n, F))
    for i in range(n):
        e = i % (depth + 1)
        for d in range(min(e + 1, depth)):
            on_spine = d < e
            go_left = (d % 2 == 0) == on_spine
            X[i, d] = (s if rng.random() < 0.3 else rng.integers(0, s + 1)) if go_left else rng.integers(s + 1, hi + 1)
    return X.astype(np.uint8)


def random_bins(rng, n, F, B, missing_bin=-1, p_missing=0.15):
    """uint8 ``[n, F]`` bins in [0, B) (B - 1 included: 255 at B = 256); with a missing bin, a share of entries hold it."""
    X = rng.integers(0, B, (n, F))
    if missing_bin >= 0:
        X = np.where(rng.random((n, F)) < p_missing, missing_bin, X)
    return X.astype(np.uint8)
