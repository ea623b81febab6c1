"""Brute-force path-dependent TreeSHAP, straight from its definition, on the ``Forest`` node arrays (NumPy only).

For one tree, a row ``x`` and a feature subset ``S``: walk from the root; at a node whose feature is in ``S``
follow the branch ``x`` takes (``b == missing_bin ? default_left : b <= split_bin``), at any other node take
both children with weights ``cover[child] / cover[node]`` (both 0 when ``cover[node] == 0``). ``g(S)`` is the
weighted sum of the leaf values reached, ``phi_i`` the Shapley value of feature ``i`` in ``g``, the bias
``g(empty)``; a forest's attribution is the ``tree_weight``-weighted sum over its trees, tree ``t`` writing
columns ``tree_out[t] ..``. ``g`` is evaluated for all ``2^U`` subsets at once as a bitmask vector. No path
merging; shares no code with the implementation. Also builds the hand-made forests of the SHAP tests."""
import math

import numpy as np

from transmogrifai_amd.models.tree_engine import Forest


def used_features(forest):
    return np.unique(forest.nodes[forest.nodes[:, 2] >= 0, 0]).astype(np.int64)


def magnitude(forest, tree_weight=None):
    """``S = sum_t |w_t| max_node |value_t|``: the scale every tolerance is stated in."""
    w = np.ones(forest.n_trees) if tree_weight is None else np.asarray(tree_weight, np.float64)
    return float(sum(abs(w[t]) * np.abs(forest.value[int(forest.tree_off[t]):int(forest.tree_off[t + 1])]).max()
                     for t in range(forest.n_trees)))


def _game(forest, t, xrow, used, masks):
    """``g(S)`` of tree ``t`` for every subset mask: float64 [2^U, K]."""
    pos = {int(f): u for u, f in enumerate(used)}
    nd, cov = forest.nodes, forest.cover.astype(np.float64)
    g = np.zeros((masks.size, forest.K))
    stack = [(int(forest.tree_off[t]), np.ones(masks.size))]
    while stack:
        k, wgt = stack.pop()
        f, sb, lc, rc = (int(v) for v in nd[k])
        if lc < 0:
            g += wgt[:, None] * forest.value[k].astype(np.float64)[None, :]
            continue
        b = int(xrow[f])
        left = bool(forest.default_left[k]) if (forest.missing_bin >= 0 and b == forest.missing_bin) else b <= sb
        ins = ((masks >> pos[f]) & 1).astype(bool)
        for child, is_left in ((lc, True), (rc, False)):
            ratio = cov[child] / cov[k] if cov[k] != 0 else 0.0
            stack.append((child, wgt * np.where(ins, 1.0 if left == is_left else 0.0, ratio)))
    return g


def shap_oracle(forest, Xb, rows=None, tree_weight=None, tree_out=None, n_out=None):
    """``(phi float64 [n, U + 1, C], used int64 [U])`` by enumeration of all feature subsets (U <= ~17)."""
    Xb = np.asarray(Xb)
    rows = np.arange(Xb.shape[0]) if rows is None else np.asarray(rows)
    T, K = forest.n_trees, forest.K
    w = np.ones(T) if tree_weight is None else np.asarray(tree_weight, np.float64)
    tout = np.zeros(T, np.int64) if tree_out is None else np.asarray(tree_out, np.int64)
    C = int(n_out) if n_out is not None else (int(tout.max()) if T else 0) + K
    used = used_features(forest)
    U = used.size
    masks = np.arange(1 << U, dtype=np.int64)
    pop = np.zeros(masks.size, np.int64)
    for u in range(U):
        pop += (masks >> u) & 1
    fact = [math.factorial(i) for i in range(U + 1)]
    phi = np.zeros((rows.size, U + 1, C))
    for i, r in enumerate(rows):
        g = np.zeros((masks.size, C))
        for t in range(T):
            g[:, tout[t]:tout[t] + K] += w[t] * _game(forest, t, Xb[r], used, masks)
        phi[i, U] = g[0]
        for u in range(U):
            without = masks[((masks >> u) & 1) == 0]
            sw = np.asarray([fact[s] * fact[U - s - 1] / fact[U] for s in range(U)])[pop[without]]
            phi[i, u] = (sw[:, None] * (g[without | (1 << u)] - g[without])).sum(0)
    return phi, used


_CASES = {}


def case(name):
    """``(forest, Xb uint8 [n, F], kwargs of forest_shap, oracle phi)`` of a named hand-built case; the oracle
    runs once per process and is shared by the CPU and the GPU tests."""
    if name not in _CASES:
        forest, Xb, kw = _build_case(name)
        _CASES[name] = (forest, Xb, kw, shap_oracle(forest, Xb, **kw)[0])
    return _CASES[name]


CASES = ["rf_k1", "rf_k3", "rf_tree_out", "rf_no_missing", "stump", "lone_leaf", "zero_cover", "dl_disagree",
         "chain15", "chain16", "chain17"]


def _build_case(name):
    if name.startswith("rf_"):
        Xb = random_bins(1, 12)
        kw = dict(tree_weight=np.linspace(0.3, -1.7, 7), rows=np.asarray([0, 3, 11, 5, 5, 8]))
        if name == "rf_k1":
            return random_forest(6, K=1), Xb, kw
        if name == "rf_k3":
            return random_forest(8, K=3), Xb, kw
        if name == "rf_tree_out":
            return random_forest(9, K=1), Xb, dict(kw, tree_out=np.arange(7) % 3)
        return random_forest(10, K=1, missing_bin=-1), Xb, kw
    if name == "stump":
        return stump(), np.asarray([[0, 0, 4, 0]], np.uint8), {}
    if name == "lone_leaf":
        return lone_leaf(), np.zeros((2, 3), np.uint8), {}
    if name == "zero_cover":
        # rows: left at the root; into the zero-cover leaf; beside it (both inner branches); missing_bin = -1
        return zero_cover_forest(), np.asarray([[0, 0], [5, 7], [3, 2], [7, 1]], np.uint8), {}
    if name == "dl_disagree":
        # bin 7 is the missing bin: rows with feature 1 missing, feature 3 missing, both, none
        return default_left_disagree_forest(), np.asarray([[0, 7, 0, 0], [0, 4, 0, 7], [0, 7, 0, 7], [0, 3, 0, 1],
                                                           [0, 6, 0, 2]], np.uint8), {}
    m = int(name[len("chain"):])
    return chain_forest(m, seed=m), np.random.default_rng(m).integers(0, 2, size=(4, m)).astype(np.uint8), {}


# --------------------------------------------------------------------------------- hand-built forests
def _assemble(trees, K, missing_bin):
    """``trees``: per tree a list of dict nodes (feat, bin, left, right, dl, value, cover) with local children."""
    off, nodes, dl, val, cov = [0], [], [], [], []
    for tr in trees:
        base = off[-1]
        for nd in tr:
            leaf = nd["left"] < 0
            nodes.append([0 if leaf else nd["feat"], 0 if leaf else nd["bin"],
                          -1 if leaf else nd["left"] + base, -1 if leaf else nd["right"] + base])
            dl.append(0 if leaf else nd["dl"])
            val.append(nd["value"])
            cov.append(nd["cover"])
        off.append(base + len(tr))
    n = len(nodes)
    return Forest(np.asarray(off, np.int64), np.asarray(nodes, np.int32).reshape(n, 4), np.asarray(dl, np.uint8),
                  np.asarray(val, np.float32).reshape(n, K), np.zeros(n, np.float32), np.asarray(cov, np.float32),
                  np.zeros(len(trees), np.int32), missing_bin)


def random_forest(seed, T=7, depth=6, F=9, n_used=8, B=8, K=1, missing_bin=7):
    """Random trees of depth <= ``depth`` over ``n_used`` of ``F`` columns. A child repeats an ancestor's
    feature with probability 1/2 (with a random threshold, so same-direction and contradictory repeats both
    occur). Covers are integers: the root has 16^depth and every split sends k/16 of it left, k in 1..15,
    so every cover ratio is >= 1/16 and exact in fp32."""
    rng = np.random.default_rng(seed)
    feats = rng.permutation(F)[:n_used]
    hi_bin = B - 2 if missing_bin >= 0 else B - 1
    trees = []
    for _ in range(T):
        tr = []

        def grow(d, cover, anc):
            i = len(tr)
            tr.append(None)
            value = rng.normal(size=K)
            if d == depth or (d > 0 and rng.random() < 0.2):
                tr[i] = dict(left=-1, value=value, cover=cover)
                return i
            f = int(rng.choice(anc)) if anc and rng.random() < 0.5 else int(rng.choice(feats))
            k = int(rng.integers(1, 16))
            lc = grow(d + 1, cover * k // 16, anc + [f])
            rc = grow(d + 1, cover - cover * k // 16, anc + [f])
            tr[i] = dict(feat=f, bin=int(rng.integers(0, hi_bin)), left=lc, right=rc, dl=int(rng.integers(0, 2)),
                         value=value, cover=cover)
            return i

        grow(0, 16 ** depth, [])
        trees.append(tr)
    return _assemble(trees, K, missing_bin)


def random_bins(seed, n, F=9, B=8):
    """Bins 0 .. B-1 (the last is the missing bin of ``random_forest``)."""
    return np.random.default_rng(seed).integers(0, B, size=(n, F)).astype(np.uint8)


def chain_forest(m, seed=0, equal=False, K=1, missing_bin=-1):
    """One tree that is a chain over ``m`` distinct features 0 .. m-1: node ``d`` splits feature ``d`` at
    bin 0, its left child is a leaf and its right child the next node, so the deepest leaf's path has ``m``
    elements. ``equal``: every split halves its cover and only the deepest leaf has a non-zero value, which
    makes the features interchangeable for a row that goes right everywhere."""
    rng = np.random.default_rng(seed)
    tr = []
    cover = float(2 ** m) if equal else float(2 ** 20)
    for d in range(m):
        frac = 0.5 if equal else float(rng.integers(1, 16)) / 16.0
        # internal node 2d, its leaf child 2d + 1, the next internal node (or the deepest leaf) 2d + 2
        tr.append(dict(feat=d, bin=0, left=2 * d + 1, right=2 * d + 2, dl=int(rng.integers(0, 2)),
                       value=rng.normal(size=K), cover=cover))
        tr.append(dict(left=-1, value=np.zeros(K) if equal else rng.normal(size=K), cover=cover * frac))
        cover = cover * (1.0 - frac)
    tr.append(dict(left=-1, value=np.ones(K) if equal else rng.normal(size=K), cover=cover))
    return _assemble([tr], K, missing_bin)


def stump(K=1, missing_bin=-1):
    return _assemble([[dict(feat=2, bin=3, left=1, right=2, dl=1, value=np.zeros(K), cover=10.0),
                       dict(left=-1, value=np.full(K, -1.5), cover=4.0),
                       dict(left=-1, value=np.full(K, 2.25), cover=6.0)]], K, missing_bin)


def lone_leaf(K=1):
    return _assemble([[dict(left=-1, value=np.full(K, 0.75), cover=5.0)]], K, -1)


def zero_cover_forest():
    """Feature 0 at the root; its right child splits feature 1 with a zero-cover right leaf (and the right
    child's own left subtree splits feature 0 again)."""
    tr = [dict(feat=0, bin=2, left=1, right=2, dl=0, value=[0.0], cover=8.0),
          dict(left=-1, value=[1.0], cover=3.0),
          dict(feat=1, bin=4, left=3, right=4, dl=1, value=[0.0], cover=5.0),
          dict(feat=0, bin=5, left=5, right=6, dl=1, value=[0.0], cover=5.0),
          dict(left=-1, value=[-3.0], cover=0.0),
          dict(left=-1, value=[2.0], cover=2.0),
          dict(left=-1, value=[0.5], cover=3.0)]
    return _assemble([tr], 1, -1)


def default_left_disagree_forest():
    """Feature 1 twice on the path root -> right -> left, the two nodes disagreeing on ``default_left``:
    a missing-bin row (bin 7) leaves that path at the second node although its merged interval is not
    empty."""
    tr = [dict(feat=1, bin=2, left=1, right=2, dl=0, value=[0.0], cover=16.0),
          dict(left=-1, value=[1.0], cover=6.0),
          dict(feat=1, bin=5, left=3, right=4, dl=0, value=[0.0], cover=10.0),
          dict(feat=3, bin=1, left=5, right=6, dl=1, value=[0.0], cover=4.0),
          dict(left=-1, value=[-2.0], cover=6.0),
          dict(left=-1, value=[4.0], cover=1.0),
          dict(left=-1, value=[-1.0], cover=3.0)]
    tr2 = [dict(feat=1, bin=2, left=1, right=2, dl=0, value=[0.0], cover=16.0),
           dict(left=-1, value=[0.5], cover=6.0),
           dict(feat=1, bin=5, left=3, right=4, dl=1, value=[0.0], cover=10.0),
           dict(left=-1, value=[3.0], cover=4.0),
           dict(left=-1, value=[-0.25], cover=6.0)]
    return _assemble([tr, tr2], 1, 7)
