"""The NumPy oracle of forest prediction (tests/forest_predict_oracle.py) against the host twin
``tmog_forest_predict_cpu`` (through ``tree_engine.forest_predict`` on CPU tensors), ``prune_forest`` and the CPU
fallback of ``forest_predict_multi``, on hand-built forests. No GPU needed; this agreement is what entitles the oracle
to judge the HIP kernels (tests/test_forest_predict_kernels_gpu.py). Exact-regime cases are bit-equal, rounded-regime
cases within the oracle's per-output summation bound."""
import numpy as np
import pytest
import torch

import forest_predict_oracle as O
from transmogrifai_amd.models import tree_engine as te


def _t(rows):
    return None if rows is None else torch.as_tensor(np.asarray(rows, np.int64))


def _predict(f, X, model_rows, model_trees, w=None):
    out = te.forest_predict(f, torch.from_numpy(X), [_t(r) for r in model_rows], model_trees, w)
    return [o.numpy() for o in out]


def _check(f, X, model_rows, model_trees, w=None, exact=True):
    got = _predict(f, X, model_rows, model_trees, w)
    assert len(got) == len(model_rows)
    for g, rows, trees in zip(got, model_rows, model_trees):
        O.assert_matches(g, f, X, rows, trees, w, exact=exact)


# ------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_on_a_tree_written_out_by_hand():
    """Root splits column 1 at bin 2 (default right); its left child splits column 0 at bin 0 (default left)."""
    nodes = np.array([[1, 2, 1, 2], [0, 0, 3, 4], [0, 0, -1, -1], [0, 0, -1, -1], [0, 0, -1, -1]], np.int32)
    val = np.array([[9], [8], [1], [2], [4]], np.float32)
    f = te.Forest(np.array([0, 5], np.int64), nodes, np.array([0, 1, 0, 0, 0], np.uint8), val,
                  np.array([.5, .25, 0, 0, 0], np.float32), np.ones(5, np.float32), np.zeros(1, np.int32), 3)
    O.check_forest(f, 2, 4)
    X = np.array([[0, 2], [1, 2], [0, 1], [3, 0], [0, 3], [1, 3]], np.uint8)
    #        bin == split -> left twice; 1 > 0 -> right; missing col 0 -> default left; missing col 1 -> default right
    assert O.walk(f, X, None, [0])[:, 0].tolist() == [2, 4, 2, 2, 1, 1]
    f.missing_bin = -1                                  # bin 3 is an ordinary bin now: 3 > 2 right, 3 > 0 right
    assert O.walk(f, X, None, [0])[:, 0].tolist() == [2, 4, 2, 4, 1, 1]
    assert O.walk(f, X, [5, 0, 0], [0, 0], [0.5])[:, 0].tolist() == [1, 2, 2]
    assert O.walk(f, X, None, [0], stop=O.variant_stop(f, 1, 0.0))[:, 0].tolist() == [8, 8, 8, 8, 1, 1]
    assert O.walk(f, X, None, [0], stop=O.variant_stop(f, 5, 0.25))[:, 0].tolist() == [2, 4, 2, 4, 1, 1]
    assert O.walk(f, X, None, [0], stop=O.variant_stop(f, 5, 0.26))[:, 0].tolist() == [8, 8, 8, 8, 1, 1]
    assert O.walk(f, X, None, [0], stop=O.variant_stop(f, 0, 0.0))[:, 0].tolist() == [9] * 6
    assert O.bound(f, X, [1], [0, 0], [2.0])[0, 0] == 4 * 2.0 ** -24 * 16
    assert O.walk(f, X, [], [0]).shape == (0, 1)


def test_generators_keep_their_promises():
    rng = np.random.default_rng(0)
    X = O.random_bins(rng, 200, 6, 16, 15)
    f = O.random_forest(rng, 7, 6, 16, 3, budget=[1, 3, 4, 41, 9, 9, 201], single_leaf=(4,), missing_bin=15, X=X)
    assert np.diff(f.tree_off).tolist() == [1, 3, 3, 41, 1, 9, 201]
    internal = f.nodes[:, 2] >= 0
    assert set(f.default_left[internal].tolist()) == {0, 1}
    nd = f.nodes[internal]
    assert (X[:, nd[:, 0]] == nd[:, 1][None, :]).any(0).mean() > 0.4            # rows on the bin == split_bin edge
    assert (X == 15).any() and (O.reach(f, X, None, [6]) != f.tree_off[6]).all()
    c = O.chain_tree(rng, 40, 40, 8, 2)
    Xc = O.chain_rows(rng, 40, 40, 8, 82)
    depth_of = np.zeros(81, np.int64)
    for k in range(81):
        if c.nodes[k, 2] >= 0:
            depth_of[c.nodes[k, 2:]] = depth_of[k] + 1
    assert np.array_equal(np.sort(depth_of[O.reach(c, Xc, None, [0])[:, 0]]), np.sort(np.minimum(np.arange(82) % 41 + 1, 40)))
    assert np.array_equal(te._node_depth(c), depth_of)        # what forest_predict_multi folds deep variants with
    assert te._node_depth(f)[f.tree_off[:-1]].tolist() == [0] * 7
    w = O.exact_weights(rng, O.EXACT_MAX_TREES)
    v = O.exact_values(rng, O.EXACT_MAX_TREES, 1)[:, 0]
    for order in (np.arange(80), rng.permutation(80)):
        assert float(np.cumsum((w * v)[order], dtype=np.float32)[-1]) == float((w.astype(np.float64) * v).sum())
    with pytest.raises(AssertionError):
        O.exact_weights(rng, O.EXACT_MAX_TREES + 1)


# ------------------------------------------------------------------------------------------------ host twin
def _mixed_case(seed, K, missing_bin, exact):
    """13 trees, two of them single leaves, one of 201 nodes; three models with a shuffled row list with repeats, an
    empty one and all rows; weights on."""
    rng = np.random.default_rng(seed)
    B, F, n = 8, 9, 301
    X = O.random_bins(rng, n, F, B, missing_bin)
    values = None if exact else (lambda m, k: O.rounded_values(rng, m, k))
    f = O.random_forest(rng, 13, F, B, K, budget=[9, 1, 31, 3, 201, 9, 15, 9, 1, 9, 63, 5, 9], single_leaf=(7,),
                        missing_bin=missing_bin, X=X, values=values)
    w = O.exact_weights(rng, 13) if exact else O.rounded_weights(rng, 13)
    rows = [rng.integers(0, n, 400), np.zeros(0, np.int64), None]
    trees = [[0, 1, 2, 3, 4], [5, 6], [12, 7, 8, 9, 10, 11, 4]]
    return f, X, rows, trees, w


@pytest.mark.parametrize("missing_bin", [-1, 7], ids=["nomissing", "missing"])
@pytest.mark.parametrize("K", [1, 2, 3, 11])
def test_exact_regime_equals_cpu_twin(K, missing_bin):
    f, X, rows, trees, w = _mixed_case(10 * K + missing_bin, K, missing_bin, True)
    _check(f, X, rows, trees, w)
    _check(f, X, rows[::-1], trees[::-1], None)                 # the empty model in the middle, no weights
    assert len(np.unique(O.walk(f, X, None, trees[2], w))) > 50


@pytest.mark.parametrize("missing_bin", [-1, 7], ids=["nomissing", "missing"])
@pytest.mark.parametrize("K", [1, 2, 3, 11])
def test_rounded_regime_within_bound_of_cpu_twin(K, missing_bin):
    f, X, rows, trees, w = _mixed_case(100 + 10 * K + missing_bin, K, missing_bin, False)
    _check(f, X, rows, trees, w, exact=False)
    _check(f, X, rows, trees, None, exact=False)


@pytest.mark.parametrize("n_models", [1, 3])
def test_all_rows_of_every_model(n_models):
    """``model_rows`` all None: one model walks ``row = i - r0``, three use the wrapper's replicated arange."""
    rng = np.random.default_rng(n_models)
    X = O.random_bins(rng, 130, 5, 32, 31)
    f = O.random_forest(rng, 6, 5, 32, 2, budget=15, single_leaf=(0,), missing_bin=31, X=X)
    w = O.exact_weights(rng, 6)
    trees = [[0, 1, 2, 3, 4, 5]] if n_models == 1 else [[0, 1], [2], [5, 4, 3]]
    _check(f, X, [None] * n_models, trees, w)


def test_bin_255_without_a_missing_bin_is_an_ordinary_bin():
    rng = np.random.default_rng(5)
    X = O.random_bins(rng, 400, 4, 256)
    X[::3, :2] = 255
    f = O.random_forest(rng, 5, 4, 256, 1, budget=41, X=X)
    f.nodes[f.tree_off[:-1], 1] = [255, 254, 0, 255, 128]       # roots split at the last bins and at bin 0
    O.check_forest(f, 4, 256)
    _check(f, X, [None], [[0, 1, 2, 3, 4]])


@pytest.mark.parametrize("missing_bin", [-1, 7], ids=["nomissing", "missing"])
def test_depth_40_chain_and_single_leaf_trees(missing_bin):
    rng = np.random.default_rng(40 + missing_bin)
    chain = O.chain_tree(rng, 40, 40, 8, 3, missing_bin=missing_bin)
    leafs = O.random_forest(rng, 2, 40, 8, 3, single_leaf=(0, 1), missing_bin=missing_bin)
    f = te.Forest.concat([leafs.tree(0), chain, leafs.tree(1)])
    O.check_forest(f, 40, 8)
    X = O.chain_rows(rng, 40, 40, 8, 123, hi=6)
    if missing_bin >= 0:
        X[rng.random(X.shape) < 0.02] = missing_bin
    assert len(np.unique(O.reach(f, X, None, [1]))) >= 30
    _check(f, X, [None, np.arange(122, -1, -1)], [[0, 1, 2], [1]], O.exact_weights(rng, 3))
    _check(f, X, [None], [[0, 2]])                               # a model of single leaves only


# ------------------------------------------------------------------------------------------- pruned variants
def _variant_case(seed, K, exact=True):
    rng = np.random.default_rng(seed)
    B, F, n = 16, 48, 211
    X = O.random_bins(rng, n, F, B, 15)
    X[:82] = O.chain_rows(rng, 40, F, B, 82, hi=14)
    values = None if exact else (lambda m, k: O.rounded_values(rng, m, k))
    body = O.random_forest(rng, 6, F, B, K, budget=[63, 1, 9, 127, 31, 3], missing_bin=15, X=X, values=values)
    chain = O.chain_tree(rng, 40, F, B, K, missing_bin=15, values=values)
    f = te.Forest.concat([body, chain])
    O.check_forest(f, F, B)
    return rng, f, X


def _variants(f):
    stored = float(f.gain[f.tree_off[3]])     # a stored fp32 gain, of a root every row visits: it must stay split
    above = float(np.nextafter(np.float32(stored), np.float32(2)))
    return [(0, 0.0), (3, 0.3), (40, 0.0), (64, 2.0), (64, stored), (64, above), (5, stored), (1, 0.0), (33, 0.0)]


@pytest.mark.parametrize("K", [1, 3])
def test_stop_rule_equals_prune_forest(K):
    """``walk`` with ``variant_stop`` on the grown forest equals ``forest_predict`` of ``prune_forest``'s forest:
    depth 0 (every root), mid-range, the full depth-40 chain, a min gain above every gain, and a min gain equal to a
    stored gain (kept: ``>=``) next to one ulp above it (cut)."""
    rng, f, X = _variant_case(K, K)
    trees = list(range(f.n_trees))
    full = O.walk(f, X, None, trees)
    seen = []
    for d, g in _variants(f):
        stop = O.variant_stop(f, d, g)
        p = te.prune_forest(f, d, g)
        O.check_forest(p, 48, 16)
        got = _predict(p, X, [None], [trees])[0]
        O.assert_matches(got, f, X, None, trees, stop=stop)
        O.assert_matches(got, p, X, None, trees)
        seen.append(O.walk(f, X, None, trees, stop=stop))
    assert np.array_equal(seen[2], full) and not np.array_equal(seen[8], full)      # depth 33 cuts the chain, 40 not
    assert np.array_equal(seen[0], np.broadcast_to(f.value[f.tree_off[:-1]].astype(np.float64).sum(0), full.shape))
    assert np.array_equal(seen[3], seen[0]) and not np.array_equal(seen[4], seen[5])
    assert te.prune_forest(f, 64, _variants(f)[4][1]).nodes.shape[0] > te.prune_forest(f, 64, _variants(f)[5][1]).nodes.shape[0]


@pytest.mark.parametrize("K,exact", [(1, True), (2, True), (3, True), (4, False), (8, True)])
def test_multi_cpu_fallback_equals_oracle(K, exact):
    rng, f, X = _variant_case(50 + K, K, exact)
    vs = _variants(f)
    rows = [None, rng.integers(0, len(X), 97), np.zeros(0, np.int64)]
    trees = [[0, 1, 2, 6], [3, 4, 5, 6, 1], [2]]
    variants = [vs, vs[1:4], vs[:2]]
    got = te.forest_predict_multi(f, torch.from_numpy(X), [_t(r) for r in rows], trees, variants)
    assert [len(g) for g in got] == [len(v) for v in variants]
    for m in range(3):
        for o, (d, g) in zip(got[m], variants[m]):
            O.assert_matches(o.numpy(), f, X, rows[m], trees[m], stop=O.variant_stop(f, d, g), exact=exact)
