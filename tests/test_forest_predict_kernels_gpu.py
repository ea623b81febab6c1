"""Kernel-level oracle tests of the forest scoring kernels in ``ops/csrc/hip/forest_predict_kernels.hip``:
``forest_predict_lds_kernel<NS>`` (F <= 512), ``forest_predict_kernel<NS>`` (the F > 512 fallback) and
``forest_predict_multi_kernel<NS, 1|2|4|8, VKP>``, each over both node sources ``NS`` (``ImageNodes``, the packed node
image, and ``DirectNodes``, which ``TMOG_PREDICT_V1=1`` selects: the autouse fixture ``node_source`` patches
``tree_engine.predict_v1``), on hand-built forests (tests/forest_predict_oracle.py, validated against the
host twin in tests/test_forest_predict_oracle.py). Each case is named after the path it forces. Exact-regime cases
compare with equality, rounded-regime cases with the oracle's per-output bound ``(T + 2) 2^-24 sum |w v|``; the
write-guard cases go through the direct C entry points with sentinel-filled buffers, whatever the fixture says, so
they run once."""
import types

import numpy as np
import pytest
import torch

import forest_predict_oracle as O
from transmogrifai_amd.models import tree_engine as te
from transmogrifai_amd.ops._native import ABI_CONSTS

PM_VK = ABI_CONSTS["TMOG_PM_VK"]
SENT = np.float32(-1.5e30)


DIRECT = "_direct_source"      # suffix of the copies at the end of the module that run on the direct node source


@pytest.fixture(autouse=True)
def node_source(request, monkeypatch):
    """Every oracle case of the module runs on both node sources, switched the way ``TMOG_PREDICT_V1`` does: under its
    own name on the image, and as ``<name>_direct_source`` (made at the end of the module) on the direct source."""
    source = "direct" if request.node.originalname.endswith(DIRECT) else "image"
    monkeypatch.setattr(te, "predict_v1", lambda: source == "direct")
    return source


def _loaded():
    from transmogrifai_amd.ops import _native
    return _native.hip_loaded()


def _lib():
    from transmogrifai_amd.ops import _native
    return _native.hip()


def _st():
    from transmogrifai_amd.ops import _native
    return _native.stream()


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _t(rows):
    return None if rows is None else torch.as_tensor(np.asarray(rows, np.int64)).cuda()


def _case(seed, F, n, tpm, *, K=1, B=16, missing=True, exact=True, budgets=(1, 3, 7, 15, 31), single_leaf=()):
    """Rows, a forest of ``sum(tpm)`` trees dealt to the models in a shuffled order, per-tree weights."""
    rng = np.random.default_rng(seed)
    mb = B - 1 if missing else -1
    X = O.random_bins(rng, n, F, B, mb)
    T = int(sum(tpm))
    values = None if exact else (lambda m, k: O.rounded_values(rng, m, k))
    f = O.random_forest(rng, T, F, B, K, budget=rng.choice(budgets, T), single_leaf=single_leaf, missing_bin=mb, X=X,
                        values=values)
    w = O.exact_weights(rng, T) if exact else O.rounded_weights(rng, T)
    perm = rng.permutation(T)
    cuts = np.cumsum([0] + list(tpm))
    trees = [perm[cuts[m]:cuts[m + 1]].tolist() for m in range(len(tpm))]
    return rng, f, X, trees, w


def _check(f, X, model_rows, model_trees, w=None, exact=True):
    got = te.forest_predict(f, _d(X), [_t(r) for r in model_rows], model_trees, w)
    torch.cuda.synchronize()
    assert len(got) == len(model_rows)
    for g, rows, trees in zip(got, model_rows, model_trees):
        O.assert_matches(g.cpu().numpy(), f, X, rows, trees, w, exact=exact)


def _check_multi(f, X, model_rows, model_trees, variants, exact=True, F_fallback=False):
    assert F_fallback == (te._pm_lds_bytes(X.shape[1]) > te._lds_limit(None))
    assert all(len(v) * f.K <= PM_VK for v in variants) and f.K in (1, 2, 4, 8)      # the kernel, not the fallback
    got = te.forest_predict_multi(f, _d(X), [_t(r) for r in model_rows], model_trees, variants)
    torch.cuda.synchronize()
    assert [len(g) for g in got] == [len(v) for v in variants]
    for m, vs in enumerate(variants):
        for o, (d, g) in zip(got[m], vs):
            O.assert_matches(o.cpu().numpy(), f, X, model_rows[m], model_trees[m], stop=O.variant_stop(f, d, g),
                             exact=exact)


# =================================================================== forest_predict_kernel (128 F > 64 KiB: F > 512)
FB_F = 520


@pytest.mark.gpu
@pytest.mark.parametrize("n_trees,trips,tail", [(1, 0, 1), (3, 0, 3), (4, 1, 0), (5, 1, 1), (8, 2, 0), (11, 2, 3)],
                         ids=lambda v: str(v))
def test_fallback_interleaved_trips_and_tail(n_trees, trips, tail):
    """F = 520 -> 128 * 520 > 65536, the launcher takes forest_predict_kernel; ``n_trees`` trees in the model give
    ``trips`` passes of the four-trees-at-a-time loop and ``tail`` trees in the scalar loop. Weights, 257 rows (a second
    block of one row), missing bin on for odd counts and off (bin 15 ordinary) for even ones."""
    assert (n_trees // 4, n_trees % 4) == (trips, tail) and 128 * FB_F > 65536
    _, f, X, trees, w = _case(n_trees, FB_F, 257, [n_trees], missing=bool(n_trees % 2))
    _check(f, X, [None], trees, w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("missing", [False, True], ids=["nomissing", "missing"])
def test_fallback_two_models_uneven(missing):
    """Model 0: 5 trees on 600 listed rows (3 blocks); model 1: 11 trees on one row, so its blocks 1 and 2 leave at
    ``i >= r1``; then the same with the models swapped (the short one first: r0 != 0 for the long one)."""
    rng, f, X, trees, w = _case(20 + missing, FB_F, 300, [5, 11], K=2, missing=missing)
    rows = [rng.integers(0, 300, 600), np.array([299])]
    _check(f, X, rows, trees, w)
    _check(f, X, rows[::-1], trees[::-1], w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_fallback_row_counts(n):
    """256-row blocks: one row, one short of a block, a full block, a block and one row; ``row_list`` None (row = i)."""
    _, f, X, trees, w = _case(30 + n, FB_F, n, [6], K=3, missing=bool(n % 2))
    _check(f, X, [None], trees, w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("n_trees,missing,K", [(11, True, 1), (4, False, 8)], ids=["11trees-missing", "4trees-K8"])
def test_fallback_rounded(n_trees, missing, K):
    rng, f, X, trees, w = _case(40 + n_trees, FB_F, 257, [n_trees], K=K, missing=missing, exact=False)
    _check(f, X, [rng.permutation(257)], trees, w, exact=False)
    assert _loaded()


# =========================================================================== forest_predict_lds_kernel (F <= 512)
@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 7, 64, 384, 385, 448, 512])
def test_lds_feature_counts(F):
    """Staged rows of 128 F bytes + 16 KiB of reduction space: 64 KiB at F = 384, then 65.1, 72 and 80 KiB of dynamic
    LDS at F = 385, 448, 512. Nine trees (a full chunk of 8 on lane 0, a chunk of one on lane 1), 129 rows."""
    assert 128 * F <= 65536
    _, f, X, trees, w = _case(100 + F, F, 129, [9], K=2, missing=bool(F % 2))
    _check(f, X, [None], trees, w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("n_trees", [1, 7, 8, 9, 32, 33, 70])
def test_lds_tree_chunks(n_trees):
    """Chunks of 8 trees, lane q of a row takes chunks q, q + 4, ...: 1 and 7 are one partial chunk (its padded slots
    re-walk the first tree and must not be added), 8 one full chunk, 9 a second lane, 32 every lane once, 33 a second
    trip with a chunk of one, 70 a third trip with a chunk of 6. Weights on."""
    _, f, X, trees, w = _case(200 + n_trees, 7, 130, [n_trees], K=1, missing=bool(n_trees % 2))
    _check(f, X, [None], trees, w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_lds_row_counts(n):
    rng, f, X, trees, w = _case(300 + n, 7, n, [10], K=2)
    _check(f, X, [None], trees, w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["none-1model", "none-3models", "unsorted-repeats", "empty-of-3"])
def test_lds_row_lists(rows):
    """``row_list`` None with one model (the kernel computes ``row = i - r0``), all None with three (the wrapper's
    replicated arange), shuffled lists with repeats next to None, an empty list first, in the middle and last."""
    tpm = [9] if rows == "none-1model" else [9, 3, 12]
    rng, f, X, trees, w = _case(400 + len(rows), 12, 200, tpm, K=2)
    if rows.startswith("none"):
        _check(f, X, [None] * len(tpm), trees, w)
    elif rows == "unsorted-repeats":
        _check(f, X, [rng.integers(0, 200, 333), None, rng.permutation(200)[:129]], trees, w)
    else:
        for e in range(3):
            lists = [rng.integers(0, 200, 130), rng.integers(0, 200, 1), rng.integers(0, 200, 257)]
            lists[e] = np.zeros(0, np.int64)
            _check(f, X, lists, trees, w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 16, 17])
def test_lds_class_counts(K):
    """K <= 8 is one launch; 9, 16 and 17 run in the wrapper's class chunks of 8 (8 + 1, 8 + 8, 8 + 8 + 1)."""
    rng, f, X, trees, w = _case(500 + K, 9, 131, [11, 2], K=K)
    _check(f, X, [None, rng.integers(0, 131, 50)], trees, w)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("missing", [False, True], ids=["nomissing", "missing"])
def test_lds_depth_40_chain_and_single_leaf_trees(missing):
    """A 40-deep chain among single-leaf trees: a single leaf first and last in a model, a model of single leaves
    only, the chain alone (seven idle slots that re-walk it)."""
    rng = np.random.default_rng(600 + missing)
    mb = 7 if missing else -1
    chain = O.chain_tree(rng, 40, 40, 8, 3, missing_bin=mb)
    rest = O.random_forest(rng, 4, 40, 8, 3, single_leaf=(0, 1, 3), missing_bin=mb)
    f = te.Forest.concat([rest.tree(0), chain, rest.tree(2), rest.tree(1), rest.tree(3)])
    O.check_forest(f, 40, 8)
    X = O.chain_rows(rng, 40, 40, 8, 123, hi=6)
    if missing:
        X[rng.random(X.shape) < 0.02] = mb
    assert len(np.unique(O.reach(f, X, None, [1]))) >= 30
    w = O.exact_weights(rng, 5)
    _check(f, X, [None, np.arange(122, -1, -1), None, None], [[0, 1, 2, 3], [1], [0, 3, 4], [4, 2, 1, 0]], w)
    assert _loaded()


@pytest.mark.gpu
def test_lds_bin_255_without_a_missing_bin():
    """``missing_bin = -1`` with bin 255 in the data and as a split bin: an ordinary bin (uint8 compare, no sign)."""
    rng = np.random.default_rng(7)
    X = O.random_bins(rng, 300, 5, 256)
    X[::3, :2] = 255
    f = O.random_forest(rng, 6, 5, 256, 1, budget=41, X=X)
    f.nodes[f.tree_off[:-1], 1] = [255, 254, 0, 255, 128, 127]
    O.check_forest(f, 5, 256)
    _check(f, X, [None], [list(range(6))])
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("n_trees,F,K", [(33, 7, 1), (70, 448, 8)], ids=["33trees", "70trees-F448-K8"])
def test_lds_rounded(n_trees, F, K):
    rng, f, X, trees, w = _case(700 + n_trees, F, 129, [n_trees], K=K, exact=False)
    _check(f, X, [rng.permutation(129)], trees, w, exact=False)
    assert _loaded()


# ================================================================================== forest_predict_multi_kernel
def _variant_case(seed, F, n, tpm, K, *, exact=True, chain=False, B=16):
    """Like ``_case``; with ``chain`` the last tree is the depth-40 chain and the first rows follow it."""
    rng = np.random.default_rng(seed)
    X = O.random_bins(rng, n, F, B, B - 1)
    T = int(sum(tpm))
    values = None if exact else (lambda m, k: O.rounded_values(rng, m, k))
    f = O.random_forest(rng, T - chain, F, B, K, budget=rng.choice([1, 7, 15, 31, 63], T - chain), missing_bin=B - 1,
                        X=X, values=values)
    if chain:
        X[:min(n, 82)] = O.chain_rows(rng, 40, F, B, 82, hi=B - 2)[:min(n, 82)]
        f = te.Forest.concat([f, O.chain_tree(rng, 40, F, B, K, missing_bin=B - 1, values=values)])
        O.check_forest(f, F, B)
    perm = np.concatenate([rng.permutation(T - chain), [T - 1] * chain]).astype(np.int64)
    cuts = np.cumsum([0] + list(tpm))
    trees = [perm[cuts[m]:cuts[m + 1]].tolist() for m in range(len(tpm))]
    return rng, f, X, trees


def _draw_variants(rng, f, V):
    """V (max_depth, min_gain) pairs: depths 0..7, gains spread over the stored ones, every other one a stored gain."""
    g = f.gain[f.nodes[:, 2] >= 0]
    out = []
    for v in range(V):
        mg = float(g[rng.integers(len(g))]) if (v % 2 and len(g)) else float(rng.random())
        out.append((int(rng.integers(0, 8)), mg))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("K,V", [(1, 1), (1, 7), (1, 32), (2, 1), (2, 5), (2, 16), (4, 1), (4, 3), (4, 8), (8, 1),
                                 (8, 2), (8, 4)])
def test_multi_instantiations_and_variant_counts(K, V):
    """Every ``KT`` instantiation with ``V K`` = K (one variant), mid-range, and exactly TMOG_PM_VK = 32: V = 32 at
    K = 1 (the all-variants mask without a 32-bit shift by 32), 16 at K = 2, 8 at K = 4, 4 at K = 8."""
    assert V * K <= PM_VK and ((V, K) not in ((32, 1), (16, 2), (8, 4), (4, 8)) or V * K == PM_VK)
    rng, f, X, trees = _variant_case(1000 + 40 * K + V, 12, 130, [6], K)
    _check_multi(f, X, [None], trees, [_draw_variants(rng, f, V)])
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 4])
def test_multi_depth_clamp_on_the_chain(K):
    """Variants of max depth 0, 1, 32, 33 and 40 (and 64) on the depth-40 chain: past depth 32 the kernel reads
    ``s_dmask[min(dep, 32)]``, the variants with ``max_depth <= 32``, so 33 and 40 must still differ from each other
    and from 32 only through the grown leaves."""
    rng, f, X, trees = _variant_case(1100 + K, 48, 123, [3], K, chain=True)
    vs = [(0, 0.0), (1, 0.0), (32, 0.0), (33, 0.0), (40, 0.0), (64, 0.0)]
    c = [f.n_trees - 1]
    outs = [O.walk(f, X, None, c, stop=O.variant_stop(f, d, g)) for d, g in vs]
    assert all(not np.array_equal(outs[i], outs[i + 1]) for i in range(4)) and np.array_equal(outs[4], outs[5])
    _check_multi(f, X, [None], trees, [vs])
    assert _loaded()


@pytest.mark.gpu
def test_multi_gain_threshold_edges():
    """A min gain equal to a stored fp32 gain keeps that split (``>=``), one ulp above cuts it; a min gain above every
    gain and max depth 0 both stop every walk at the root."""
    rng, f, X, trees = _variant_case(1200, 12, 200, [5], 2)
    root = int(f.tree_off[np.argmax(np.diff(f.tree_off))])
    stored = float(f.gain[root])
    above = float(np.nextafter(np.float32(stored), np.float32(2)))
    vs = [(64, stored), (64, above), (64, 2.0), (0, 0.0), (3, stored), (64, 0.0)]
    outs = [O.walk(f, X, None, trees[0], stop=O.variant_stop(f, d, g)) for d, g in vs]
    assert not np.array_equal(outs[0], outs[1]) and np.array_equal(outs[2], outs[3])
    _check_multi(f, X, [None], trees, [vs])
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("n_trees", [1, 4, 5, 16, 17, 40])
def test_multi_tree_chunks(n_trees):
    """Chunks of 4 trees over 4 lanes per row: a partial chunk, one full, a second lane, every lane once (16), a
    second trip with a chunk of one (17), a third (40)."""
    rng, f, X, trees = _variant_case(1300 + n_trees, 12, 70, [n_trees], 2)
    _check_multi(f, X, [None], trees, [_draw_variants(rng, f, 4)])
    assert _loaded()


@pytest.mark.gpu
def test_multi_two_models_of_one_forest():
    """Different variant counts, row lists (one shuffled with repeats, the other all rows; then one empty) and trees of
    one shared forest, the chain among them."""
    rng, f, X, trees = _variant_case(1400, 48, 150, [7, 3], 4, chain=True)
    vs = [_draw_variants(rng, f, 8), [(40, 0.0), (2, 0.5), (33, 0.1)]]
    _check_multi(f, X, [rng.integers(0, 150, 201), None], trees, vs)
    _check_multi(f, X, [np.zeros(0, np.int64), rng.permutation(150)[:65]], trees, vs)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [12, 512, 513, 1024, 2040, 2045])
def test_multi_feature_counts(F):
    """64 F bytes of staged rows + 32 KiB of accumulators (+ 132 bytes of static depth table): 64 KiB at F = 512,
    just past it at 513, 96 KiB at 1024, 159.6 KiB at 2040, and 2045, the last F under the 160 KiB refusal (60 bytes
    to spare)."""
    assert te._pm_lds_bytes(F) <= 160 * 1024 and 64 * F + 32768 + 132 <= 163840
    rng, f, X, trees = _variant_case(1500 + F, F, 65, [5], 2)
    _check_multi(f, X, [None], trees, [_draw_variants(rng, f, 3)])
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [2046, 2049])
def test_multi_past_the_lds_limit_falls_back_by_value(F):
    """F = 2046 is the first to need more than 160 KiB (64 * 2046 + 32 KiB of dynamic LDS alone still fits: the
    kernel's 132 static bytes tip it), 2049 exceeds it in dynamic LDS alone: the documented fallback prunes and
    predicts each variant (forest_predict_kernel, F > 512) and must give the same values."""
    assert te._pm_lds_bytes(2045) <= 160 * 1024 < te._pm_lds_bytes(2046) and 64 * 2046 + 32768 <= 163840
    rng, f, X, trees = _variant_case(1600 + F, F, 65, [5], 2)
    _check_multi(f, X, [None], trees, [_draw_variants(rng, f, 3)], F_fallback=True)
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_multi_row_counts(n):
    rng, f, X, trees = _variant_case(1700 + n, 48, n, [6], 1, chain=True)
    _check_multi(f, X, [None], trees, [_draw_variants(rng, f, 5) + [(40, 0.0)]])
    assert _loaded()


@pytest.mark.gpu
@pytest.mark.parametrize("K,n_trees,F", [(1, 17, 12), (8, 40, 513)], ids=["K1-17trees", "K8-40trees-F513"])
def test_multi_rounded(K, n_trees, F):
    rng, f, X, trees = _variant_case(1800 + K, F, 130, [n_trees], K, exact=False)
    _check_multi(f, X, [rng.permutation(130)], trees, [_draw_variants(rng, f, 4)], exact=False)
    assert _loaded()


# ===================================================================================== C entry points: write guards
def _raw_args(f, X, model_rows, model_trees, w):
    """The arrays ``forest_predict`` ships, as device tensors (kept alive by the caller)."""
    order = [t for ts in model_trees for t in ts]
    mto = np.concatenate([[0], np.cumsum([len(ts) for ts in model_trees])]).astype(np.int64)
    counts = [len(r) for r in model_rows]
    mro = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    row_list = np.concatenate(model_rows).astype(np.int32)
    a = dict(X=_d(X), mro=_d(mro), rows=_d(row_list), mto=_d(mto), toff=_d(f.tree_off[:-1][order].astype(np.int64)),
             tw=_d(np.asarray(w, np.float32)[order]), nodes=_d(f.nodes), dl=_d(f.default_left), val=_d(f.value))
    return a, counts


PAD = 64


@pytest.mark.gpu
@pytest.mark.parametrize("F", [12, FB_F], ids=["lds", "fallback"])
def test_predict_writes_exactly_its_rows(F):
    """tmog_hip_forest_predict into a sentinel-filled buffer with a sentinel head and tail: exactly the
    ``[sum rows_m, K]`` region holds values, of three models with 129, 0 and 257 rows."""
    rng, f, X, trees, w = _case(2000 + F, F, 200, [5, 2, 9], K=3)
    rows = [rng.integers(0, 200, 129), np.zeros(0, np.int64), rng.integers(0, 200, 257)]
    a, counts = _raw_args(f, X, rows, trees, w)
    total = sum(counts) * 3
    buf = _d(np.full(PAD + total + PAD, SENT, np.float32))
    rc = _lib().tmog_hip_forest_predict(_p(a["X"]), F, 3, _p(a["mro"]), _p(a["rows"]), max(counts), _p(a["mto"]),
                                        _p(a["toff"]), _p(a["tw"]), _p(a["nodes"]), _p(a["dl"]), f.missing_bin,
                                        _p(a["val"]), 3, buf.data_ptr() + 4 * PAD, _st())
    torch.cuda.synchronize()
    assert rc == 0
    got = buf.cpu().numpy()
    assert (got[:PAD] == SENT).all() and (got[PAD + total:] == SENT).all()
    body = got[PAD:PAD + total].reshape(-1, 3)
    assert (body != SENT).all()
    O.assert_matches(body[:129], f, X, rows[0], trees[0], w)
    O.assert_matches(body[129:], f, X, rows[2], trees[2], w)
    assert _loaded()


def _multi_args(f, X, model_rows, model_trees, variants, vout):
    a, counts = _raw_args(f, X, model_rows, model_trees, np.ones(f.n_trees, np.float32))
    voff = np.concatenate([[0], np.cumsum([len(v) for v in variants])]).astype(np.int32)
    vdep = np.asarray([d for vs in variants for d, _ in vs], np.int32)
    mask = np.zeros(len(f.nodes), np.uint32)
    leaf = f.nodes[:, 2] < 0
    for m, vs in enumerate(variants):                       # node_mask: the variants that stop at a node at any depth
        for t in model_trees[m]:
            sl = slice(int(f.tree_off[t]), int(f.tree_off[t + 1]))
            for k, (_, g) in enumerate(vs):
                mask[sl] |= ((f.gain[sl] < np.float32(g)) | leaf[sl]).astype(np.uint32) << np.uint32(k)
    a.update(mask=_d(mask.view(np.int32)), voff=_d(voff), vdep=_d(vdep), vout=_d(np.asarray(vout, np.int64)))
    return a, counts


def _call_multi(a, F, n_models, max_rows, f, K, out_ptr):
    return _lib().tmog_hip_forest_predict_multi(
        _p(a["X"]), F, n_models, _p(a["mro"]), _p(a["rows"]), max_rows, _p(a["mto"]), _p(a["toff"]), _p(a["tw"]),
        _p(a["nodes"]), _p(a["dl"]), f.missing_bin, _p(a["val"]), K, _p(a["mask"]), _p(a["voff"]), _p(a["vdep"]),
        _p(a["vout"]), out_ptr, _st())


@pytest.mark.gpu
def test_multi_writes_exactly_its_variant_regions():
    """tmog_hip_forest_predict_multi with ``var_out_off`` regions placed out of order and with gaps in a
    sentinel-filled buffer: exactly the ``[rows_m, K]`` region of every variant changes; gaps, head and tail do not."""
    K = 2
    rng, f, X, trees = _variant_case(2100, 12, 150, [5, 3], K)
    rows = [rng.integers(0, 150, 65), rng.integers(0, 150, 130)]
    variants = [[(2, 0.0), (64, 0.3), (0, 0.0)], [(1, 0.2), (64, 0.0)]]
    size = [65 * K] * 3 + [130 * K] * 2
    slot = [3, 0, 4, 1, 2]                                  # placement order of the five regions
    vout, pos = [0] * 5, 7
    for s in np.argsort(slot):
        vout[s] = pos
        pos += size[s] + 5
    a, counts = _multi_args(f, X, rows, trees, variants, vout)
    buf = _d(np.full(PAD + pos + PAD, SENT, np.float32))
    rc = _call_multi(a, 12, 2, max(counts), f, K, buf.data_ptr() + 4 * PAD)
    torch.cuda.synchronize()
    assert rc == 0
    got = buf.cpu().numpy()
    written = np.zeros(got.size, bool)
    i = 0
    for m, vs in enumerate(variants):
        for d, g in vs:
            lo = PAD + vout[i]
            written[lo:lo + size[i]] = True
            O.assert_matches(got[lo:lo + size[i]].reshape(-1, K), f, X, rows[m], trees[m], stop=O.variant_stop(f, d, g))
            i += 1
    assert (got[written] != SENT).all() and (got[~written] == SENT).all() and (~written).sum() == 2 * PAD + 7 + 5 * 5
    assert _loaded()


@pytest.mark.gpu
def test_launcher_guards_refuse_without_a_launch():
    """``K > 8`` -> -2 from tmog_hip_forest_predict; K = 3 -> -2 and an LDS request above 160 KiB (F = 2049, and 2046
    once the kernel's static table is counted) -> -3 from the multi entry; the output buffer stays untouched."""
    rng, f, X, trees = _variant_case(2200, 12, 20, [3], 9)
    rows = [np.arange(20)]
    a, counts = _multi_args(f, X, rows, trees, [[(2, 0.0)]], [0])
    buf = _d(np.full(20 * 9 + PAD, SENT, np.float32))
    lib = _lib()
    assert lib.tmog_hip_forest_predict(_p(a["X"]), 12, 1, _p(a["mro"]), _p(a["rows"]), 20, _p(a["mto"]), _p(a["toff"]),
                                       _p(a["tw"]), _p(a["nodes"]), _p(a["dl"]), f.missing_bin, _p(a["val"]), 9,
                                       _p(buf), _st()) == -2
    assert _call_multi(a, 12, 1, 20, f, 3, _p(buf)) == -2
    rng, f2, X2, trees2 = _variant_case(2201, 2049, 20, [3], 2)
    a2, _ = _multi_args(f2, X2, rows, trees2, [[(2, 0.0)]], [0])
    assert _call_multi(a2, 2049, 1, 20, f2, 2, _p(buf)) == -3
    assert _call_multi(a2, 2046, 1, 20, f2, 2, _p(buf)) == -3     # dynamic + the kernel's static LDS: 163844 bytes
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
    assert _loaded()



# ===================================================================== the oracle cases again, on the direct source
# A copy of every test above that scores through ``tree_engine`` (the three raw-entry tests call the direct entries
# themselves and run once), with its marks and parameters, under the name the fixture looks for.
RAW_ENTRY = ("test_predict_writes_exactly_its_rows", "test_multi_writes_exactly_its_variant_regions",
             "test_launcher_guards_refuse_without_a_launch")
for _name, _test in list(globals().items()):
    if _name.startswith("test_") and _name not in RAW_ENTRY:
        _copy = types.FunctionType(_test.__code__, globals(), _name + DIRECT, _test.__defaults__, _test.__closure__)
        _copy.__dict__.update(_test.__dict__)
        _copy.__doc__ = _test.__doc__
        globals()[_name + DIRECT] = _copy
