"""The kernels of ``ops/csrc/hip/forest_predict_kernels.hip`` (``forest_predict_lds_kernel``, ``forest_predict_kernel``
and ``forest_predict_multi_kernel<NS, KT, VKP>``) over the packed node image that ``forest_image_kernel`` builds,
against

* the numpy walk of tests/forest_predict_oracle.py, in its exact and its rounded regime, and
* the same kernels over the direct node source (``TMOG_PREDICT_V1=1``, here reached by patching
  ``tree_engine.predict_v1``): in the rounded regime, with random fp32 values and weights, every output must be
  bit-identical, because each output element sees the same fp32 operations in the same order on both paths.

Both paths run one kernel body, so the bit equality shows that the two node sources agree, not that two
implementations do. The independent reference is the numpy walk: the exact regime by equality, the rounded regime
within the walk's own bound, and each is asserted on both paths.

One forest per (F, K) is built once and shared by the cases; the LDS kernels stage rows with 16-byte loads at F = 64,
4-byte loads at F = 132 and the byte loop at F = 5; F = 513 takes the kernel that leaves rows in global memory."""
import functools

import numpy as np
import pytest
import torch

import forest_predict_oracle as O
from transmogrifai_amd.models import tree_engine as te

SENT = np.float32(-1.5e30)
PAD = 64
B = 16
TREES = (1, 3, 4, 5, 17, 33)            # chunk and stride edges of both LDS kernels (4 x 4 and 8 x 4 trees a trip)
ROWS = (0, 1, 63, 64, 65, 129, 300)     # block edges of the 64- and 128-row workgroups, an empty model


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


@functools.lru_cache(maxsize=None)
def _forest(F, K, exact):
    """300 rows and sum(TREES) = 63 trees: a single leaf first, random trees of 0..31 splits, and last a chain of
    depth min(13, F); a missing bin with both default directions. The arrays are shared by the cases: never edited."""
    rng = np.random.default_rng(1000 * F + 10 * K + exact)
    mb = B - 1
    T = sum(TREES)
    values = None if exact else (lambda m, k: O.rounded_values(rng, m, k))
    X = O.random_bins(rng, 300, F, B, mb)
    depth = min(13, F)
    X[:56] = np.where(rng.random((56, F)) < 0.05, mb, O.chain_rows(rng, depth, F, B, 56, hi=B - 2))
    body = O.random_forest(rng, T - 1, F, B, K, budget=rng.choice([1, 3, 7, 15, 31, 63], T - 1), single_leaf=(0,),
                           missing_bin=mb, X=X, values=values)
    f = te.Forest.concat([body, O.chain_tree(rng, depth, F, B, K, missing_bin=mb, values=values)])
    O.check_forest(f, F, B)
    assert int(te._node_depth(f).max()) >= depth and set(np.unique(f.default_left)) == {0, 1}
    assert (X == mb).any() and te.image_fits(f)
    w = O.exact_weights(rng, T) if exact else O.rounded_weights(rng, T)
    perm = np.concatenate([rng.permutation(T - 1), [T - 1]])      # the chain ends the 33-tree model
    cuts = np.cumsum([0] + list(TREES))
    trees = [perm[cuts[m]:cuts[m + 1]].tolist() for m in range(len(TREES))]
    return f, X, trees, w


def _fresh(f):
    """The same forest as a new object: no image cached on it."""
    return te.Forest(f.tree_off, f.nodes, f.default_left, f.value, f.gain, f.cover, f.tree_model, f.missing_bin)


def _both(monkeypatch, call):
    """``call()`` on the image path, then on the direct node source."""
    monkeypatch.setattr(te, "predict_v1", lambda: False)
    new = call()
    monkeypatch.setattr(te, "predict_v1", lambda: True)
    old = call()
    torch.cuda.synchronize()
    return new, old


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


# ================================================================================================= the record
def test_image_packing_against_numpy():
    """CPU only: ``pack_node_image`` field by field, and the limits of the record."""
    rng = np.random.default_rng(5)
    f = O.random_forest(rng, 9, 300, 256, 2, budget=31, missing_bin=255)
    f.nodes[f.tree_off[:-1], 0] = [0, 1, 255, 256, 299, 7, 8, 9, 10]
    f.nodes[f.tree_off[:-1], 1] = [0, 255, 254, 128, 127, 1, 2, 3, 4]
    mask = rng.integers(0, 2 ** 32, len(f.nodes), dtype=np.uint64).astype(np.uint32)
    img = te.pack_node_image(f.nodes, f.default_left, mask)
    assert img.dtype == np.uint32 and img.shape == (len(f.nodes), 4)
    for i in range(len(f.nodes)):
        feat, sbin, left, right = (int(v) for v in f.nodes[i])
        assert int(img[i, 0]) == feat + (sbin << 16) + (int(f.default_left[i] != 0) << 24)
        assert int(img[i, 1]) == int(mask[i])
        assert int(img[i, 2]) == left % 2 ** 32 and int(img[i, 3]) == right % 2 ** 32
    assert (te.pack_node_image(f.nodes, f.default_left)[:, 1] == 0).all()
    assert np.array_equal(img[:, 0] & 0xFFFF, f.nodes[:, 0]) and np.array_equal((img[:, 0] >> 16) & 0xFF, f.nodes[:, 1])
    assert te.image_fits(f)
    for col, v, ok in ((0, 65535, True), (0, 65536, False), (1, 255, True), (1, 256, False), (0, -1, False)):
        g = _fresh(f)
        g.nodes = f.nodes.copy()
        g.nodes[3, col] = v
        assert te.image_fits(g) == ok, (col, v)


@pytest.mark.gpu
def test_image_kernel_matches_the_packing():
    f, X, trees, w = _forest(64, 2, True)
    rng = np.random.default_rng(11)
    mask = rng.integers(0, 2 ** 32, len(f.nodes), dtype=np.uint64).astype(np.uint32)
    for mk in (None, mask):
        buf = _d(np.full((len(f.nodes) + 2, 4), -7, np.int32))
        nodes, dl, mt = _d(f.nodes), _d(f.default_left), (None if mk is None else _d(mk.view(np.int32)))
        assert _lib().tmog_hip_forest_image(_p(nodes), _p(dl), _p(mt), len(f.nodes), buf.data_ptr() + 16, _st()) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[0] == -7).all() and (got[-1] == -7).all()
        assert np.array_equal(got[1:-1].view(np.uint32), te.pack_node_image(f.nodes, f.default_left, mk))


# ============================================================================================ plain scoring
def _plain(f, X, model_rows, model_trees, w):
    return te.forest_predict(_fresh(f), _d(X), [_t(r) for r in model_rows], model_trees, w)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("F", [5, 64, 132, 513])
def test_plain_listed_rows(F, K, monkeypatch):
    """Seven models of one call: 0, 1, 63, 64, 65, 129 and 300 listed rows (shuffled, with repeats) with 1, 3, 4, 5,
    17, 33 and again 1 trees. (a) exact regime against the walk, on both paths; (a, b) rounded regime against the
    walk's bound and bit-identical between the paths."""
    for exact in (True, False):
        f, X, trees, w = _forest(F, K, exact)
        r2 = np.random.default_rng(F + K)
        rows = [r2.integers(0, 300, n) for n in ROWS]
        mt = [trees[0]] + trees                       # the empty model has trees too
        new, old = _both(monkeypatch, lambda: _plain(f, X, rows, mt, w))
        for g, h, r, ts in zip(new, old, rows, mt):
            assert g.shape == (len(r), K)
            O.assert_matches(g.cpu().numpy(), f, X, r, ts, w, exact=exact)
            O.assert_matches(h.cpu().numpy(), f, X, r, ts, w, exact=exact)
            assert np.array_equal(_bits(g), _bits(h))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 300])
@pytest.mark.parametrize("F", [5, 64, 132, 513])
def test_plain_all_rows_without_a_row_list(F, n, monkeypatch):
    """One model over the first ``n`` rows, ``row_list`` null (the kernels compute the row from the block), rounded
    regime: the bound, and the two paths bit for bit; then three models (the wrapper's replicated arange)."""
    f, X, trees, w = _forest(F, 2, False)
    Xn = np.ascontiguousarray(X[:n])
    new, old = _both(monkeypatch, lambda: _plain(f, Xn, [None], [trees[5]], w))
    O.assert_matches(new[0].cpu().numpy(), f, Xn, None, trees[5], w, exact=False)
    assert np.array_equal(_bits(new[0]), _bits(old[0]))
    if n == 129:
        new, old = _both(monkeypatch, lambda: _plain(f, Xn, [None] * 3, trees[2:5], w))
        for g, h, ts in zip(new, old, trees[2:5]):
            O.assert_matches(g.cpu().numpy(), f, Xn, None, ts, w, exact=False)
            assert np.array_equal(_bits(g), _bits(h))


@pytest.mark.gpu
def test_plain_empty_rows():
    f, X, trees, w = _forest(64, 2, True)
    got = te.forest_predict(_fresh(f), _d(X[:0]), [None], [trees[3]], w)
    assert got[0].shape == (0, 2)


# ========================================================================================== variant scoring
def _variants(rng, f, V):
    """V (max_depth, min_gain) pairs: depths 0..13, one of them past the kernel's depth table (33: its depth part is
    folded into the node masks), min gains spread over the stored ones, every other one a stored gain."""
    g = f.gain[f.nodes[:, 2] >= 0]
    out = []
    for v in range(V):
        mg = float(g[rng.integers(len(g))]) if v % 2 else float(rng.random()) * 0.5
        out.append((int(rng.integers(0, 14)), mg))
    out[V // 2] = (33, 0.0)
    return out


def _multi(f, X, model_rows, model_trees, variants):
    return te.forest_predict_multi(_fresh(f), _d(X), [_t(r) for r in model_rows], model_trees, variants)


@pytest.mark.gpu
@pytest.mark.parametrize("K,V", [(1, 1), (1, 9), (1, 32), (2, 1), (2, 9), (3, 9)])
@pytest.mark.parametrize("F", [5, 64, 132, 513])
def test_multi_listed_rows(F, K, V, monkeypatch):
    """Three models of one shared forest with 33, 5 and 17 trees, V, 1 and min(V, 3) variants and 300, 0 and 65
    listed rows. V K picks the 8-, 16- or 32-sum register tile (1, 2 -> 8; 9 -> 16; 18, 32 -> 32); K = 3 is not a
    kernel instantiation: the wrapper prunes and scores each variant with the plain kernels. Both regimes against
    the walk, and the paths bit for bit."""
    for exact in (True, False):
        f, X, trees, w = _forest(F, K, exact)
        r2 = np.random.default_rng(100 * F + 10 * K + V)
        vs = [_variants(r2, f, V), [(2, 0.25)], _variants(r2, f, V)[:min(V, 3)]]
        rows = [r2.integers(0, 300, 300), np.zeros(0, np.int64), r2.permutation(300)[:65]]
        mt = [trees[5], trees[3], trees[4]]
        new, old = _both(monkeypatch, lambda: _multi(f, X, rows, mt, vs))
        assert [len(g) for g in new] == [len(v) for v in vs]
        for m in range(3):
            for g, h, (d, mg) in zip(new[m], old[m], vs[m]):
                O.assert_matches(g.cpu().numpy(), f, X, rows[m], mt[m], stop=O.variant_stop(f, d, mg), exact=exact)
                assert np.array_equal(_bits(g), _bits(h))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("trees_i", [0, 1, 2, 3, 4], ids=lambda i: f"{TREES[i]}trees")
def test_multi_all_rows_and_tree_counts(n, trees_i, monkeypatch):
    """One model over all ``n`` rows (no list from the caller), 1, 3, 4, 5 and 17 trees, nine variants at K = 2."""
    f, X, trees, w = _forest(132, 2, False)
    Xn = np.ascontiguousarray(X[:n])
    vs = [_variants(np.random.default_rng(n + trees_i), f, 9)]
    new, old = _both(monkeypatch, lambda: _multi(f, Xn, [None], [trees[trees_i]], vs))
    for g, h, (d, mg) in zip(new[0], old[0], vs[0]):
        O.assert_matches(g.cpu().numpy(), f, Xn, None, trees[trees_i], stop=O.variant_stop(f, d, mg), exact=False)
        assert np.array_equal(_bits(g), _bits(h))


# ============================================================================ forests the record cannot hold
@pytest.mark.gpu
def test_feature_index_past_16_bits_takes_the_direct_kernels():
    """A forest that splits on column 65540 does not fit the record: no image is built and the result is the
    walk's (the direct node source, which reads ``nodes``)."""
    rng = np.random.default_rng(77)
    F = 65600
    X = O.random_bins(rng, 65, F, B, B - 1)
    f = O.random_forest(rng, 5, F, B, 2, budget=15, missing_bin=B - 1, X=X)
    f.nodes[f.tree_off[1], 0] = 65540
    assert f.nodes[f.tree_off[1], 2] >= 0 and not te.image_fits(f)
    got = te.forest_predict(f, _d(X), [None], [list(range(5))])
    torch.cuda.synchronize()
    assert [e[2] for e in f._images.values()] == [None]
    O.assert_matches(got[0].cpu().numpy(), f, X, None, list(range(5)))


@pytest.mark.gpu
def test_split_bin_past_8_bits_takes_the_direct_kernels():
    """Split bin 300 (every bin goes left): outside the record, so the LDS and the variant kernel run over the direct
    node source."""
    f0, X, trees, w = _forest(64, 2, True)
    f = _fresh(f0)
    f.nodes = f0.nodes.copy()
    roots = f.tree_off[:-1][f.nodes[f.tree_off[:-1], 2] >= 0]
    f.nodes[roots[:7], 1] = 300
    assert not te.image_fits(f)
    got = te.forest_predict(f, _d(X), [None], [trees[5]], w)
    vs = [[(3, 0.0), (13, 0.2), (33, 0.0)]]
    gm = te.forest_predict_multi(f, _d(X), [None], [trees[5]], vs)
    torch.cuda.synchronize()
    assert len(f._images) == 2 and all(e[2] is None for e in f._images.values())
    O.assert_matches(got[0].cpu().numpy(), f, X, None, trees[5], w)
    for g, (d, mg) in zip(gm[0], vs[0]):
        O.assert_matches(g.cpu().numpy(), f, X, None, trees[5], stop=O.variant_stop(f, d, mg))


# ================================================================================================ the cache
@pytest.mark.gpu
def test_replacing_a_forest_array_rebuilds_the_image(monkeypatch):
    monkeypatch.setattr(te, "predict_v1", lambda: False)
    f0, X, trees, w = _forest(64, 2, True)
    f = _fresh(f0)
    Xd = _d(X)
    vs = [[(3, 0.0), (13, 0.2)]]

    def images():
        return {k[0]: e[2] for k, e in f._images.items()}

    def check():
        got = te.forest_predict(f, Xd, [None], [trees[5]], w)
        gm = te.forest_predict_multi(f, Xd, [None], [trees[5]], vs)
        torch.cuda.synchronize()
        O.assert_matches(got[0].cpu().numpy(), f, X, None, trees[5], w)
        for g, (d, mg) in zip(gm[0], vs[0]):
            O.assert_matches(g.cpu().numpy(), f, X, None, trees[5], stop=O.variant_stop(f, d, mg))
        return images()

    first = check()
    assert set(first) == {"plain", "multi"} and all(v is not None for v in first.values())
    again = check()
    assert all(again[k] is first[k] for k in first)                      # a second batch scores from the same image
    f.nodes = f0.nodes.copy()
    internal = np.nonzero(f.nodes[:, 2] >= 0)[0]
    f.nodes[internal, 1] = (f.nodes[internal, 1] + 5) % (B - 1)           # other split bins: other results
    second = check()
    assert all(second[k] is not first[k] for k in first)
    f.default_left = (1 - f0.default_left).astype(np.uint8)
    third = check()
    assert all(third[k] is not second[k] for k in first)
    f.gain = (f0.gain * np.float32(0.5)).astype(np.float32)               # only the variant masks read the gains
    fourth = check()
    assert fourth["plain"] is third["plain"] and fourth["multi"] is not third["multi"]
    vs[0][1] = (13, 0.05)                                                 # other variants: other mask words
    fifth = check()
    assert fifth["multi"] is not fourth["multi"]


# ===================================================================================== write guards, raw entries
def _raw(f, X, model_rows, model_trees, w, mask=None):
    order = [t for ts in model_trees for t in ts]
    mto = np.concatenate([[0], np.cumsum([len(ts) for ts in model_trees])]).astype(np.int64)
    counts = [len(r) for r in model_rows]
    mro = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    a = dict(X=_d(X), mro=_d(mro), rows=_d(np.concatenate(model_rows).astype(np.int32)), mto=_d(mto),
             toff=_d(f.tree_off[:-1][order].astype(np.int64)), tw=_d(np.asarray(w, np.float32)[order]),
             val=_d(f.value), img=_d(te.pack_node_image(f.nodes, f.default_left, mask).view(np.int32)))
    return a, counts


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 513], ids=["lds", "global-rows"])
def test_predict_image_writes_exactly_its_rows(F):
    f, X, trees, w = _forest(F, 3, True)
    rng = np.random.default_rng(12)
    rows = [rng.integers(0, 300, 129), np.zeros(0, np.int64), rng.integers(0, 300, 257)]
    mt = [trees[3], trees[1], trees[4]]
    a, counts = _raw(f, X, rows, mt, w)
    total = sum(counts) * 3
    buf = _d(np.full(PAD + total + PAD, SENT, np.float32))
    rc = _lib().tmog_hip_forest_predict_image(_p(a["X"]), F, 3, _p(a["mro"]), _p(a["rows"]), max(counts), _p(a["mto"]),
                                              _p(a["toff"]), _p(a["tw"]), _p(a["img"]), f.missing_bin, _p(a["val"]), 3,
                                              buf.data_ptr() + 4 * PAD, _st())
    torch.cuda.synchronize()
    assert rc == 0
    got = buf.cpu().numpy()
    assert (got[:PAD] == SENT).all() and (got[PAD + total:] == SENT).all()
    body = got[PAD:PAD + total].reshape(-1, 3)
    assert (body != SENT).all()
    O.assert_matches(body[:129], f, X, rows[0], mt[0], w)
    O.assert_matches(body[129:], f, X, rows[2], mt[2], w)


@pytest.mark.gpu
def test_multi_image_writes_exactly_its_variant_regions():
    """Regions placed out of order with gaps in a sentinel-filled buffer, random tree weights (rounded regime)."""
    K, F = 2, 132
    f, X, trees, w = _forest(F, K, False)
    rng = np.random.default_rng(13)
    rows = [rng.integers(0, 300, 65), rng.integers(0, 300, 130)]
    mt = [trees[3], trees[4]]
    variants = [[(2, 0.0), (64, 0.3), (0, 0.0)], [(1, 0.2), (64, 0.0)]]
    size = [65 * K] * 3 + [130 * K] * 2
    slot = [3, 0, 4, 1, 2]
    vout, pos = [0] * 5, 7
    for s in np.argsort(slot):
        vout[s] = pos
        pos += size[s] + 5
    mask = np.zeros(len(f.nodes), np.uint32)
    leaf = f.nodes[:, 2] < 0
    for m, vs in enumerate(variants):
        for t in mt[m]:
            sl = slice(int(f.tree_off[t]), int(f.tree_off[t + 1]))
            for k, (_, g) in enumerate(vs):
                mask[sl] |= ((f.gain[sl] < np.float32(g)) | leaf[sl]).astype(np.uint32) << np.uint32(k)
    a, counts = _raw(f, X, rows, mt, w, mask)
    voff = _d(np.array([0, 3, 5], np.int32))
    vdep = _d(np.asarray([d for vs in variants for d, _ in vs], np.int32))
    vo = _d(np.asarray(vout, np.int64))
    buf = _d(np.full(PAD + pos + PAD, SENT, np.float32))
    lib = _lib()
    rc = lib.tmog_hip_forest_predict_multi_image(
        _p(a["X"]), F, 2, _p(a["mro"]), _p(a["rows"]), max(counts), _p(a["mto"]), _p(a["toff"]), _p(a["tw"]),
        _p(a["img"]), f.missing_bin, _p(a["val"]), K, _p(voff), _p(vdep), _p(vo), 3, buf.data_ptr() + 4 * PAD, _st())
    torch.cuda.synchronize()
    assert rc == 0
    got = buf.cpu().numpy()
    written = np.zeros(got.size, bool)
    i = 0
    for m, vs in enumerate(variants):
        for d, g in vs:
            lo = PAD + vout[i]
            written[lo:lo + size[i]] = True
            O.assert_matches(got[lo:lo + size[i]].reshape(-1, K), f, X, rows[m], mt[m], w,
                             stop=O.variant_stop(f, d, g), exact=False)
            i += 1
    assert (got[written] != SENT).all() and (got[~written] == SENT).all()
    before = got.copy()
    # refusals leave the buffer alone: K = 3, more variants than sums, LDS past 160 KiB
    args = lambda F_, K_, mv: (  # noqa: E731
        _p(a["X"]), F_, 2, _p(a["mro"]), _p(a["rows"]), max(counts), _p(a["mto"]), _p(a["toff"]), _p(a["tw"]),
        _p(a["img"]), f.missing_bin, _p(a["val"]), K_, _p(voff), _p(vdep), _p(vo), mv, buf.data_ptr() + 4 * PAD, _st())
    assert lib.tmog_hip_forest_predict_multi_image(*args(F, 3, 3)) == -2
    assert lib.tmog_hip_forest_predict_multi_image(*args(F, 2, 17)) == -2
    assert lib.tmog_hip_forest_predict_multi_image(*args(2560, 2, 3)) == -3
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
