"""``Learner.partial_dependence_pairs`` of the tree learners, Friedman's H-statistic and
``OpWorkflowModel.partial_dependence_pairs`` on the small fits of tests/test_partial_dependence.py, against
rescoring: both columns of a pair set to a value inside each of their bins and the model's own ``predict`` averaged
over the rows. The bound is that file's ``_tol`` (the same quantities through the same maps, so the same slopes): a
cell of a surface is, like a point of a curve, the fp64-exact mean of the tree sums where ``predict`` sums T fp32
terms."""
import itertools
import json

import numpy as np
import pytest
import torch

import forest_loco_oracle as L
import forest_pd_oracle as O
import forest_pd_pairs_oracle as O2
import test_partial_dependence as TP
from transmogrifai_amd.insights.partial_dependence import PairDependence, h_statistic
from transmogrifai_amd.models import tree_engine as te
from transmogrifai_amd.models.tree_engine import Forest


def _pairs_of(model, d, k=3):
    return list(itertools.combinations(TP._top_columns(model, d, k), 2))


def _rescored2(model, X, a, b, bins_a, bins_b):
    """``predict`` on copies of ``X`` with columns ``a`` and ``b`` at a value inside each pair of the bins: (raw,
    response) float64 ``[len(bins_a), len(bins_b), n, C']``."""
    spec = model.learner._forest(model.state)[1]
    n, m = X.shape[0], len(bins_a) * len(bins_b)
    big = X.repeat(m, 1)
    for k, (i, j) in enumerate(itertools.product(bins_a, bins_b)):
        big[k * n:(k + 1) * n, a] = TP._bin_value(spec, a, int(i))
        big[k * n:(k + 1) * n, b] = TP._bin_value(spec, b, int(j))
    pred, raw, prob = model.learner.predict(model.state, big)
    raw = (raw if raw.shape[1] > 0 else pred.reshape(-1, 1)).to(torch.float64)
    resp = (prob if prob.shape[1] > 0 else pred.reshape(-1, 1)).to(torch.float64)
    return (raw.reshape(len(bins_a), len(bins_b), n, -1), resp.reshape(len(bins_a), len(bins_b), n, -1))


def _some(bins, k=9):
    """At most ``k`` of a column's valid bins, evenly spread, the first and the last two (the last ordinary bin and
    the missing bin, when there is one) among them: rescoring costs one ``predict`` of every row per cell, and a
    real column has up to 63 bins here. The engine below the learners is checked on every cell of every surface
    against the brute-force oracle, on that oracle's forests, in tests/test_forest_pd_pairs.py."""
    if len(bins) <= k:
        return bins
    pick = sorted(set(np.linspace(0, len(bins) - 2, k - 1).round().astype(int).tolist()) | {len(bins) - 1})
    return bins[torch.tensor(pick)]


# ------------------------------------------------------------------------------------------------ learner level
@pytest.mark.parametrize("key", TP.TREE_KEYS)
def test_learner_surfaces_match_rescoring(key):
    _, scored, vec, model = TP._fit(key)
    X = scored[vec.name].values
    n, d = int(X.shape[0]), int(X.shape[1])
    learner, state = model.learner, model.state
    spec = learner._forest(state)[1]
    pairs = _pairs_of(model, d)
    assert len(pairs) == 3
    raw, valid, counts = learner.partial_dependence_pairs(state, X, pairs, scale="raw")
    resp, valid2, counts2 = learner.partial_dependence_pairs(state, X, pairs, scale="response")
    NB = int(spec.B)
    assert tuple(raw.shape) == (3, NB, NB, TP._OUT[key]) and tuple(resp.shape) == (3, NB, NB, TP._OUT[key])
    assert raw.dtype == torch.float64 and valid.dtype == torch.bool and tuple(valid.shape) == (3, NB, NB)
    assert torch.equal(valid, valid2) and torch.equal(counts, counts2)
    assert counts.sum((1, 2)).tolist() == [n] * 3                   # every row sits in one cell of every pair
    assert not counts[~valid].any()
    cols = sorted({c for p in pairs for c in p})
    _, valid1, counts1, _ = learner.partial_dependence(state, X, cols, scale="raw")
    tol_raw, tol_resp = TP._tol(key, model, TP._RAW_SLOPE), TP._tol(key, model, TP._RESPONSE_SLOPE)
    moved = 0.0
    for p, (a, b) in enumerate(pairs):
        va, vb = valid1[cols.index(a)], valid1[cols.index(b)]
        assert torch.equal(valid[p], va[:, None] & vb[None, :])
        assert torch.equal(counts[p].sum(1), counts1[cols.index(a)])
        assert torch.equal(counts[p].sum(0), counts1[cols.index(b)])
        ia, ib = _some(torch.nonzero(va).reshape(-1)), _some(torch.nonzero(vb).reshape(-1))
        want_raw, want_resp = _rescored2(model, X, a, b, ia.tolist(), ib.tolist())
        err_raw = (raw[p][ia][:, ib] - want_raw.mean(2)).abs().max().item()
        err_resp = (resp[p][ia][:, ib] - want_resp.mean(2)).abs().max().item()
        print(f"{key} pair ({a}, {b}) of {len(ia)} x {len(ib)} bins: raw {err_raw:.3e} <= {tol_raw:.3e}, "
              f"response {err_resp:.3e} <= {tol_resp:.3e}")
        assert err_raw <= tol_raw and err_resp <= tol_resp
        moved = max(moved, (raw[p][ia][:, ib].amax((0, 1)) - raw[p][ia][:, ib].amin((0, 1))).max().item())
    assert moved > 1e-3                                             # the surfaces are not flat


def test_rows_blocks_and_errors(monkeypatch):
    _, scored, vec, model = TP._fit("xgb")
    X = scored[vec.name].values
    pairs = _pairs_of(model, int(X.shape[1]))
    rows = torch.tensor([5, 17, 17, 250])
    learner, state = model.learner, model.state
    v, valid, counts = learner.partial_dependence_pairs(state, X, pairs, rows=rows, scale="raw")
    assert counts.sum((1, 2)).tolist() == [4] * 3 and torch.equal(v[..., 0], -v[..., 1])
    resp = learner.partial_dependence_pairs(state, X, pairs, scale="response")[0]
    from transmogrifai_amd.models import trees as TR
    monkeypatch.setattr(TR, "PD_ICE_BLOCK_BYTES", 7 * len(pairs) * valid.shape[1] ** 2 * 8)    # blocks of 7 rows
    blocked = learner.partial_dependence_pairs(state, X, pairs, scale="response")[0]
    assert (blocked - resp).abs().max().item() <= 1e-12
    with pytest.raises(ValueError, match="scale"):
        learner.partial_dependence_pairs(state, X, pairs, scale="logit")
    with pytest.raises(ValueError, match="outside"):
        learner.partial_dependence_pairs(state, X, [(0, int(X.shape[1]))])
    with pytest.raises(ValueError, match="different"):
        learner.partial_dependence_pairs(state, X, [(1, 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["xgb3", "rfreg"])
def test_learner_surfaces_on_the_device(key):
    """The same model on a device matrix. The kernel's sums are the host twin's integers (bitwise, see
    tests/test_forest_pd_pairs_gpu.py); the bounds after them are those of
    ``test_partial_dependence.test_learner_partial_dependence_on_the_device``: ``4 * 2^-53 M`` on the raw scale,
    ``1e-12`` through the device's exp."""
    _, scored, vec, model = TP._fit(key)
    X = scored[vec.name].values
    pairs = _pairs_of(model, int(X.shape[1]))
    rows = torch.arange(0, 300, 2)
    for scale in ("raw", "response"):
        host = model.learner.partial_dependence_pairs(model.state, X, pairs, rows=rows, scale=scale)
        dev = model.learner.partial_dependence_pairs(model.state, X.to("cuda"), pairs, rows=rows.to("cuda"),
                                                     scale=scale)
        assert all(t.is_cuda for t in dev)
        assert torch.equal(dev[1].cpu(), host[1]) and torch.equal(dev[2].cpu(), host[2])
        M = host[0].abs().max().item() + abs(float(model.state.get("base_margin", 0.0)))
        err = (dev[0].cpu() - host[0]).abs().max().item()
        print(f"{key} {scale}: device - host {err:.3e}")
        assert err <= (4 * 2.0 ** -53 * M if scale == "raw" else 1e-12)


def test_base_learner_has_no_partial_dependence_pairs():
    from transmogrifai_amd.models.base import Learner
    with pytest.raises(NotImplementedError, match="tree learners"):
        Learner().partial_dependence_pairs({}, torch.zeros(1, 2), [(0, 1)])


# -------------------------------------------------------------------------------------------------- H-statistic
def _engine_h(forest, Xb, pair, NB, **kw):
    """H of the pair on the raw scale through the engine: mean surface, mean curves, the rows' own bins."""
    X = torch.from_numpy(Xb)
    n = Xb.shape[0]
    surface = te.forest_partial_dependence_pairs(forest, X, [pair], NB, **kw)[0] / n
    curves = te.forest_partial_dependence(forest, X, list(pair), NB, **kw) / n
    xa, xb = (torch.from_numpy(Xb[:, c].astype(np.int64)) for c in pair)
    counts = torch.bincount(xa * NB + xb, minlength=NB * NB).reshape(NB, NB)
    return h_statistic(surface, counts, curves[0], curves[1], counts.sum(1), counts.sum(0))


def _numpy_h(surface, curve_a, curve_b, Xb, pair, NB):
    """The formula of the issue in NumPy: ``surface [NB, NB, C]`` and the curves ``[NB, C]`` are means over rows."""
    w = np.zeros((NB, NB))
    np.add.at(w, (Xb[:, pair[0]].astype(np.int64), Xb[:, pair[1]].astype(np.int64)), 1.0)
    wa, wb = w.sum(1), w.sum(0)
    f_ab = surface - np.einsum("ij,ijc->c", w, surface) / w.sum()
    f_a = curve_a - wa @ curve_a / wa.sum()
    f_b = curve_b - wb @ curve_b / wb.sum()
    num = np.einsum("ij,ijc->c", w, (f_ab - f_a[:, None] - f_b[None, :]) ** 2)
    den = np.einsum("ij,ijc->c", w, f_ab ** 2)
    return np.where(den > 0, np.sqrt(num / np.where(den > 0, den, 1.0)), 0.0)


def test_h_is_zero_when_no_tree_holds_both_columns():
    leaves = [(0, 0, -1, -1)]
    t1 = L._hand([(0, 10, 1, 2), (0, 4, 3, 4)] + leaves * 3, [0, 0, 3, 1, 2])
    t2 = L._hand([(1, 20, 1, 2)] + leaves + [(1, 25, 3, 4)] + leaves * 2, [0, -1, 0, 5, 0.5])
    t3 = L._hand([(2, 7, 1, 2)] + leaves * 2, [0, 9, -9])
    forest = Forest.concat([t1, t2, t3])
    Xb = np.random.default_rng(61).integers(0, O.B, (67, 3)).astype(np.uint8)
    h = _engine_h(forest, Xb, (0, 1), O.B)
    assert tuple(h.shape) == (1,) and 0.0 <= h.item() <= 1e-9
    assert _engine_h(forest, Xb, (2, 1), O.B).item() <= 1e-9


def test_h_is_one_for_an_xor_tree_on_a_product_grid():
    leaves = [(0, 0, -1, -1)]
    forest = L._hand([(0, 15, 1, 2), (1, 15, 3, 4), (1, 15, 5, 6)] + leaves * 4, [0, 0, 0, 1, -1, -1, 1])
    Xb = np.asarray([(i, j) for i in range(O.B) for j in range(O.B)], np.uint8)
    assert abs(_engine_h(forest, Xb, (0, 1), O.B).item() - 1.0) <= 1e-12
    flat = L._hand(leaves, [3.0])                                   # a flat surface: the denominator is 0
    assert _engine_h(flat, Xb, (0, 1), O.B).item() == 0.0


@pytest.mark.parametrize("name", ["chain12_missing", "mixed_depths_k3"])
def test_h_of_a_mixed_case_equals_the_formula_on_the_oracle(name):
    """The engine's surfaces and curves agree with the oracle's within ``tolerance`` (about 1e-12 here, on values of
    order 1), and H is a ratio of weighted sums of squares of them: 1e-9 leaves three digits for the ratio's
    conditioning and is far below any error of the formula itself."""
    forest, Xb, pairs, NB, kw, want = O2.case(name)
    assert "rows" not in kw
    pair = pairs[0]
    curves = O.ice(forest, Xb, list(pair), NB, **kw).mean(0)
    ref = _numpy_h(want[:, 0].mean(0), curves[0], curves[1], Xb, pair, NB)
    got = _engine_h(forest, Xb, pair, NB, **kw).numpy()
    print(f"{name}: H {got} formula {ref}")
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-9
    assert 1e-3 < ref.max() < 1 - 1e-3                              # neither additive nor pure interaction


# ----------------------------------------------------------------------------------------------- workflow level
def test_default_pairs_are_the_pairs_of_the_top_contributions():
    wf, scored, vec, model = TP._fit("xgb")
    X = scored[vec.name].values
    res = wf.partial_dependence_pairs(top_k=3)
    assert isinstance(res, PairDependence) and res.scale == "response" and res.rows == 300
    assert res.learner == "OpXGBoostClassifier"
    pairs = _pairs_of(model, int(X.shape[1]))
    assert [(p.a.index, p.b.index) for p in res.pairs] == pairs
    hist = scored[vec.name].metadata.column_history()
    values, valid, counts = model.learner.partial_dependence_pairs(model.state, X, pairs, scale="response")
    for k, p in enumerate(res.pairs):
        assert p.a.name == hist[p.a.index]["columnName"] and p.b.parentFeature == hist[p.b.index]["parentFeatureName"]
        ia, ib = [g.bin for g in p.a.grid], [g.bin for g in p.b.grid]
        assert torch.equal(valid[k], torch.zeros_like(valid[k]).index_put_(
            (torch.tensor(ia)[:, None], torch.tensor(ib)[None, :]), torch.tensor(True)))
        assert len(p.values) == len(ia) and all(len(line) == len(ib) for line in p.values)
        assert sum(sum(line) for line in p.counts) == 300
        assert [sum(line) for line in p.counts] == [g.count for g in p.a.grid]
        assert p.values[0][1] == values[k, ia[0], ib[1]].tolist() and p.counts[1][0] == int(counts[k, ia[1], ib[0]])
        assert all(abs(sum(cell) - 1) < 1e-12 for line in p.values for cell in line)
        assert len(p.h_statistic) == 2 and all(0.0 <= h <= 1.0 + 1e-12 for h in p.h_statistic)
    named = wf.partial_dependence_pairs(pairs=[(pairs[0][1], hist[pairs[0][0]]["columnName"])], scale="raw")
    assert [(p.a.index, p.b.index) for p in named.pairs] == [(pairs[0][1], pairs[0][0])]
    assert named.pairs[0].values == [list(line) for line in zip(*wf.partial_dependence_pairs(
        pairs=[pairs[0]], scale="raw").pairs[0].values)]


def test_a_raw_feature_name_of_several_columns_is_a_value_error():
    wf, scored, vec, _ = TP._fit("rf2")
    hist = scored[vec.name].metadata.column_history()
    derived = [h["index"] for h in hist if "c" in h["parentFeatureOrigins"]]
    assert len(derived) >= 3
    with pytest.raises(ValueError, match=str(derived).replace("[", r"\[").replace("]", r"\]")):
        wf.partial_dependence_pairs(pairs=[("c", 0)])
    with pytest.raises(ValueError, match="nothing_like_this"):
        wf.partial_dependence_pairs(pairs=[(0, "nothing_like_this")])
    with pytest.raises(ValueError, match="different"):
        wf.partial_dependence_pairs(pairs=[(0, 0)])
    with pytest.raises(ValueError, match="2-tuple"):
        wf.partial_dependence_pairs(pairs=[(0, 1, 2)])


def test_json_round_trip():
    wf, _, _, _ = TP._fit("rfreg")
    res = wf.partial_dependence_pairs(top_k=3)
    text = res.to_json()
    d = json.loads(text, parse_constant=lambda s: pytest.fail(f"non-standard JSON constant {s}"))
    assert d["pairs"][0]["a"]["grid"][0]["lower"] == "-Infinity" and "row_ids" not in d
    assert len(d["pairs"]) == 3 and len(d["pairs"][0]["h_statistic"]) == 1
    back = PairDependence.from_json(text)
    assert back.pairs == res.pairs and back.to_json_dict() == res.to_json_dict()


def test_the_seed_decides_the_sample():
    wf, _, _, _ = TP._fit("gbt")
    a, b, c = (wf.partial_dependence_pairs(top_k=2, sample=100, seed=s) for s in (3, 3, 4))
    assert a.rows == 100 and a.row_ids.numel() == 100 and a.row_ids.unique().numel() == 100
    assert torch.equal(a.row_ids, b.row_ids) and a.to_json_dict() == b.to_json_dict()
    assert not torch.equal(a.row_ids, c.row_ids) and a.to_json_dict() != c.to_json_dict()
    assert wf.partial_dependence_pairs(top_k=2, sample=None).row_ids is None
    ref = wf.partial_dependence(top_k=2, sample=100, seed=3)
    assert torch.equal(a.row_ids, ref.row_ids)                      # the sample of partial_dependence


def test_a_linear_model_is_a_value_error():
    wf, _, _, _ = TP._fit("lr")
    with pytest.raises(ValueError, match="OpLogisticRegression"):
        wf.partial_dependence_pairs()
