"""``Learner.partial_dependence`` of the tree learners and ``OpWorkflowModel.partial_dependence`` on the seven small
fits of tests/test_record_insights_loco_paths.py (rebuilt here), against rescoring: the column set to a value inside
each of its bins and the model's own ``predict`` averaged over the rows.

Bound. ``partial_dependence`` is fp64-exact up to the fixed-point quantum; ``predict`` sums T fp32 terms, so the two
agree within that file's ``tol = 2 L T 2^-23 S`` with ``S = sum_t |w_t| max |value_t|`` and ``L`` the bound of the
slope of the map from the tree sums to the compared column: 1 for the raw scores (``1 / num_trees`` for the RF
regressor's prediction); for the response 1/4 for XGBoost's sigmoid, 1/2 for GBT's ``sigmoid(2 m)`` and for the
softmax (row sums of its Jacobian are ``2 p (1 - p)``), 1 for the regressors, and ``(1 + K) / num_trees`` for the
forests' vote shares ``r_i / sum r`` (``sum r = num_trees``: ``|d p_i| <= (|d r_i| + p_i sum_j |d r_j|) / sum r``).
The mean over the rows is within the bound of each row."""
import json

import numpy as np
import pytest
import torch

import forest_loco_oracle as O
from transmogrifai_amd.features import types as T
from transmogrifai_amd.insights.partial_dependence import PartialDependence
from transmogrifai_amd.testkit.feature_builder import TestFeatureBuilder

_FITS = {}
_MODELS = {
    "rf2": ("OpRandomForestClassifier", 2, dict(num_trees=8, max_depth=4)),
    "rf3": ("OpRandomForestClassifier", 3, dict(num_trees=8, max_depth=4)),
    "rfreg": ("OpRandomForestRegressor", 0, dict(num_trees=8, max_depth=4)),
    "gbt": ("OpGBTClassifier", 2, dict(max_iter=6, max_depth=3)),
    "xgb": ("OpXGBoostClassifier", 2, dict(num_round=8, max_depth=4)),
    "xgb3": ("OpXGBoostClassifier", 3, dict(num_round=6, max_depth=3, objective="multi:softprob")),
    "xgbreg": ("OpXGBoostRegressor", 0, dict(num_round=8, max_depth=3)),
    "lr": ("OpLogisticRegression", 2, {}),
}
_RAW_SLOPE = {"rf2": 1.0, "rf3": 1.0, "rfreg": 1 / 8, "gbt": 1.0, "xgb": 1.0, "xgb3": 1.0, "xgbreg": 1.0}
_RESPONSE_SLOPE = {"rf2": 3 / 8, "rf3": 4 / 8, "rfreg": 1 / 8, "gbt": 0.5, "xgb": 0.25, "xgb3": 0.5, "xgbreg": 1.0}
_OUT = {"rf2": 2, "rf3": 3, "rfreg": 1, "gbt": 2, "xgb": 2, "xgb3": 3, "xgbreg": 1}
TREE_KEYS = [k for k in _MODELS if k != "lr"]
SEED = 5


def _fit(key, n=300):
    """A real column, a picklist, hashed free text and a date (about 300 rows), and one model on top, fitted once:
    (workflow model, scored dataset, vector feature, fitted model stage)."""
    if key in _FITS:
        return _FITS[key]
    from transmogrifai_amd.dsl import transmogrify
    from transmogrifai_amd.models import linear as LN, trees as TR
    from transmogrifai_amd.workflow.workflow import OpWorkflow
    cls, classes, params = _MODELS[key]
    rng = np.random.default_rng(SEED)
    a = rng.normal(size=n)
    c = rng.choice(["x", "y", "z"], size=n)
    words = [f"w{i}" for i in range(12)]
    txt = [" ".join(rng.choice(words, size=rng.integers(1, 4))) for _ in range(n)]
    hour = rng.integers(0, 24, size=n)
    dts = [int(1.5e12 + rng.integers(0, 400) * 86_400_000 + h * 3_600_000) for h in hour]
    z = a + (c == "x") + np.array([1.5 * ("w1" in t.split()) - 1.0 * ("w2" in t.split()) for t in txt]) \
        + 1.5 * np.cos(2 * np.pi * hour / 24) + rng.normal(scale=0.3, size=n)
    y = z if classes == 0 else np.digitize(z, np.quantile(z, np.linspace(0, 1, classes + 1)[1:-1])).astype(float)
    ds, (lab, fa, fc, ft, fd) = TestFeatureBuilder.of(("y", T.RealNN, list(y)), ("a", T.Real, list(a)),
                                                      ("c", T.PickList, list(c)), ("t", T.Text, txt),
                                                      ("d", T.DateTime, dts), response="y")
    vec = transmogrify([fa, fc, ft, fd])
    pred = getattr(TR if hasattr(TR, cls) else LN, cls)(**params).set_input(lab, vec).get_output()
    wf_model = OpWorkflow().set_result_features(pred, vec).set_input_dataset(ds).train()
    scored = wf_model.score(keep_intermediate_features=True)
    _FITS[key] = (wf_model, scored, vec, wf_model.get_origin_stage_of(pred))
    return _FITS[key]


def _top_columns(model, d, k):
    c = np.abs(np.asarray(model.learner.feature_contributions(model.state, d), np.float64))
    c = c.sum(0) if c.ndim > 1 else c
    return [int(i) for i in np.argsort(-c, kind="stable")[:k] if c[i] > 0]


def _bin_value(spec, c, b):
    """A value that ``quantize`` puts into bin ``b`` of column ``c``: threshold ``b`` itself (bins are ``(lower,
    upper]``; the matrix and the thresholds are cast to the same type), above the last threshold for the last
    bin, NaN for the missing bin."""
    nt = int(spec.n_thresh[c])
    if spec.missing_bin >= 0 and b == spec.missing_bin:
        return float("nan")
    if b < nt:
        return float(spec.thresholds[c, b])
    if nt == 0:
        return 0.0
    v = float(spec.thresholds[c, nt - 1])
    return v + max(1.0, abs(v))


def _rescored(model, X, c, bins):
    """``predict`` on copies of ``X`` with column ``c`` at a value inside each bin: (raw, response) float64
    ``[len(bins), n, C']``."""
    spec = model.learner._forest(model.state)[1]
    n = X.shape[0]
    big = X.repeat(len(bins), 1)
    for k, b in enumerate(bins):
        big[k * n:(k + 1) * n, c] = _bin_value(spec, c, int(b))
    pred, raw, prob = model.learner.predict(model.state, big)
    raw = (raw if raw.shape[1] > 0 else pred.reshape(-1, 1)).to(torch.float64)
    resp = (prob if prob.shape[1] > 0 else pred.reshape(-1, 1)).to(torch.float64)
    return raw.reshape(len(bins), n, -1), resp.reshape(len(bins), n, -1)


def _tol(key, model, slope):
    forest = model.learner._forest(model.state)[0]
    w = np.asarray(model.state["tree_weights"], np.float32) if "tree_weights" in model.state else None
    return 2 * slope[key] * forest.n_trees * 2.0 ** -23 * O.magnitude(forest, w)


# ------------------------------------------------------------------------------------------------ learner level
@pytest.mark.parametrize("key", TREE_KEYS)
def test_learner_partial_dependence_matches_rescoring(key):
    _, scored, vec, model = _fit(key)
    X = scored[vec.name].values
    n, d = int(X.shape[0]), int(X.shape[1])
    learner, state = model.learner, model.state
    spec = learner._forest(state)[1]
    cols = _top_columns(model, d, 3)
    assert len(cols) == 3
    raw, valid, counts, none = learner.partial_dependence(state, X, cols, scale="raw")
    resp, valid2, counts2, ice = learner.partial_dependence(state, X, cols, scale="response", ice=True)
    NB = int(spec.B)
    assert none is None and tuple(raw.shape) == (3, NB, _OUT[key]) and tuple(resp.shape) == (3, NB, _OUT[key])
    assert tuple(ice.shape) == (n, 3, NB, _OUT[key]) and torch.equal(valid, valid2) and torch.equal(counts, counts2)
    assert raw.dtype == torch.float64 and valid.dtype == torch.bool
    assert counts.sum(1).tolist() == [n] * 3                        # every row sits in one bin of every column
    assert not counts[~valid].any()
    tol_raw, tol_resp = _tol(key, model, _RAW_SLOPE), _tol(key, model, _RESPONSE_SLOPE)
    moved = 0.0
    for q, c in enumerate(cols):
        bins = torch.nonzero(valid[q]).reshape(-1).tolist()
        want_bins = list(range(int(spec.n_bins[c]))) + ([spec.missing_bin] if spec.missing_bin >= 0 else [])
        assert bins == sorted(set(want_bins))
        want_raw, want_resp = _rescored(model, X, c, bins)
        err_raw = (raw[q, bins] - want_raw.mean(1)).abs().max().item()
        err_resp = (resp[q, bins] - want_resp.mean(1)).abs().max().item()
        err_ice = (ice[:, q, bins] - want_resp.transpose(0, 1)).abs().max().item()
        print(f"{key} column {c}: raw {err_raw:.3e} <= {tol_raw:.3e}, response {err_resp:.3e} / ice {err_ice:.3e} "
              f"<= {tol_resp:.3e}")
        assert err_raw <= tol_raw and err_resp <= tol_resp and err_ice <= tol_resp
        moved = max(moved, (raw[q, bins].max(0).values - raw[q, bins].min(0).values).max().item())
    assert moved > 1e-3                                             # the curves are not flat
    assert (resp - ice.mean(0)).abs().max().item() <= 1e-12


def test_rows_and_raw_ice():
    _, scored, vec, model = _fit("xgb")
    X = scored[vec.name].values
    cols = _top_columns(model, int(X.shape[1]), 2)
    rows = torch.tensor([5, 17, 17, 250])
    v, valid, counts, ice = model.learner.partial_dependence(model.state, X, cols, rows=rows, scale="raw", ice=True)
    assert counts.sum(1).tolist() == [4, 4] and ice.shape[0] == 4
    assert (v - ice.mean(0)).abs().max().item() <= 1e-12
    assert torch.equal(ice[..., 0], -ice[..., 1]) and torch.equal(ice[1], ice[2])
    with pytest.raises(ValueError, match="scale"):
        model.learner.partial_dependence(model.state, X, cols, scale="logit")
    with pytest.raises(ValueError, match="outside"):
        model.learner.partial_dependence(model.state, X, [int(X.shape[1])])


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["xgb3", "rfreg"])
def test_learner_partial_dependence_on_the_device(key):
    """The same model on a device matrix. The kernel's sums are the host twin's integers (bitwise, see
    tests/test_forest_pd_gpu.py); after them the raw scale takes at most three fp64 operations on values within
    ``M = max |value| + |base_margin|`` (the division by the row count, which the device does as a multiplication
    by the rounded reciprocal: two roundings; the base margin), each rounding by at most ``2^-53 M``: ``4 * 2^-53
    M`` bounds the difference. The response goes through the device's exp: ``1e-12`` as for the ICE mean above."""
    _, scored, vec, model = _fit(key)
    X = scored[vec.name].values
    cols = _top_columns(model, int(X.shape[1]), 3)
    rows = torch.arange(0, 300, 2)
    for scale in ("raw", "response"):
        host = model.learner.partial_dependence(model.state, X, cols, rows=rows, scale=scale, ice=True)
        dev = model.learner.partial_dependence(model.state, X.to("cuda"), cols, rows=rows.to("cuda"), scale=scale,
                                               ice=True)
        assert all(t.is_cuda for t in dev)
        assert torch.equal(dev[1].cpu(), host[1]) and torch.equal(dev[2].cpu(), host[2])
        for d, h in ((dev[0], host[0]), (dev[3], host[3])):
            M = h.abs().max().item() + abs(float(model.state.get("base_margin", 0.0)))
            err = (d.cpu() - h).abs().max().item()
            print(f"{key} {scale}: device - host {err:.3e}")
            assert err <= (4 * 2.0 ** -53 * M if scale == "raw" else 1e-12)


def test_base_learner_has_no_partial_dependence():
    from transmogrifai_amd.models.base import Learner
    with pytest.raises(NotImplementedError, match="tree learners"):
        Learner().partial_dependence({}, torch.zeros(1, 1), [0])


# ----------------------------------------------------------------------------------------------- workflow level
def test_default_columns_are_the_top_contributions():
    wf, scored, vec, model = _fit("xgb")
    d = int(scored[vec.name].values.shape[1])
    res = wf.partial_dependence(top_k=3)
    assert isinstance(res, PartialDependence) and res.scale == "response" and res.rows == 300
    assert res.learner == "OpXGBoostClassifier"
    assert [c.index for c in res.columns] == _top_columns(model, d, 3)
    hist = scored[vec.name].metadata.column_history()
    spec = model.learner._forest(model.state)[1]
    for c in res.columns:
        assert c.name == hist[c.index]["columnName"] and c.parentFeature == hist[c.index]["parentFeatureName"]
        pts = [g for g in c.grid if not g.missing]
        assert len(pts) == int(spec.n_bins[c.index]) and sum(g.count for g in c.grid) == 300
        assert pts[0].lower == float("-inf") and pts[-1].upper == float("inf")
        assert all(a.upper == b.lower for a, b in zip(pts, pts[1:]))
        assert [g.missing for g in c.grid].count(True) == (1 if spec.missing_bin >= 0 else 0)
        assert all(len(g.values) == 2 and abs(sum(g.values) - 1) < 1e-12 for g in c.grid)
    values, _, _, _ = model.learner.partial_dependence(model.state, scored[vec.name].values,
                                                       [c.index for c in res.columns], scale="response")
    assert res.columns[0].grid[0].values == values[0, res.columns[0].grid[0].bin].tolist()


def test_raw_feature_name_expands_to_its_columns():
    wf, scored, vec, _ = _fit("rf2")
    hist = scored[vec.name].metadata.column_history()
    derived = [h["index"] for h in hist if "c" in h["parentFeatureOrigins"]]
    assert len(derived) >= 3
    res = wf.partial_dependence(features=["c", 0], scale="raw")
    assert [c.index for c in res.columns] == derived + ([0] if 0 not in derived else [])
    assert {tuple(c.parentFeature) for c in res.columns[:len(derived)]} == {("c",)}
    assert any(c.indicatorValue for c in res.columns)
    with pytest.raises(ValueError, match="nothing_like_this"):
        wf.partial_dependence(features=["nothing_like_this"])


def test_json_round_trip():
    wf, _, _, _ = _fit("rfreg")
    res = wf.partial_dependence(top_k=2, ice=True)
    text = res.to_json()
    d = json.loads(text, parse_constant=lambda s: pytest.fail(f"non-standard JSON constant {s}"))
    assert d["columns"][0]["grid"][0]["lower"] == "-Infinity" and "ice" not in d
    back = PartialDependence.from_json(text)
    assert back.columns == res.columns and back.to_json_dict() == res.to_json_dict()
    assert back.ice is None and res.ice is not None
    assert tuple(res.ice.shape)[:2] == (300, 2) and res.ice.shape[3] == 1
    mean = res.ice.mean(0)
    for q, c in enumerate(res.columns):
        for g in c.grid:
            assert abs(mean[q, g.bin, 0].item() - g.values[0]) <= 1e-12


def test_the_seed_decides_the_sample():
    wf, _, _, _ = _fit("gbt")
    a, b, c = (wf.partial_dependence(top_k=2, sample=100, seed=s) for s in (3, 3, 4))
    assert a.rows == 100 and a.row_ids.numel() == 100 and a.row_ids.unique().numel() == 100
    assert torch.equal(a.row_ids, b.row_ids) and a.to_json_dict() == b.to_json_dict()
    assert not torch.equal(a.row_ids, c.row_ids) and a.to_json_dict() != c.to_json_dict()
    assert wf.partial_dependence(top_k=1, sample=None).row_ids is None


def test_a_linear_model_is_a_value_error():
    wf, _, _, _ = _fit("lr")
    with pytest.raises(ValueError, match="OpLogisticRegression"):
        wf.partial_dependence()
