"""RecordInsightsSHAP: exact TreeSHAP record insights over plain, text-hash-group and date-group columns.

Bounds: the insights of a record plus the bias equal the learner's raw prediction to the fp32 summation
bound of the predictor, ``(T + 2) * 2^-24 * S`` with ``S = sum_t |w_t| max_node |value_t|``; device and host
attributions agree to ``1e-9 * S`` (both fp64)."""
import json

import numpy as np
import pytest
import torch

from transmogrifai_amd.features import types as T
from transmogrifai_amd.stages.insights.record_insights import RecordInsightsSHAP, parse_insights
from transmogrifai_amd.testkit.feature_builder import TestFeatureBuilder

_FITS = {}


def _fit_mixed(key, n=300, seed=3):
    """Real + picklist + hashed free text + a date, and one of the tree models on top (fitted once)."""
    if (key, n) in _FITS:
        return _FITS[key, n]
    from transmogrifai_amd.dsl import transmogrify
    from transmogrifai_amd.models import trees as TR
    from transmogrifai_amd.workflow.workflow import OpWorkflow
    model_cls, classes, params = {
        "rf": (TR.OpRandomForestClassifier, 2, dict(num_trees=8, max_depth=4)),
        "gbt": (TR.OpGBTClassifier, 2, dict(max_iter=5, max_depth=3)),
        "xgb": (TR.OpXGBoostClassifier, 2, dict(num_round=6, max_depth=3)),
        "xgb3": (TR.OpXGBoostClassifier, 3, dict(num_round=4, max_depth=3, objective="multi:softprob")),
        "xgbreg": (TR.OpXGBoostRegressor, 2, dict(num_round=6, max_depth=3)),
    }[key]
    rng = np.random.default_rng(seed)
    a = rng.normal(size=n)
    c = rng.choice(["x", "y", "z"], size=n)
    words = [f"w{i}" for i in range(400)]
    txt = [" ".join(rng.choice(words, size=rng.integers(1, 6))) for _ in range(n)]
    day = 86_400_000
    dts = [int(1.5e12 + rng.integers(0, 400) * day + rng.integers(0, 24) * 3_600_000) for _ in range(n)]
    z = 2 * a + (c == "x") + np.array([0.5 * ("w1" in t) for t in txt]) + rng.normal(scale=0.5, size=n)
    y = np.digitize(z, np.quantile(z, np.linspace(0, 1, classes + 1)[1:-1])).astype(float)
    ds, (lab, fa, fc, ft, fd) = TestFeatureBuilder.of(("y", T.RealNN, list(y)), ("a", T.Real, list(a)),
                                                      ("c", T.PickList, list(c)), ("t", T.Text, txt),
                                                      ("d", T.DateTime, dts), response="y")
    vec = transmogrify([fa, fc, ft, fd])
    pred = model_cls(**params).set_input(lab, vec).get_output()
    wf_model = OpWorkflow().set_result_features(pred, vec).set_input_dataset(ds).train()
    scored = wf_model.score(keep_intermediate_features=True)
    _FITS[key, n] = (scored, vec, wf_model.get_origin_stage_of(pred), ds, wf_model, pred)
    return _FITS[key, n]


def _magnitude(stage):
    """(S, T) of the fitted model's forest with its tree weights."""
    learner, state = stage.learner, stage.state
    forest = learner._forest(state)[0]
    w = np.asarray(state["tree_weights"], np.float64) if "tree_weights" in state else np.ones(forest.n_trees)
    S = sum(abs(w[t]) * np.abs(forest.value[int(forest.tree_off[t]):int(forest.tree_off[t + 1])]).max()
            for t in range(forest.n_trees))
    return float(S), forest.n_trees


def _raw(stage, X):
    pred, raw, _ = stage.learner.predict(stage.state, X)
    return (raw if raw.shape[1] > 0 else pred.reshape(-1, 1)).to(torch.float64)


def _maps(stage, ds):
    return [parse_insights(m) for m in stage.transform(ds)[stage.get_output().name].to_list()]


@pytest.mark.parametrize("key", ["rf", "gbt", "xgb", "xgb3", "xgbreg"])
def test_insights_plus_bias_equal_the_raw_prediction(key):
    scored, vec, model = _fit_mixed(key)[:3]
    X = scored[vec.name].values
    shap = RecordInsightsSHAP(model, top_k=X.shape[1] + 1).set_input(vec)
    maps = _maps(shap, scored)
    want = _raw(model, X)
    bias = shap.bias(X)
    C = want.shape[1]
    assert bias.shape == (C,) and C == {"rf": 2, "gbt": 2, "xgb": 2, "xgb3": 3, "xgbreg": 1}[key]
    S, n_trees = _magnitude(model)
    worst = 0.0
    for i, m in enumerate(maps):
        tot = bias.clone()
        for v in m.values():
            assert [c for c, _ in v] == list(range(C))
            tot += torch.as_tensor([x for _, x in v], dtype=torch.float64)
        worst = max(worst, (tot - want[i]).abs().max().item())
    print(key, "additivity error / S =", worst / S, "bound", (n_trees + 2) * 2.0 ** -24)
    assert worst <= (n_trees + 2) * 2.0 ** -24 * S
    assert any(len(m) > 2 for m in maps)


def test_text_group_insight_is_the_sum_of_its_members():
    scored, vec, model = _fit_mixed("xgb")[:3]
    X = scored[vec.name].values
    hist = scored[vec.name].metadata.column_history()
    shap = RecordInsightsSHAP(model, top_k=X.shape[1] + 1).set_input(vec)
    rendered = shap.transform(scored)[shap.get_output().name].to_list()
    phi, used = model.learner.shap_values(model.state, X)
    text = [h["index"] for h in hist if "Text" in {t.rsplit(".", 1)[-1] for t in h["parentFeatureType"]}
            and h["indicatorValue"] is None and h["descriptorValue"] is None]
    slots = [u for u, c in enumerate(used) if int(c) in text]
    assert len(slots) > 1, "the model splits on fewer than two text-hash columns"
    member_sum = phi[:, slots].sum(1)
    S, _ = _magnitude(model)
    seen = 0
    for i, m in enumerate(rendered):
        hits = [(json.loads(k)["index"], json.loads(v)) for k, v in m.items() if json.loads(k)["index"] in text]
        if not member_sum[i].any():
            assert not hits
            continue
        assert len(hits) == 1                                          # the whole group, exactly once
        col, vals = hits[0]
        active = [j for j in text if X[i, j] != 0]
        assert col == (active[0] if active else int(used[slots[0]]))
        assert abs(vals[1][1] - member_sum[i, 1].item()) <= 1e-12 * S
        seen += 1
    assert seen > 0


@pytest.mark.parametrize("strategy", ["abs", "positive and negative"])
@pytest.mark.parametrize("key", ["xgb", "xgb3"])
def test_top_k_selection(key, strategy):
    scored, vec, model = _fit_mixed(key)[:3]
    sub = scored.take(torch.arange(80))
    X = sub[vec.name].values
    full = _maps(RecordInsightsSHAP(model, top_k=X.shape[1] + 1, top_k_strategy=strategy).set_input(vec), sub)
    top = _maps(RecordInsightsSHAP(model, top_k=3, top_k_strategy=strategy).set_input(vec), sub)
    pred = model.learner.predict(model.state, X)[0]
    for i, (f, t) in enumerate(zip(full, top)):
        ex = 1 if key == "xgb" else int(pred[i])
        assert all(t[k] == f[k] for k in t)
        allv = [v[ex][1] for v in f.values()]
        got = [v[ex][1] for v in t.values()]
        if strategy == "abs":
            want = sorted(allv, key=lambda v: -abs(v))[:3]
            assert sorted(got, key=lambda v: -abs(v)) == want and got == want
        else:
            want = sorted([v for v in allv if v >= 0], reverse=True)[:3] + \
                sorted([v for v in allv if v < 0])[:3]
            assert sorted(got) == sorted(want)
            assert got == sorted(got, reverse=True)


def test_transform_row_matches_the_column_path():
    scored, vec, model = _fit_mixed("rf")[:3]
    shap = RecordInsightsSHAP(model, top_k=5).set_input(vec)
    out = shap.transform(scored)[shap.get_output().name].to_list()
    X = scored[vec.name].values.numpy()
    for i in (0, 7, 123, 299):
        assert shap.transform_row(X[i]) == out[i]


def test_checkpoint_round_trip(tmp_path):
    from transmogrifai_amd.workflow.workflow import OpWorkflow, OpWorkflowModel
    scored, vec, model, ds, wf_model, pred = _fit_mixed("xgb3")
    ins = RecordInsightsSHAP(model, top_k=4, top_k_strategy="positive and negative").set_input(vec).get_output()
    m2 = OpWorkflow().set_result_features(ins, pred).with_model_stages(wf_model).set_input_dataset(ds).train()
    before = m2.score()[ins.name].to_list()
    assert any(before)
    m2.save(str(tmp_path / "m"))
    loaded = OpWorkflowModel.load(str(tmp_path / "m")).set_input_dataset(ds)
    assert loaded.score()[ins.name].to_list() == before


def test_model_without_shap_values_is_a_value_error():
    from transmogrifai_amd.models.linear import OpLogisticRegression
    from transmogrifai_amd.models.base import Learner
    scored, vec, model, ds, wf_model, pred = _fit_mixed("rf")
    lab = [f for f in wf_model.raw_features if f.name == "y"][0]
    lr = OpLogisticRegression().set_input(lab, vec).fit(scored)
    with pytest.raises(ValueError, match="RecordInsightsLOCO"):
        RecordInsightsSHAP(lr, top_k=3).set_input(vec).transform(scored)
    with pytest.raises(NotImplementedError, match="RecordInsightsLOCO"):
        Learner().shap_values({}, scored[vec.name].values)


@pytest.mark.gpu
def test_device_insights_match_the_host():
    """5,000 records on the device: the same columns, attributions within 1e-9 S of the host twin's."""
    from transmogrifai_amd.data.columns import VectorColumn
    from transmogrifai_amd.data.dataset import Dataset
    scored, vec, model = _fit_mixed("xgb3")[:3]
    base = scored[vec.name]
    X = base.values.repeat(17, 1)[:5000]
    S, _ = _magnitude(model)
    shap = RecordInsightsSHAP(model, top_k=6).set_input(vec)
    host = shap.transform(Dataset({vec.name: VectorColumn(X, base.metadata)}))[shap.get_output().name]
    dev = shap.transform(Dataset({vec.name: VectorColumn(X.cuda(), base.metadata)}))[shap.get_output().name]
    assert dev.cols.is_cuda and len(dev) == 5000
    phi_h, _ = model.learner.shap_values(model.state, X)
    phi_d, _ = model.learner.shap_values(model.state, X.cuda())
    assert (phi_d.cpu() - phi_h).abs().max().item() <= 1e-9 * S
    # rank by rank the selecting score column agrees; the chosen column may differ only between candidates that
    # tie to the tolerance (``torch.topk`` orders ties differently on the two devices, e.g. the candidates of
    # strength 0 in the predicted class), and where it is the same column all its score columns agree
    tol = 1e-9 * S
    K = host.cols.shape[1]
    ex = model.learner.predict(model.state, X)[0].to(torch.long).view(-1, 1, 1).expand(-1, K, 1)
    vh, vd = host.diffs.gather(2, ex).squeeze(2), dev.diffs.cpu().gather(2, ex).squeeze(2)
    assert (vh - vd).abs().max().item() <= tol
    same = dev.cols.cpu() == host.cols
    near = (vh[:, :, None] - vh[:, None, :]).abs() <= tol
    tied = (near.sum(2) > 1) | (vh.abs() <= tol)
    assert (same | tied).all()
    assert ((dev.diffs.cpu() - host.diffs).abs().amax(2)[same]).max().item() <= tol
