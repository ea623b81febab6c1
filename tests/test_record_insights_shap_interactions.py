"""RecordInsightsSHAPInteractions: exact SHAP interaction record insights over plain, text-hash-group and
date-group columns.

Bounds: main effects + pair effects + bias equal the learner's raw prediction to the fp32 summation bound of the
predictor, ``(T + 2) * 2^-24 * S`` with ``S = sum_t |w_t| max_node |value_t|`` (the bound of the
``RecordInsightsSHAP`` tests); folding only adds fp64 numbers, ``1e-12 * S``; device and host agree to
``1e-9 * S`` (both fp64)."""
import json

import numpy as np
import pytest
import torch

from test_record_insights_shap import _fit_mixed, _magnitude, _raw
from transmogrifai_amd.stages.insights.record_insights import (RecordInsightsSHAP, RecordInsightsSHAPInteractions,
                                                                parse_interaction_insights)

ALL = 1 << 20          # a top_k no record reaches: every pair is reported


def _rendered(stage, ds):
    return stage.transform(ds)[stage.get_output().name].to_list()


def _text_columns(hist):
    return [h["index"] for h in hist if "Text" in {t.rsplit(".", 1)[-1] for t in h["parentFeatureType"]}
            and h["indicatorValue"] is None and h["descriptorValue"] is None]


@pytest.mark.parametrize("key", ["rf", "xgb", "xgb3"])
def test_main_effects_pair_effects_and_bias_equal_the_raw_prediction(key):
    scored, vec, model = _fit_mixed(key)[:3]
    X = scored[vec.name].values
    st = RecordInsightsSHAPInteractions(model, top_k=ALL).set_input(vec)
    maps = [parse_interaction_insights(m) for m in _rendered(st, scored)]
    want = _raw(model, X)
    C = want.shape[1]
    main = st.main_effects(X)
    bias = st.bias(X)
    assert main.shape[0] == X.shape[0] and main.shape[2] == C and bias.shape == (C,)
    S, n_trees = _magnitude(model)
    worst = 0.0
    for i, m in enumerate(maps):
        tot = bias + main[i].sum(0)
        for v in m.values():
            assert [c for c, _ in v] == list(range(C))
            tot = tot + torch.as_tensor([x for _, x in v], dtype=torch.float64)
        worst = max(worst, (tot - want[i]).abs().max().item())
    print(key, "additivity error / S =", worst / S, "bound", (n_trees + 2) * 2.0 ** -24)
    assert worst <= (n_trees + 2) * 2.0 ** -24 * S
    assert any(len(m) > 2 for m in maps)
    # the main effects and the pairs of a candidate are its RecordInsightsSHAP attribution
    phi = model.learner.shap_values(model.state, X)[0]
    assert (main.sum(1) + sum_pairs(maps, C) - phi[:, :-1].sum(1)).abs().max().item() <= 1e-9 * S


def sum_pairs(maps, C):
    out = torch.zeros(len(maps), C, dtype=torch.float64)
    for i, m in enumerate(maps):
        for v in m.values():
            out[i] += torch.as_tensor([x for _, x in v], dtype=torch.float64)
    return out


def test_text_group_pairs_fold_into_its_main_effect_and_its_pairs_sum_its_members():
    scored, vec, model = _fit_mixed("xgb")[:3]
    X = scored[vec.name].values
    hist = scored[vec.name].metadata.column_history()
    st = RecordInsightsSHAPInteractions(model, top_k=ALL).set_input(vec)
    rendered = _rendered(st, scored)
    Phi, used = model.learner.shap_interaction_values(model.state, X)
    text = _text_columns(hist)
    slots = [u for u, c in enumerate(used) if int(c) in text]
    assert len(slots) > 1, "the model splits on fewer than two text-hash columns"
    S, _ = _magnitude(model)
    # candidates: plain used columns in column order, then the groups in order of their first used column
    plan_cand = st._shap_plan(hist, used, X.device)[0]
    tc = int(plan_cand[slots[0]])
    assert all(int(plan_cand[u]) == tc for u in slots)
    within = Phi[:, slots][:, :, slots].sum((1, 2))
    assert (st.main_effects(X)[:, tc] - within).abs().max().item() <= 1e-12 * S
    slot_of = {int(c): u for u, c in enumerate(used)}
    seen = 0
    for i, m in enumerate(rendered):
        for k, v in m.items():
            a, b = (h["index"] for h in json.loads(k))
            assert a < b and not (a in text and b in text)             # no pair inside the group
            if (a in text) == (b in text):
                continue
            t, p = (a, b) if a in text else (b, a)
            active = [j for j in text if X[i, j] != 0]
            assert t == (active[0] if active else int(used[slots[0]]))
            if p not in slot_of or _in_a_group(st, hist, p):
                continue
            member_sum = 2 * Phi[i, slots, slot_of[p]].sum(0)
            assert abs(json.loads(v)[1][1] - member_sum[1].item()) <= 1e-12 * S
            seen += 1
    assert seen > 0


def _in_a_group(st, hist, col):
    return any(col in cols for cols in st._groups(hist).values())


@pytest.mark.parametrize("strategy", ["abs", "positive and negative"])
@pytest.mark.parametrize("key", ["xgb", "xgb3"])
def test_top_k_selection(key, strategy):
    scored, vec, model = _fit_mixed(key)[:3]
    sub = scored.take(torch.arange(80))
    X = sub[vec.name].values
    mk = lambda k: RecordInsightsSHAPInteractions(model, top_k=k, top_k_strategy=strategy).set_input(vec)  # noqa: E731
    full = [parse_interaction_insights(m) for m in _rendered(mk(ALL), sub)]
    top = [parse_interaction_insights(m) for m in _rendered(mk(3), sub)]
    pred = model.learner.predict(model.state, X)[0]
    assert any(len(f) > 3 for f in full)
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


def test_pair_effect_is_twice_the_interaction_value():
    """A pair of plain columns: the reported effect is ``Phi_ab + Phi_ba`` of the learner's matrix."""
    scored, vec, model = _fit_mixed("xgb")[:3]
    X = scored[vec.name].values
    hist = scored[vec.name].metadata.column_history()
    st = RecordInsightsSHAPInteractions(model, top_k=ALL).set_input(vec)
    Phi, used = model.learner.shap_interaction_values(model.state, X)
    slot_of = {int(c): u for u, c in enumerate(used)}
    S, _ = _magnitude(model)
    seen = 0
    for i, m in enumerate(_rendered(st, scored)[:100]):
        for k, v in m.items():
            a, b = (h["index"] for h in json.loads(k))
            if _in_a_group(st, hist, a) or _in_a_group(st, hist, b):
                continue
            want = Phi[i, slot_of[a], slot_of[b]] + Phi[i, slot_of[b], slot_of[a]]
            assert abs(json.loads(v)[1][1] - want[1].item()) <= 1e-12 * S
            seen += 1
    assert seen > 0


def test_transform_row_matches_the_column_path():
    scored, vec, model = _fit_mixed("rf")[:3]
    st = RecordInsightsSHAPInteractions(model, top_k=5).set_input(vec)
    out = _rendered(st, scored)
    X = scored[vec.name].values.numpy()
    assert any(out)
    for i in (0, 7, 123, 299):
        assert st.transform_row(X[i]) == out[i]


def test_checkpoint_round_trip(tmp_path):
    from transmogrifai_amd.workflow.workflow import OpWorkflow, OpWorkflowModel
    scored, vec, model, ds, wf_model, pred = _fit_mixed("xgb3")
    ins = RecordInsightsSHAPInteractions(model, top_k=4, top_k_strategy="positive and negative") \
        .set_input(vec).get_output()
    m2 = OpWorkflow().set_result_features(ins, pred).with_model_stages(wf_model).set_input_dataset(ds).train()
    before = m2.score()[ins.name].to_list()
    assert any(before)
    m2.save(str(tmp_path / "m"))
    loaded = OpWorkflowModel.load(str(tmp_path / "m")).set_input_dataset(ds)
    assert loaded.score()[ins.name].to_list() == before


def test_model_without_interaction_values_is_a_value_error():
    from transmogrifai_amd.models.linear import OpLogisticRegression
    scored, vec, model, ds, wf_model, pred = _fit_mixed("rf")
    lab = [f for f in wf_model.raw_features if f.name == "y"][0]
    lr = OpLogisticRegression().set_input(lab, vec).fit(scored)
    with pytest.raises(ValueError, match="RecordInsightsLOCO"):
        RecordInsightsSHAPInteractions(lr, top_k=3).set_input(vec).transform(scored)


def test_parse_interaction_insights_inverts_the_rendering():
    scored, vec, model = _fit_mixed("xgb3")[:3]
    hist = scored[vec.name].metadata.column_history()
    st = RecordInsightsSHAPInteractions(model, top_k=6).set_input(vec)
    col = st.transform(scored)[st.get_output().name]
    index_of = {h["columnName"]: h["index"] for h in hist}
    assert len(index_of) == len(hist)
    cols, diffs = col.cols.numpy(), col.diffs.numpy()
    for i in (0, 5, 50, 299):
        parsed = parse_interaction_insights(col.row(i))
        want = {(int(a), int(b)): [(j, float(x)) for j, x in enumerate(d)]
                for (a, b), d in zip(cols[i], diffs[i]) if a >= 0}
        assert want and {(index_of[a], index_of[b]): v for (a, b), v in parsed.items()} == want
        assert all(index_of[a] < index_of[b] for a, b in parsed)
    # the stage is the parent's sibling: the same candidates, registered under its own operation name
    assert issubclass(RecordInsightsSHAPInteractions, RecordInsightsSHAP)
    assert st.operation_name == "recordInsightsSHAPInteractions"


@pytest.mark.gpu
def test_device_insights_match_the_host():
    """1,000 records on the device: the same pairs, pair effects within 1e-9 S of the host twin's."""
    from transmogrifai_amd.data.columns import VectorColumn
    from transmogrifai_amd.data.dataset import Dataset
    scored, vec, model = _fit_mixed("xgb3")[:3]
    base = scored[vec.name]
    X = base.values.repeat(4, 1)[:1000]
    S, _ = _magnitude(model)
    st = RecordInsightsSHAPInteractions(model, top_k=6).set_input(vec)
    host = st.transform(Dataset({vec.name: VectorColumn(X, base.metadata)}))[st.get_output().name]
    dev = st.transform(Dataset({vec.name: VectorColumn(X.cuda(), base.metadata)}))[st.get_output().name]
    assert dev.cols.is_cuda and len(dev) == 1000 and dev.cols.shape == host.cols.shape
    # rank by rank the selecting score column agrees; the chosen pair may differ only between pairs that tie to
    # the tolerance (``torch.topk`` orders ties differently on the two devices), and where it is the same pair
    # all its score columns agree
    tol = 1e-9 * S
    K = host.cols.shape[1]
    ex = model.learner.predict(model.state, X)[0].to(torch.long).view(-1, 1, 1).expand(-1, K, 1)
    vh, vd = host.diffs.gather(2, ex).squeeze(2), dev.diffs.cpu().gather(2, ex).squeeze(2)
    assert (vh - vd).abs().max().item() <= tol
    same = (dev.cols.cpu() == host.cols).all(2)
    near = (vh[:, :, None] - vh[:, None, :]).abs() <= tol
    tied = (near.sum(2) > 1) | (vh.abs() <= tol)
    assert (same | tied).all()
    assert ((dev.diffs.cpu() - host.diffs).abs().amax(2)[same]).max().item() <= tol
    assert dev.row(3) == dev.to("cpu").row(3)
