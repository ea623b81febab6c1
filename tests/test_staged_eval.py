"""Staged evaluation of boosted forests on the CPU backend, and the held-out early stopping built on it.

The host twin ``tmog_forest_staged_eval_cpu`` (through ``tree_engine.forest_staged_eval``) is judged by the NumPy oracle
of tests/staged_eval_oracle.py in its exact regime; ``staged_eval`` of fitted models is compared with one
``learner.margin`` per prefix; a fit with ``train_test_ratio < 1`` is replayed from ``watch_split`` and the oracle's
curve of the unstopped model."""
import json

import numpy as np
import pytest
import torch

import forest_predict_oracle as FO
import staged_eval_oracle as SO
from transmogrifai_amd.models import tree_engine as te
from transmogrifai_amd.models import trees as TR
from transmogrifai_amd.models.base import FitJob

METRICS = SO.BINARY + SO.REGRESSION + SO.MULTI
# trees per stage: one stage; 16 stages (one launch), single-leaf trees among them; 17 stages of unequal size, two of
# them empty, behind a 40-deep chain: the margins are carried over a launch boundary
SHAPES = {"s1": dict(stages=(3,), shape="random", missing=False, row_list=False),
          "s16": dict(stages=(1,) * 16, shape="leaf", missing=True, row_list=True),
          "s17": dict(stages=(2, 0, 3, 1, 1, 4, 1, 2, 1, 0, 1, 5, 1, 1, 2, 1, 3), shape="chain", missing=True,
                      row_list=True)}


def run_case(c, dev="cpu", raw=True):
    rows = None if c["rows"] is None else torch.as_tensor(c["rows"]).to(dev)
    fn = te.forest_staged_eval_raw if raw else te.forest_staged_eval
    return fn(c["forest"], torch.from_numpy(c["X"]).to(dev), rows, torch.from_numpy(c["y"]).to(dev),
              stage_off=c["stage_off"], tree_col=c["tree_col"], K=c["K"], tree_weight=c["weights"], metric=c["metric"],
              margin_scale=c["scale"], base=c["base"])


def check_case(c, dev="cpu"):
    """Raw results and margins of one case against the oracle; returns them for further comparisons."""
    m, want, bound = SO.expect(c)
    got, margins = run_case(c, dev)
    n, S = m.shape[1], m.shape[0]
    assert margins.dtype == torch.float64 and tuple(margins.shape) == (n, c["K"])
    if S:
        np.testing.assert_array_equal(margins.cpu().numpy(), m[-1])
    SO.assert_raw(got.cpu().numpy(), want, bound, c["metric"])
    vals, _ = run_case(c, dev, raw=False)
    assert isinstance(vals, np.ndarray) and vals.dtype == np.float64 and vals.shape == (S,)
    if c["metric"] == "aucpr":
        from transmogrifai_amd.evaluators.metrics import binned_aupr_from_counts
        ref = binned_aupr_from_counts(torch.from_numpy(want.astype(np.int32)).to(dev)).cpu().numpy()
        np.testing.assert_array_equal(vals, ref)
    elif c["metric"] in SO.EXACT:
        np.testing.assert_array_equal(vals, SO.finish(want, n, c["metric"]))
    else:
        assert (np.abs(vals - SO.finish(want, n, c["metric"])) <= bound / max(n, 1) * (1 + 2.0 ** -50)).all()
    return got, margins


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("metric", SO.BINARY + SO.REGRESSION)
def test_host_twin_matches_oracle(metric, shape):
    check_case(SO.case(11 + len(shape) + METRICS.index(metric), metric, n=257, F=45, **SHAPES[shape]))


@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("metric", SO.MULTI)
def test_host_twin_matches_oracle_multiclass(metric, shape, K):
    check_case(SO.case(50 + K + METRICS.index(metric), metric, n=131, F=45, K=K, **SHAPES[shape]))


@pytest.mark.parametrize("metric", METRICS)
def test_no_rows_and_no_stages(metric):
    K = 3 if metric in SO.MULTI else 1
    got, margins = check_case(SO.case(3, metric, n=0, F=5, K=K, stages=(2, 1)))
    assert tuple(margins.shape) == (0, K) and not got.cpu().numpy().any()
    c = SO.case(4, metric, n=20, F=5, K=K, stages=())
    got, margins = check_case(c)
    assert got.shape[0] == 0
    np.testing.assert_array_equal(margins.numpy(), np.zeros((20, K)) + c["base"])       # the base margins, untouched


def test_margins_carry_between_calls():
    """Two calls, the second started from the margins of the first, equal one call over all stages."""
    c = SO.case(21, "logloss", n=100, F=9, stages=(2, 1, 3, 1))
    whole, m_whole = run_case(c)
    X, y = torch.from_numpy(c["X"]), torch.from_numpy(c["y"])
    kw = dict(tree_col=c["tree_col"], tree_weight=c["weights"], metric="logloss", margin_scale=c["scale"])
    a, m_a = te.forest_staged_eval_raw(c["forest"], X, None, y, stage_off=c["stage_off"][:3], base=c["base"], **kw)
    b, m_b = te.forest_staged_eval_raw(c["forest"], X, None, y, stage_off=c["stage_off"][2:], margins=m_a, **kw)
    np.testing.assert_array_equal(torch.cat([a, b]).numpy(), whole.numpy())
    np.testing.assert_array_equal(m_b.numpy(), m_whole.numpy())


def test_wrapper_validates_its_inputs():
    c = SO.case(5, "mlogloss", n=30, F=5, K=3, stages=(2, 2))
    X, y = torch.from_numpy(c["X"]), torch.from_numpy(c["y"])
    ok = dict(stage_off=c["stage_off"], tree_col=c["tree_col"], K=3, metric="mlogloss")
    for bad in (dict(metric="auc"), dict(stage_off=[0, 5]), dict(stage_off=[2, 1]), dict(tree_col=[0, 1, 2, 3]),
                dict(K=1), dict(metric="logloss"), dict(tree_weight=[1.0])):
        with pytest.raises(ValueError):
            te.forest_staged_eval(c["forest"], X, None, y, **dict(ok, **bad))
    with pytest.raises(ValueError):
        te.forest_staged_eval(c["forest"], X, torch.tensor([0, 30]), y, **ok)
    # the C entry point refuses an unknown metric code and a binary metric over K margins
    from transmogrifai_amd.ops import _native as N
    m = torch.zeros(30, 3, dtype=torch.float64)
    for code, K in ((7, 1), (-1, 1), (N.ABI_CONSTS["TMOG_EVAL_LOGLOSS"], 3)):
        assert N.host().tmog_forest_staged_eval_cpu(None, 5, None, 0, None, None, None, None, None, None, -1, None, 0,
                                                    None, K, code, 1.0, 16, N.ptr(m), None, None, None) != 0


# ============================================================================================== fitted models
def _data(n=2000, seed=2, kind="binary"):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 6, generator=g, dtype=torch.float64)
    X[:, 1:] = torch.round(X[:, 1:])
    if kind == "binary":
        y = ((X[:, 0] > 0.3) ^ (torch.rand(n, generator=g) < 0.15)).double()
    elif kind == "regression":
        y = 2.0 * X[:, 0] + X[:, 1] + 2.0 * torch.randn(n, generator=g, dtype=torch.float64)
    else:
        y = ((X[:, 0] > -0.4).double() + (X[:, 0] > 0.5).double())
        flip = torch.rand(n, generator=g) < 0.2
        y = torch.where(flip, torch.randint(0, 3, (n,), generator=g).double(), y)
    return X, y


def _prefix(st, k):
    """The model of the first ``k`` trees of a fitted state."""
    f = te.Forest.from_state(st["forest"])
    out = {a: b for a, b in st.items() if not a.startswith("_")}
    out.update(forest=te.Forest.concat([f.tree(t) for t in range(k)]).to_state(),
               tree_weights=np.asarray(st["tree_weights"], np.float32)[:k], num_trees=k)
    return out


def _logloss(m, y, scale=1.0):
    sm = scale * m
    return float((torch.log1p(torch.exp(-sm.abs())) + sm.clamp_min(0) - y * sm).mean())


_FITTED = [("xgb_binary", "OpXGBoostClassifier", "binary", dict(num_round=10, max_depth=3), None, 1.0),
           ("xgb_regressor", "OpXGBoostRegressor", "regression", dict(num_round=10, max_depth=3), None, 1.0),
           ("xgb_softprob", "OpXGBoostClassifier", "multi", dict(num_round=6, max_depth=3, objective="multi:softprob"),
            None, 1.0),
           ("gbt_classifier", "OpGBTClassifier", "binary", dict(max_iter=8, max_depth=3), None, 2.0),
           ("gbt_regressor", "OpGBTRegressor", "regression", dict(max_iter=8, max_depth=3), None, 2.0)]


@pytest.mark.parametrize("name,learner,kind,params,metric,scale", _FITTED, ids=[f[0] for f in _FITTED])
def test_staged_eval_of_fitted_models(name, learner, kind, params, metric, scale):
    """``staged_eval`` against one ``learner.margin`` per prefix and the metric in torch. ``margin`` accumulates in
    fp32: per row it is within ``e = (T + 2) 2^-24 sum |w v|`` of the fp64 margin (forest_predict_oracle.bound), which
    moves the mean logloss by at most ``mean(s e)`` (|d term / d m| <= s), the rmse by at most ``sqrt(mean e^2)``
    (triangle inequality) and the mean mlogloss by at most ``mean(2 max_c e_c)`` (the gradient of logsumexp(m) - m_l
    has 1-norm <= 2)."""
    from transmogrifai_amd.models.base import learner_class
    X, y = _data(2000, 5, kind)
    L = learner_class(learner)()
    st = L.fit_batch(X, y, [FitJob(dict(L.defaults, **params), None)])[0]
    K = 3 if kind == "multi" else 1
    curve = L.staged_eval(st, X, y)
    rounds = st["num_trees"] // K
    assert curve.shape == (rounds,) and curve.dtype == np.float64 and rounds >= 6
    forest, Xb = L._binned_for(st, X, None)
    tw = np.asarray(st["tree_weights"], np.float64)
    for r in range(rounds):
        k = (r + 1) * K
        m = L.margin(_prefix(st, k), X)
        e = [FO.bound(forest, Xb.numpy(), None, list(range(c, k, K)), tw)[:, 0] for c in range(K)]
        if kind == "binary":
            ref, tol = _logloss(m, y, scale), scale * e[0].mean()
        elif kind == "regression":
            ref, tol = float(((m - y) ** 2).mean().sqrt()), np.sqrt((e[0] ** 2).mean())
        else:
            ref = float(-torch.log_softmax(m, 1).gather(1, y.long()[:, None]).mean())
            tol = (2 * np.max(np.stack(e), 0)).mean()
        assert abs(curve[r] - ref) <= tol + 1e-12 * max(1.0, abs(ref)), (r, curve[r], ref, tol)
    # another metric and a row subset go through the same pass
    rows = torch.arange(0, 2000, 3)
    other = {"binary": "error", "regression": "mae", "multi": "merror"}[kind]
    sub = L.staged_eval(st, X, y, metric=other, rows=rows)
    m = L.margin(st, X, rows)
    last = {"binary": lambda: float(((m > 0) != (y[rows] > 0.5)).double().mean()),
            "regression": lambda: float((m - y[rows]).abs().mean()),
            "multi": lambda: float((m.argmax(1) != y[rows].long()).double().mean())}[kind]()
    assert abs(sub[-1] - last) <= (5e-3 if kind != "regression" else 1e-4)      # fp32 margins may flip a tied row


# ============================================================================================== held-out watch
def _replay(L, X, y, params, rows, patience, metric, K=1):
    """The rule of the learners on the oracle's curve: ``(best round, stop round, curve, unstopped state, training
    rows)``. The curve is the oracle's, on the watch rows, of the model grown for every round on the training rows."""
    tr, wr = TR.watch_split(rows, params["train_test_ratio"], params["seed"])
    free = dict(params, train_test_ratio=1.0, num_early_stopping_rounds=0)
    full = L.fit_batch(X, y, [FitJob(free, tr)])[0]
    forest, Xb = L._binned_for(full, X, None)
    T = forest.n_trees
    m = SO.staged_margins(forest, Xb.numpy(), wr.numpy(), np.arange(0, T + 1, K), np.arange(T) % K, K,
                          np.asarray(full["tree_weights"], np.float64), full["base_margin"])
    yw = y[wr].float().double().numpy()          # the learners' labels are fp32
    if metric == "logloss":
        curve = np.array([float(SO.logloss_terms(m[s, :, 0], yw, 1.0).mean()) for s in range(len(m))])
    elif metric == "mlogloss":
        curve = np.array([float(SO.mlogloss_terms(m[s], yw.astype(np.int64)).mean()) for s in range(len(m))])
    else:
        curve = SO.finish(SO.raw(m, yw, metric)[0], len(wr), metric)
    best, best_round, stop = -np.inf, 0, None
    for r, v in enumerate(-curve):
        if v > best + 1e-12:
            best, best_round = v, r
        elif r - best_round >= patience:
            stop = r
            break
    return best_round, stop, curve, free, tr


def _same_model(a, b):
    assert a["num_trees"] == b["num_trees"]
    for k in ("tree_off", "nodes", "default_left", "value"):
        np.testing.assert_array_equal(np.asarray(a["forest"][k]), np.asarray(b["forest"][k]), err_msg=k)
    np.testing.assert_array_equal(a["tree_weights"], b["tree_weights"])
    assert a["base_margin"] == b["base_margin"]


_WATCHED = {"binary": ("OpXGBoostClassifier", "binary", dict(eval_metric="logloss"), "logloss", 1),
            "regressor": ("OpXGBoostRegressor", "regression", dict(eval_metric="rmse"), "rmse", 1),
            "softprob": ("OpXGBoostClassifier", "multi", dict(eval_metric="mlogloss", objective="multi:softprob"),
                         "mlogloss", 3)}


def _watched_fit(which, n=3000, device="cpu", **over):
    from transmogrifai_amd.models.base import learner_class
    name, kind, extra, metric, K = _WATCHED[which]
    X, y = _data(n, 2, kind)
    L = learner_class(name)()
    params = dict(L.defaults, num_round=40, max_depth=4, eta=0.5, num_early_stopping_rounds=3, train_test_ratio=0.75,
                  **extra)
    params.update(over)
    rows = torch.arange(n)
    st = L.fit_batch(X.to(device), y.to(device), [FitJob(params, rows.to(device))])[0]
    return L, X, y, params, rows, st, metric, K


@pytest.mark.parametrize("which", list(_WATCHED))
def test_watch_early_stopping_replays(which):
    """The fitted model is the job fit on ``watch_split``'s training rows, without stopping, for ``best + 1`` rounds,
    ``best`` being what the stopping rule gives on the oracle's held-out curve; ``eval_history`` is that curve up to
    the round that stopped the fit."""
    L, X, y, params, rows, st, metric, K = _watched_fit(which)
    best, stop, curve, free, tr = _replay(L, X, y, params, rows, 3, metric, K)
    assert stop is not None and st["num_trees"] == (best + 1) * K < 40 * K
    _same_model(st, L.fit_batch(X, y, [FitJob(dict(free, num_round=best + 1), tr)])[0])
    assert st["best_iteration"] == best and st["eval_metric"] == metric and st["train_test_ratio"] == 0.75
    assert st["eval_history"].shape == (stop + 1,)
    np.testing.assert_allclose(st["eval_history"], curve[:stop + 1], rtol=1e-12, atol=0)
    # the stopped model's own curve on the watch rows is the history up to the kept rounds
    np.testing.assert_allclose(L.staged_eval(st, X, y, metric=metric, rows=TR.watch_split(rows, 0.75, 0)[1]),
                               st["eval_history"][:best + 1], rtol=1e-12, atol=0)


def test_watch_model_does_not_depend_on_the_chunk(monkeypatch):
    _, _, _, _, _, base, _, _ = _watched_fit("binary")
    for chunk in ("1", "5"):
        monkeypatch.setenv("TMOG_XGB_WATCH_CHUNK", chunk)
        st = _watched_fit("binary")[5]
        _same_model(st, base)
        np.testing.assert_array_equal(st["eval_history"], base["eval_history"])
        assert st["best_iteration"] == base["best_iteration"]


def test_watch_model_alone_and_in_a_batch():
    """Jobs with other rows and ratios beside it do not change a job's model: the split is a function of the global
    row id and the seed."""
    L, X, y, params, rows, alone, _, _ = _watched_fit("binary")
    jobs = [FitJob(dict(params, train_test_ratio=0.6, eval_metric="error"), torch.arange(500, 3000)),
            FitJob(params, rows),
            FitJob(dict(params, train_test_ratio=1.0, num_round=5), torch.arange(0, 2500))]
    out = L.fit_batch(X, y, jobs)
    _same_model(out[1], alone)
    np.testing.assert_array_equal(out[1]["eval_history"], alone["eval_history"])
    assert out[0]["eval_metric"] == "error" and out[0]["train_test_ratio"] == 0.6
    assert "eval_history" not in out[2] and out[2]["num_trees"] == 5


def test_watch_without_patience_records_the_whole_curve():
    L, X, y, params, rows, st, metric, K = _watched_fit("binary", num_round=8, num_early_stopping_rounds=0,
                                                         eval_metric="aucpr")
    assert st["num_trees"] == 8 and st["eval_history"].shape == (8,) and st["eval_metric"] == "aucpr"
    assert st["best_iteration"] == int(np.argmax(st["eval_history"]))


def test_stages_accept_train_test_ratio():
    for stage in (TR.OpXGBoostClassifier, TR.OpXGBoostRegressor):
        assert stage(num_round=3, train_test_ratio=0.8)._accepts_param("train_test_ratio")
        assert stage.learner_cls.defaults["train_test_ratio"] == 1.0
    assert "train_test_ratio" not in TR.GBTClassifierLearner.defaults


def test_watch_validation_and_round_trips(tmp_path):
    from transmogrifai_amd.models.base import learner_class
    L, X, y, params, rows, st, _, _ = _watched_fit("binary", num_round=6)
    new = {"eval_metric", "eval_history", "best_iteration", "train_test_ratio"}
    assert new <= set(st)
    plain = L.fit_batch(X, y, [FitJob(dict(params, train_test_ratio=1.0, num_round=3), rows)])[0]
    assert not new & set(plain)
    for name, bad in (("OpXGBoostClassifier", dict(eval_metric="rmse")), ("OpXGBoostRegressor", dict(eval_metric="aucpr")),
                      ("OpXGBoostClassifier", dict(eval_metric="logloss", objective="multi:softprob"))):
        Lb = learner_class(name)()
        with pytest.raises(ValueError, match="eval_metric"):
            Lb.fit_batch(X, y, [FitJob(dict(Lb.defaults, num_round=2, train_test_ratio=0.75, **bad), rows)])
    with pytest.raises(ValueError, match="watch"):
        # the training side of the split holds no watch rows
        L.fit_batch(X, y, [FitJob(dict(params, train_test_ratio=0.75), TR.watch_split(rows, 0.75, params["seed"])[0])])
    back = L.state_from_json(json.loads(json.dumps(L.state_to_json(st))))
    assert back["eval_metric"] == st["eval_metric"] and back["best_iteration"] == st["best_iteration"]
    assert back["train_test_ratio"] == st["train_test_ratio"]
    np.testing.assert_array_equal(np.asarray(back["eval_history"], np.float64), st["eval_history"])
    # the op-model.json round trip of the fitted stage
    from transmogrifai_amd.models.base import OpPredictorModel
    model = OpPredictorModel("OpXGBoostClassifier", st, dict(params))
    again = OpPredictorModel()
    again.load_ctor_args(json.loads(json.dumps(model.ctor_args())))
    for k in ("eval_metric", "best_iteration", "train_test_ratio"):
        assert again.state[k] == st[k]
    np.testing.assert_array_equal(np.asarray(again.state["eval_history"], np.float64), st["eval_history"])
    np.testing.assert_array_equal(L.predict(again.state, X)[2].numpy(), L.predict(st, X)[2].numpy())
