"""Multiclass XGBoost (``objective="multi:softprob"`` / ``"multi:softmax"``): K Newton trees a round coupled by the
softmax round epilogue (models/trees.py ``_SoftmaxObjective`` under ``_newton_boost``). CPU path = the torch fp64
epilogue."""
import json
import os
import socket
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

from transmogrifai_amd.models.base import FitJob
from transmogrifai_amd.models.trees import XGBoostClassifierLearner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IRIS = os.path.join(ROOT, "tests", "golden", "reference", "helloworld", "src", "main", "resources", "IrisDataset",
                    "iris.data")
ARRAYS = ("tree_off", "nodes", "default_left", "value", "gain", "cover")


def _blobs(n=900, d=4, k=3, seed=0, noise=1.0):
    g = np.random.default_rng(seed)
    c = g.integers(0, k, n)
    centres = 3.0 * np.eye(k, d)
    X = centres[c] + noise * g.normal(size=(n, d))
    return torch.as_tensor(X), torch.as_tensor(c.astype(np.float64))


def _params(**kw):
    return dict(XGBoostClassifierLearner.defaults, **{"objective": "multi:softprob", **kw})


def _same_state(a, b):
    for k in ARRAYS:
        np.testing.assert_array_equal(np.asarray(a["forest"][k]), np.asarray(b["forest"][k]), err_msg=k)
    np.testing.assert_array_equal(np.asarray(a["tree_weights"]), np.asarray(b["tree_weights"]))
    assert a["num_trees"] == b["num_trees"] and a["n_classes"] == b["n_classes"]


def test_shape_and_contract():
    X, y = _blobs()
    L = XGBoostClassifierLearner()
    st = L.fit_batch(X, y, [FitJob(_params(num_round=10, max_depth=3), torch.arange(600))])[0]
    pred, raw, prob = L.predict(st, X)
    n = X.shape[0]
    assert prob.shape == (n, 3)
    assert float((prob.sum(1) - 1.0).abs().max()) <= 1e-12
    assert torch.equal(pred, prob.argmax(1).to(pred.dtype))
    assert raw.shape == (n, 3)
    assert st["n_classes"] == 3
    assert st["num_trees"] == 30
    assert st["objective"] == "multi:softprob"
    assert float((pred[600:] == y[600:]).double().mean()) > 0.9
    # predict_batch goes through the same margins
    rows = torch.arange(600, n)
    pb = L.predict_batch([st], X, [rows])[0]
    torch.testing.assert_close(pb[2], prob[600:], rtol=0, atol=0)
    assert L.feature_contributions(st, 4).shape == (4,)


def test_softmax_objective_trains_the_same_model():
    X, y = _blobs(seed=1)
    L = XGBoostClassifierLearner()
    rows = torch.arange(0, 900, 2)
    a = L.fit_batch(X, y, [FitJob(_params(num_round=5, max_depth=3), rows)])[0]
    b = L.fit_batch(X, y, [FitJob(_params(num_round=5, max_depth=3, objective="multi:softmax"), rows)])[0]
    _same_state(a, b)
    assert b["objective"] == "multi:softmax"
    # num_class given: the same trees as max(label) + 1
    c = L.fit_batch(X, y, [FitJob(_params(num_round=5, max_depth=3, num_class=3), rows)])[0]
    _same_state(a, c)


def test_single_leaf_closed_form():
    """X constant: no split exists, every tree is one leaf ``-eta sum(g_k) / (sum(h_k) + lambda)``, replayed in
    numpy fp64. What separates the engine from the closed form is its fixed-point (g, h) and the fp32 leaf
    values. The same construction with ``binary:logistic`` (n = 300, one class of 150/100/50 against the rest,
    5 rounds, eta 0.3, lambda 1) deviates from its own closed form by at most 1.58e-7 in probability (1.37e-7
    for the class of 100, 1.58e-7 for the class of 50, 0 for the class of 150), measured on the code before
    the multiclass objective existed; three coupled trees are allowed 4x that: 6.32e-7."""
    n, eta, lam = 300, 0.3, 1.0
    c = np.repeat([0, 1, 2], [150, 100, 50])
    X = torch.ones(n, 4, dtype=torch.float64)
    L = XGBoostClassifierLearner()
    st = L.fit_batch(X, torch.as_tensor(c.astype(np.float64)),
                     [FitJob(_params(num_round=5, eta=eta, reg_lambda=lam, max_depth=3), torch.arange(n))])[0]
    assert st["num_trees"] == 15
    assert len(np.asarray(st["forest"]["nodes"])) == 15          # one leaf per tree
    prob = L.predict(st, X)[2].numpy()
    m = np.full((n, 3), 0.5)
    onehot = np.eye(3)[c]
    for _ in range(5):
        e = np.exp(m - m.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        g, h = p - onehot, np.maximum(2.0 * p * (1.0 - p), 1e-16)
        m = m - eta * g.sum(0) / (h.sum(0) + lam)
    e = np.exp(m - m.max(1, keepdims=True))
    ref = e / e.sum(1, keepdims=True)
    dev = float(np.abs(prob - ref).max())
    print("closed-form max |prob - ref| =", dev)
    assert dev <= 4 * 1.58e-7


def _noisy(n=1500, seed=2):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 6, generator=g, dtype=torch.float64)
    X[:, 1:] = torch.round(X[:, 1:])
    y = (X[:, 0] > -0.4).long() + (X[:, 0] > 0.5).long()
    flip = torch.rand(n, generator=g) < 0.2
    y = torch.where(flip, torch.randint(0, 3, (n,), generator=g), y).double()
    return X, y


def test_early_stopping_merror_trims_whole_rounds():
    """Early stopping on the training merror (the default metric of a multiclass objective; minimised, read back
    late): the kept trees are exactly rounds 0..best_round of a replay without early stopping."""
    X, y = _noisy()
    n, K, esr = X.shape[0], 3, 3
    params = _params(num_round=60, max_depth=2, eta=0.3, num_early_stopping_rounds=esr)
    L = XGBoostClassifierLearner()
    rows = torch.arange(n)
    st = L.fit_batch(X, y, [FitJob(params, rows)])[0]
    assert st["num_trees"] % K == 0
    assert st["num_trees"] < 60 * K
    explicit = L.fit_batch(X, y, [FitJob(dict(params, eval_metric="merror", maximize_evaluation_metrics=True),
                                         rows)])[0]
    _same_state(st, explicit)
    kept = st["num_trees"] // K
    # replay: the training merror after each round (the first r + 1 rounds do not depend on later rounds)
    best, best_round, replay = float("inf"), 0, {}
    for r in range(kept + esr):
        s = L.fit_batch(X, y, [FitJob(dict(params, num_early_stopping_rounds=0, num_round=r + 1), rows)])[0]
        replay[r] = s
        v = float((L.predict(s, X)[0] != y).double().mean())
        if v < best - 1e-12:
            best, best_round = v, r
        elif r - best_round >= esr:
            break
    assert kept == best_round + 1
    _same_state(st, replay[best_round])
    # mlogloss is minimised too and keeps whole rounds
    ll = L.fit_batch(X, y, [FitJob(dict(params, eval_metric="mlogloss", num_round=8), rows)])[0]
    assert ll["num_trees"] % K == 0 and ll["num_trees"] > 0


def test_mixed_fit_batch_leaves_the_binary_job_alone():
    X, y3 = _blobs(n=600, seed=3)
    y2 = (y3 > 0).double()
    L = XGBoostClassifierLearner()
    rows = torch.arange(0, 600, 2)
    bparams = dict(XGBoostClassifierLearner.defaults, num_round=6, max_depth=3)
    ref = L.fit_batch(X, y2, [FitJob(bparams, rows)])[0]
    # one call, one y: the 0/1 label serves both (the multiclass job is told its class count)
    mixed = L.fit_batch(X, y2, [FitJob(bparams, rows), FitJob(_params(num_round=4, max_depth=3, num_class=3), rows)])
    _same_state(ref, mixed[0])
    assert mixed[0]["base_margin"] == ref["base_margin"] and "objective" not in mixed[0]
    assert mixed[1]["n_classes"] == 3 and mixed[1]["num_trees"] == 12
    # and the 0/1/2 label for the multiclass job in a call of its own
    multi = L.fit_batch(X, y3, [FitJob(_params(num_round=4, max_depth=3), rows)])[0]
    assert multi["n_classes"] == 3
    assert L.predict(multi, X)[2].shape == (600, 3)
    torch.testing.assert_close(L.predict(mixed[0], X)[2], L.predict(ref, X)[2], rtol=0, atol=0)


def test_boost_job_bytes_count_the_pseudo_jobs():
    from transmogrifai_amd.models import trees as TR
    job = FitJob({"max_depth": 4}, torch.arange(1000), None)
    assert TR._boost_job_bytes(job, 5000, 10, 32, 3) == 3 * TR._boost_job_bytes(job, 5000, 10, 32)


def test_multiclass_selector_with_xgboost(tmp_path):
    from transmogrifai_amd.dsl import transmogrify
    from transmogrifai_amd.features import types as T
    from transmogrifai_amd.features.builder import FeatureBuilder
    from transmogrifai_amd.local.scoring import batch_score_function, score_function
    from transmogrifai_amd.readers.files import CSVReader
    from transmogrifai_amd.selector.factories import MultiClassificationModelSelector
    from transmogrifai_amd.stages.insights.record_insights import RecordInsightsLOCO
    from transmogrifai_amd.tuning.splitters import DataCutter
    from transmogrifai_amd.workflow.workflow import OpWorkflow, OpWorkflowModel
    grid = MultiClassificationModelSelector.models_and_params()["OpXGBoostClassifier"]
    assert len(grid) == 6 and all(g["objective"] == "multi:softprob" for g in grid)
    assert MultiClassificationModelSelector.defaults == ["OpLogisticRegression", "OpRandomForestClassifier"]
    schema = [("sepalLength", "double"), ("sepalWidth", "double"), ("petalLength", "double"),
              ("petalWidth", "double"), ("irisClass", "string")]
    feats = [FeatureBuilder.Real(n).as_predictor() for n, _ in schema[:4]]
    labels = FeatureBuilder.Text("irisClass").as_response().indexed()
    vec = transmogrify(feats)
    two = [dict(g, num_round=15, eta=0.3) for g in grid[:2]]
    pred = MultiClassificationModelSelector.with_cross_validation(
        splitter=DataCutter(reserve_test_fraction=0.2, seed=42), num_folds=2, seed=42,
        model_types_to_use=["OpXGBoostClassifier"], models_and_parameters=[("OpXGBoostClassifier", two)]
    ).set_input(labels, vec).get_output()
    wf = OpWorkflow().set_result_features(pred, labels, vec).set_reader(CSVReader(IRIS, schema))
    model = wf.train()
    stage = model.get_origin_stage_of(pred)
    summ = stage.metadata["summary"]
    assert summ["bestModelType"] == "OpXGBoostClassifier"
    assert stage.state["n_classes"] == 3 and stage.state["objective"] == "multi:softprob"
    scored = model.score(keep_intermediate_features=True)
    batch = scored[pred.name].to_list()
    lab = scored[labels.name].to_list()
    probs = np.asarray([T.Prediction(b).probability for b in batch])
    assert probs.shape == (len(batch), 3)
    assert np.mean([b["prediction"] == l for b, l in zip(batch, lab)]) > 0.9
    assert model.model_insights(pred).features          # ModelInsights reads the forest's feature contributions
    # op-model.json round trip
    model.save(str(tmp_path / "m"))
    loaded = OpWorkflowModel.load(str(tmp_path / "m")).set_reader(CSVReader(IRIS, schema))
    again = np.asarray([T.Prediction(b).probability for b in loaded.score()[pred.name].to_list()])
    np.testing.assert_array_equal(again, probs)
    # local row scoring
    with open(IRIS) as f:
        recs = [{n: (float(v) if t == "double" else v) for (n, t), v in zip(schema, line.strip().split(","))}
                for line in f.readlines()[:5]]
    row_fn = score_function(loaded)
    for r, br, p in zip(recs, batch_score_function(loaded)(recs), probs[:5]):
        assert np.allclose(T.Prediction(row_fn(r)[pred.name]).probability, p, atol=1e-9)
        assert np.allclose(T.Prediction(br[pred.name]).probability, p, atol=1e-9)
    # LOCO over the fitted model: one score column per class
    loco = RecordInsightsLOCO(stage, top_k=2).set_input(vec)
    col = loco.transform(scored.take(torch.arange(10)))[loco.get_output().name]
    assert col.diffs.shape[0] == 10 and col.diffs.shape[2] == 3


# ------------------------------------------------------------------------------------- 2 ranks, gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sig(state):
    return {k: np.asarray(state["forest"][k]).tolist() for k in ARRAYS} | {"num_trees": int(state["num_trees"])}


def _fit_par(par):
    g = torch.Generator().manual_seed(0)
    n, d = 2000, 16
    X = torch.randn(n, d, generator=g)
    X[:, 5] = (X[:, 5] > 0.3).float()               # 0/1 indicator columns (one present bin under missing=0)
    X[:, 9] = (X[:, 9] > -0.2).float()
    s = X[:, 0] - 0.7 * X[:, 3] + 0.9 * X[:, 5] + 0.3 * torch.randn(n, generator=g)
    y = ((s > -0.5).long() + (s > 0.6).long()).float()
    rows = [torch.arange(0, 1400), torch.arange(600, 2000)]
    ctx = {"par": par} if par is not None else {}
    L = XGBoostClassifierLearner()
    jobs = [FitJob(_params(num_round=4, max_depth=4, min_child_weight=mcw, missing=0.0, max_bins=32,
                           num_early_stopping_rounds=2), r) for mcw in (1.0, 10.0) for r in rows]
    return [_sig(s) for s in L.fit_batch(X, y, jobs, context=ctx)]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from transmogrifai_amd.parallel.learner_parallel import LearnerParallel
        res = _fit_par(LearnerParallel())
        with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


def test_feature_parallel_two_ranks_give_the_one_rank_model(tmp_path):
    ref = _fit_par(None)
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    for r in range(2):
        with open(tmp_path / f"r{r}.json") as f:
            assert json.load(f) == ref, f"multiclass forest differs on rank {r}"
    assert any(len(s["nodes"]) > 3 * s["num_trees"] for s in ref)      # the trees are not trivial
