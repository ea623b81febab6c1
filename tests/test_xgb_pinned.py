"""XGBoost boosting pinned bit for bit: fixed batches through every objective of the Newton round driver
(models/trees.py ``_newton_boost``) on the CPU path, compared with states recorded under ``tests/golden/xgb_pinned/``.
Host-side changes to the boosting loop must leave every tree, leaf value and tree weight unchanged.

``PYTHONPATH=. python tests/test_xgb_pinned.py`` rewrites the fixtures from the code it imports."""
import os

import numpy as np
import pytest
import torch

from transmogrifai_amd.models.base import FitJob
from transmogrifai_amd.models.trees import XGBoostClassifierLearner, XGBoostRegressorLearner

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xgb_pinned")
D = XGBoostClassifierLearner.defaults


def _data_a(dev):
    n, d = 600, 9
    g = torch.Generator().manual_seed(9)
    X = torch.randn(n, d, dtype=torch.float64, generator=g)
    X[:, 1::3] = (X[:, 1::3] > 0.7).to(torch.float64)
    s = X[:, 0] + X[:, 1] - X[:, 4] + 0.3 * torch.randn(n, dtype=torch.float64, generator=g)
    yb = (s > 0).to(torch.float64)
    y3 = ((s > 0.6).to(torch.float64) + (s > -0.6).to(torch.float64))
    return [t.to(dev) for t in (X, s, yb, y3, torch.arange(0, n, 2), torch.arange(1, n, 2), torch.arange(n))]


def _data_b(dev):
    n = 600
    g = torch.Generator().manual_seed(2)
    X = torch.randn(n, 6, dtype=torch.float64, generator=g)
    X[:, 1:] = X[:, 1:].round()
    flip = torch.rand(n, generator=g) < 0.15
    yb = ((X[:, 0] > 0.3) ^ flip).to(torch.float64)
    y3 = (X[:, 0] > 0.5).to(torch.int64) + (X[:, 0] > -0.5).to(torch.int64)
    y3 = torch.where(flip, (y3 + 1) % 3, y3).to(torch.float64)
    return [t.to(dev) for t in (X, yb, y3, torch.arange(n))]


def _job(rows, defaults=D, **kw):
    return FitJob(dict(defaults, **{"missing": 0.0, **kw}), rows)


def _binary_a(dev="cpu"):
    X, _, yb, _, ev, od, al = _data_a(dev)
    sq_default_missing = FitJob(dict(D, objective="reg:squarederror", num_round=6, max_depth=3), od)
    return XGBoostClassifierLearner().fit_batch(X, yb, [
        _job(ev, num_round=8, max_depth=3),
        _job(od, num_round=5, max_depth=4, subsample=0.7, seed=3),
        _job(al, num_round=40, max_depth=2, num_early_stopping_rounds=2),
        _job(ev, objective="reg:squarederror", num_round=6, max_depth=3, num_early_stopping_rounds=3),
        sq_default_missing])                # a second bin key


def _multi_a(dev="cpu"):
    X, _, _, y3, ev, od, al = _data_a(dev)
    return XGBoostClassifierLearner().fit_batch(X, y3, [
        _job(ev, objective="multi:softprob", num_round=5, max_depth=3),
        _job(al, objective="multi:softmax", num_round=30, max_depth=2, num_early_stopping_rounds=2,
             eval_metric="mlogloss"),
        _job(od, objective="multi:softprob", num_round=4, max_depth=3, subsample=0.6, seed=5),
        _job(ev, num_round=7, max_depth=3)])


def _regressor_a(dev="cpu"):
    X, s, _, _, ev, _, al = _data_a(dev)
    RD = XGBoostRegressorLearner.defaults
    return XGBoostRegressorLearner().fit_batch(X, s, [
        _job(ev, RD, num_round=6, max_depth=3),
        _job(al, RD, num_round=3, max_depth=4, subsample=0.8, num_early_stopping_rounds=2)])


_STOP = dict(num_round=60, max_depth=2, num_early_stopping_rounds=2)


def _stop_binary_b(dev="cpu"):
    X, yb, _, al = _data_b(dev)
    return XGBoostClassifierLearner().fit_batch(X, yb, [_job(al, **_STOP),
                                                        _job(al, objective="reg:squarederror", **_STOP)])


def _stop_merror_b(dev="cpu"):
    X, _, y3, al = _data_b(dev)
    return XGBoostClassifierLearner().fit_batch(X, y3, [
        _job(al, objective="multi:softprob", eval_metric="merror", **_STOP)])


def _stop_mlogloss_b(dev="cpu"):
    X, _, y3, al = _data_b(dev)
    return XGBoostClassifierLearner().fit_batch(X, y3, [
        _job(al, objective="multi:softprob", eval_metric="mlogloss", **dict(_STOP, num_round=6))])


BATCHES = {"binary_a": _binary_a, "multi_a": _multi_a, "regressor_a": _regressor_a,
           "stop_binary_b": _stop_binary_b, "stop_merror_b": _stop_merror_b, "stop_mlogloss_b": _stop_mlogloss_b}


def _flat(states):
    """The pinned part of a batch's states as one dict of arrays (the ``.npz`` layout)."""
    out = {}
    for i, st in enumerate(states):
        out[f"{i}.nodes"] = np.asarray(st["forest"]["nodes"])
        out[f"{i}.value"] = np.asarray(st["forest"]["value"])
        out[f"{i}.tree_weights"] = np.asarray(st["tree_weights"])
        out[f"{i}.scalars"] = np.asarray([st["num_trees"], st["n_classes"]], np.int64)
        out[f"{i}.base_margin"] = np.asarray(st["base_margin"], np.float64)
        out[f"{i}.keys"] = np.asarray(sorted(k for k in st if not k.startswith("_")))
        out[f"{i}.objective"] = np.asarray(st.get("objective", ""))
    return out


@pytest.fixture(scope="module")
def fitted():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = BATCHES[name]()
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_states_equal_the_recorded_ones(name, fitted):
    got = _flat(fitted(name))
    with np.load(os.path.join(GOLDEN, name + ".npz")) as want:
        assert sorted(want.files) == sorted(got)
        for k in want.files:
            assert want[k].dtype == got[k].dtype and np.array_equal(want[k], got[k]), f"{name}: {k}"


def test_early_stopping_cases_trim(fitted):
    """The stopping cases must really stop, or they would not exercise the trim to the best round."""
    a, b = fitted("stop_binary_b")
    (c,) = fitted("stop_merror_b")
    assert a["num_trees"] < 60 and b["num_trees"] < 60 and c["num_trees"] < 60
    assert c["num_trees"] % 3 == 0                      # whole rounds
    assert "objective" not in a and b["objective"] == "reg:squarederror"


def test_regressor_does_not_stop_early(fitted):
    assert [st["num_trees"] for st in fitted("regressor_a")] == [6, 3]


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for _name, _fn in BATCHES.items():
        _states = _fn()
        np.savez_compressed(os.path.join(GOLDEN, _name + ".npz"), **_flat(_states))
        print(_name, [st["num_trees"] for st in _states])
