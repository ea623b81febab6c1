"""SHAP interaction values on the host: ``tree_engine.forest_shap_interactions``
(``tmog_forest_shap_interactions_cpu``) against the brute-force definition of ``tree_shap_interaction_oracle``.

Tolerance: ``1e-9 * S`` with ``S = sum_t |w_t| max_node |value_t|``, the bound of the SHAP tests: both sides are
fp64 and every cover ratio of the generated trees is >= 1/256. Totals are compared with ``forest_predict`` to its
fp32 summation bound ``3 * 2^-24 * S`` (one tree) / ``(T + 2) * 2^-24 * S``."""
import numpy as np
import pytest
import torch

import tree_shap_interaction_oracle as IO
import tree_shap_oracle as O
from test_record_insights_shap import _fit_mixed, _magnitude, _raw
from transmogrifai_amd.models import tree_engine as te


def _inter(forest, Xb, kw, dev="cpu"):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    Phi, used = te.forest_shap_interactions(forest, torch.from_numpy(np.ascontiguousarray(Xb)).to(dev),
                                            None if rows is None else torch.as_tensor(rows).to(dev), **kw)
    return Phi, used


def _shap(forest, Xb, kw):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    return te.forest_shap(forest, torch.from_numpy(np.ascontiguousarray(Xb)),
                          None if rows is None else torch.as_tensor(rows), **kw)[0]


@pytest.mark.parametrize("name", O.CASES)
def test_host_twin_matches_bruteforce(name):
    forest, Xb, kw, want = IO.case(name)
    got, used = _inter(forest, Xb, kw)
    assert tuple(got.shape) == want.shape and got.dtype == torch.float64
    assert used.dtype == np.int64 and (used == O.used_features(forest)).all()
    S = O.magnitude(forest, kw.get("tree_weight"))
    err = np.abs(got.numpy() - want).max()
    print(name, "max error / S =", err / S)
    assert err <= 1e-9 * S


@pytest.mark.parametrize("name", O.CASES)
def test_symmetric_and_rows_sum_to_shap(name):
    forest, Xb, kw, _ = IO.case(name)
    Phi, _ = _inter(forest, Xb, kw)
    S = O.magnitude(forest, kw.get("tree_weight"))
    assert torch.equal(Phi, Phi.transpose(1, 2))
    assert (Phi.sum(2) - _shap(forest, Xb, kw)).abs().max().item() <= 1e-9 * S


@pytest.mark.parametrize("name", O.CASES)
def test_total_is_the_prediction(name):
    forest, Xb, kw, _ = IO.case(name)
    Phi, _ = _inter(forest, Xb, kw)
    rows = None if kw.get("rows") is None else torch.as_tensor(kw["rows"])
    w = None if kw.get("tree_weight") is None else np.asarray(kw["tree_weight"], np.float32)
    pred = te.forest_predict(forest, torch.from_numpy(Xb), [rows], [list(range(forest.n_trees))], w)[0]
    total = Phi.sum((1, 2))
    if "tree_out" in kw:                                 # the predictor sums the trees into one column
        total = total.sum(1, keepdim=True)
    S = O.magnitude(forest, kw.get("tree_weight"))
    err = (total - pred.to(torch.float64)).abs().max().item()
    print(name, "total error / S =", err / S)
    assert err <= 3 * 2.0 ** -24 * S


def test_lone_leaf_is_all_bias():
    forest, Xb, kw, _ = O.case("lone_leaf")
    Phi, used = _inter(forest, Xb, kw)
    assert used.size == 0 and tuple(Phi.shape) == (2, 1, 1, 1)
    assert (Phi == 0.75).all()


def test_stump_has_a_main_effect_and_a_bias_only():
    forest, Xb, kw, _ = O.case("stump")
    Phi, used = _inter(forest, Xb, kw)
    assert tuple(Phi.shape) == (1, 2, 2, 1)
    assert Phi[0, 0, 0, 0] != 0 and Phi[0, 1, 1, 0] != 0
    assert Phi[0, 0, 1, 0] == 0 and Phi[0, 1, 0, 0] == 0
    assert torch.equal(Phi[:, [0, 1], [0, 1]], _shap(forest, Xb, kw))


def test_two_stumps_on_different_columns_do_not_interact():
    a = O.stump()
    b = O.stump()
    b.nodes[0, 0] = 1                                    # the second stump splits column 1
    forest = te.Forest.concat([a, b])
    Xb = np.asarray([[0, 0, 4, 0], [0, 5, 0, 0], [0, 2, 2, 0]], np.uint8)
    Phi, used = _inter(forest, Xb, dict(tree_weight=np.asarray([1.0, -0.5])))
    assert used.tolist() == [1, 2]
    assert (Phi[:, 0, 1] == 0).all() and (Phi[:, 1, 0] == 0).all()
    assert (Phi[:, 0, 0] != 0).all() and (Phi[:, 1, 1] != 0).all()


@pytest.mark.parametrize("m", [2, 5, 9, 33])
def test_equal_chain_closed_form(m):
    """Interchangeable features, a row that goes right everywhere: every off-diagonal cell is
    ``(1 - 2^-(m-1)) / (4 (m - 1))``."""
    f = O.chain_forest(m, equal=True)
    Phi, _ = _inter(f, np.ones((2, m), np.uint8), {})
    off = Phi[:, :m, :m, 0][:, ~np.eye(m, dtype=bool)]
    assert (off - (1.0 - 0.5 ** (m - 1)) / (4 * (m - 1))).abs().max().item() <= 1e-9


def test_n_out_too_small_is_an_error():
    forest, Xb, kw, _ = O.case("rf_tree_out")
    with pytest.raises(ValueError):
        te.forest_shap_interactions(forest, torch.from_numpy(Xb), n_out=2, tree_out=kw["tree_out"])


def test_column_beyond_the_matrix_is_an_error():
    forest, Xb, kw, _ = O.case("rf_k1")
    with pytest.raises(ValueError):
        te.forest_shap_interactions(forest, torch.from_numpy(np.ascontiguousarray(Xb[:, :3])))


@pytest.mark.parametrize("key", ["rf", "gbt", "xgb", "xgb3", "xgbreg"])
def test_learner_interactions_sum_to_shap_values_and_the_raw_score(key):
    scored, vec, model = _fit_mixed(key)[:3]
    X = scored[vec.name].values[:120]
    learner, state = model.learner, model.state
    Phi, used = learner.shap_interaction_values(state, X)
    phi, used2 = learner.shap_values(state, X)
    S, n_trees = _magnitude(model)
    U = len(used)
    assert (used == used2).all() and tuple(Phi.shape) == (120, U + 1, U + 1, phi.shape[2])
    assert torch.equal(Phi, Phi.transpose(1, 2))
    assert (Phi.sum(2) - phi).abs().max().item() <= 1e-9 * S
    assert (Phi[:, :U, :U][:, ~np.eye(U, dtype=bool)] != 0).any()
    assert (Phi.sum((1, 2)) - _raw(model, X)).abs().max().item() <= (n_trees + 2) * 2.0 ** -24 * S


def test_learner_without_interactions_is_not_implemented():
    from transmogrifai_amd.models.base import Learner
    with pytest.raises(NotImplementedError, match="RecordInsightsLOCO"):
        Learner().shap_interaction_values({}, torch.zeros(1, 1))
