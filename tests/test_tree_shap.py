"""Exact TreeSHAP on the host: ``tree_engine.forest_paths`` / ``forest_shap`` (``tmog_forest_shap_cpu``)
against the brute-force definition of ``tree_shap_oracle``.

Tolerance: ``1e-9 * S`` with ``S = sum_t |w_t| max_node |value_t|``; both sides are fp64 and every cover
ratio of the generated trees is >= 1/256, so the unwind divisions cannot amplify rounding past it."""
import numpy as np
import pytest
import torch

import tree_shap_oracle as O
from transmogrifai_amd.models import tree_engine as te


def _shap(forest, Xb, kw, dev="cpu"):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    phi, used = te.forest_shap(forest, torch.from_numpy(Xb).to(dev),
                               None if rows is None else torch.as_tensor(rows).to(dev), **kw)
    return phi.cpu().numpy(), used


@pytest.mark.parametrize("name", O.CASES)
def test_host_twin_matches_bruteforce(name):
    forest, Xb, kw, want = O.case(name)
    got, used = _shap(forest, Xb, kw)
    assert got.shape == want.shape and got.dtype == np.float64
    assert used.dtype == np.int64 and (used == O.used_features(forest)).all()
    S = O.magnitude(forest, kw.get("tree_weight"))
    err = np.abs(got - want).max()
    print(name, "max error / S =", err / S)
    assert err <= 1e-9 * S


def test_cases_have_the_properties_they_are_named_for():
    f = O.case("rf_k1")[0]
    fp = te.forest_paths(f)
    assert O.used_features(f).size <= 8 and f.n_trees == 7
    assert fp.p_out.size == int((f.nodes[:, 2] < 0).sum())              # one path per leaf
    assert 1 < np.diff(fp.p_off).max() <= 6
    lo, hi = fp.e_rng & 0xFFF, (fp.e_rng >> 12) & 0xFFF
    assert (lo > hi).any(), "no contradictory repeat (unsatisfiable merged interval)"
    assert ((lo > 0) & (hi < 4095) & (lo <= hi)).any(), "no element merged from both directions"
    inner = f.nodes[:, 2] >= 0
    ratios = f.cover[f.nodes[inner, 2:]] / f.cover[inner][:, None]
    assert ratios.min() >= 1.0 / 256 and (fp.e_z < ratios.min()).any()     # merged elements multiply ratios
    assert (te.forest_paths(O.case("zero_cover")[0]).e_z == 0).any()


def test_lone_leaf_is_all_bias():
    forest, Xb, kw, _ = O.case("lone_leaf")
    got, used = _shap(forest, Xb, kw)
    assert used.size == 0 and got.shape == (2, 1, 1)
    assert (got[:, 0, 0] == 0.75).all()


def test_path_order_and_length_bins():
    forest = te.Forest.concat([O.chain_forest(m, seed=m) for m in (17, 3, 33, 16, 65)])
    fp = te.forest_paths(forest)
    m = np.diff(fp.p_off)
    b = np.searchsorted([16, 32, 64], m)
    assert (np.diff(b) >= 0).all()
    assert fp.bin_off.tolist() == [0, int((m <= 16).sum()), int((m <= 32).sum()), int((m <= 64).sum())]
    assert fp.bin_off[3] == m.size - 2 and m.max() == 65        # the 65-chain's two deepest leaves


def test_chain33_efficiency_and_symmetry():
    """33 distinct features: beyond the oracle. Efficiency: bias + sum phi is the prediction. Symmetry: with
    equal covers and a row that satisfies every element, all phi_i are equal."""
    f = O.chain_forest(33, seed=3)
    X = np.random.default_rng(3).integers(0, 2, size=(6, 33)).astype(np.uint8)
    got, _ = _shap(f, X, {})
    pred = te.forest_predict(f, torch.from_numpy(X), [None], [[0]])[0].numpy().astype(np.float64)
    S = O.magnitude(f)
    assert np.abs(got.sum(1) - pred).max() <= 1e-9 * S + 3 * 2.0 ** -24 * S
    fe = O.chain_forest(33, equal=True)
    Xe = np.ones((2, 33), np.uint8)
    Xe[1, 20] = 0                     # leaves the chain at node 20: prediction 0
    ge, _ = _shap(fe, Xe, {})
    want = (1.0 - 0.5 ** 33) / 33
    assert np.abs(ge[0, :33, 0] - want).max() <= 1e-9
    assert abs(ge[0, 33, 0] - 0.5 ** 33) <= 1e-9
    assert abs(ge[1].sum()) <= 1e-9


def _grown(mode):
    """Forests grown by the engine on the host: RF-style class-count trees with bootstrap weights, Newton
    (XGBoost-style) trees with a missing bin."""
    g = torch.Generator().manual_seed(0)
    N, F, B = 1500, 10, 32
    missing = mode == te.MODE_GH
    X = torch.randint(0, B - (1 if missing else 0), (N, F), dtype=torch.uint8, generator=g)
    if missing:
        X[torch.rand(N, F, generator=g) < 0.2] = B - 1
    y = ((X[:, 0].float() + 0.5 * X[:, 3].float() + 3 * torch.randn(N, generator=g)) > 20).float()
    T = 4
    t1 = torch.round(torch.randn(T, N, generator=g) * 8) / 8
    t2 = torch.full((T, N), 0.25)
    jobs = []
    for m in range(T):
        rows = torch.arange(N)[torch.arange(N) % (m + 2) != 0]
        w = torch.randint(0, 3, (rows.numel(),), generator=g) if mode == te.MODE_CLS else None
        jobs.append(te.TreeJob(m, te.TreeParams(max_depth=6, min_instances=2, reg_lambda=1.0, min_child_weight=0.5),
                               rows, w))
    kind = te.KIND_GINI if mode == te.MODE_CLS else te.KIND_NEWTON
    f = te.grow_forest(X, np.full(F, B - 1 if missing else B), jobs, mode=mode, kind=kind, y=y, t1=t1, t2=t2, B=B,
                       missing_bin=(B - 1) if missing else -1, rng_seed=3)
    return f, X


@pytest.mark.parametrize("mode", [te.MODE_CLS, te.MODE_GH])
def test_efficiency_against_forest_predict(mode):
    """bias + sum phi equals ``forest_predict`` to the predictor's fp32 summation bound (T + 2) 2^-24 S."""
    f, X = _grown(mode)
    T = f.n_trees
    w = np.linspace(0.5, 1.5, T).astype(np.float32)
    rows = torch.arange(0, X.shape[0], 7)
    phi, used = te.forest_shap(f, X, rows, tree_weight=w)
    pred = te.forest_predict(f, X, [rows], [list(range(T))], w)[0].to(torch.float64)
    S = O.magnitude(f, w)
    err = (phi.sum(1) - pred).abs().max().item()
    print("efficiency error / S =", err / S, "bound", (T + 2) * 2.0 ** -24)
    assert phi.shape == (rows.numel(), used.size + 1, f.K)
    assert err <= (T + 2) * 2.0 ** -24 * S


def test_n_out_too_small_is_an_error():
    forest, Xb, kw, _ = O.case("rf_tree_out")
    with pytest.raises(ValueError):
        te.forest_shap(forest, torch.from_numpy(Xb), n_out=2, tree_out=kw["tree_out"])
