"""SHAP interaction values on the device: ``tmog_hip_forest_shap_interactions`` against the brute-force oracle,
the host twin, and itself (bitwise reproducible).

Tolerance: ``1e-9 * S`` as on the host; the kernel's fixed-point accumulation adds at most
``paths * m * 2^-62 * S`` to a cell (one rounding per conditioning position of a path), far below it."""
import numpy as np
import pytest
import torch

import tree_shap_interaction_oracle as IO
import tree_shap_oracle as O
from transmogrifai_amd.models import tree_engine as te

pytestmark = pytest.mark.gpu


@pytest.fixture
def no_host_twin(monkeypatch):
    """The device path must not come back through the host fallback in these tests."""
    def refuse(*a):
        raise AssertionError("fell back to the host twin")
    monkeypatch.setattr(te.N.host(), "tmog_forest_shap_interactions_cpu", refuse)
    monkeypatch.setattr(te.N.host(), "tmog_forest_shap_cpu", refuse)


def _inter(forest, Xb, kw, dev="cuda"):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    Phi, used = te.forest_shap_interactions(forest, torch.from_numpy(np.ascontiguousarray(Xb)).to(dev),
                                            None if rows is None else torch.as_tensor(rows).to(dev), **kw)
    return Phi, used


@pytest.mark.parametrize("name", O.CASES)
def test_kernel_matches_bruteforce(name, no_host_twin):
    """chain15 and chain16 run W = 16, chain17 runs W = 32."""
    forest, Xb, kw, want = IO.case(name)
    got, _ = _inter(forest, Xb, kw)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape
    S = O.magnitude(forest, kw.get("tree_weight"))
    err = np.abs(got.cpu().numpy() - want).max()
    print(name, "max error / S =", err / S)
    assert err <= 1e-9 * S
    assert torch.equal(got, got.transpose(1, 2))


@pytest.mark.parametrize("name", ["rf_k1", "rf_k3", "rf_tree_out"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 257])
def test_kernel_row_counts_cross_tile_and_wave_edges(name, n, no_host_twin):
    """n rows (the case's rows repeated) with and without a row list: the edges of any power-of-two row tile
    up to 64 and a partial last tile."""
    forest, Xb, kw, want = IO.case(name)
    base = kw["rows"]
    rows = base[np.arange(n) % base.size]
    S = O.magnitude(forest, kw["tree_weight"])
    got, _ = _inter(forest, Xb, dict(kw, rows=rows))
    assert np.abs(got.cpu().numpy() - want[np.arange(n) % base.size]).max() <= 1e-9 * S
    kw2 = {k: v for k, v in kw.items() if k != "rows"}
    got2, _ = _inter(forest, Xb[rows], kw2)                         # no row list
    assert torch.equal(got, got2)


def test_kernel_feature_chunks_of_one(no_host_twin):
    """17 used features x 700 output columns: one conditioning feature's [17 x 700] int64 tile is 95 KB, so a
    workgroup holds one row and one feature and gridDim.y runs over 17 chunks."""
    forest, Xb, kw, want = IO.case("chain17")
    got, _ = _inter(forest, Xb, dict(tree_out=np.asarray([5]), n_out=700))
    got = got.cpu().numpy()
    S = O.magnitude(forest)
    assert got.shape == (4, 18, 18, 700)
    assert np.abs(got[..., 5] - want[..., 0]).max() <= 1e-9 * S
    got[..., 5] = 0
    assert not got.any()


def test_kernel_chain33_matches_host_twin(request):
    """W = 64 with 70 rows (row tiles with a partial last one), and the closed form on the equal chain."""
    f = O.chain_forest(33, seed=3)
    X = np.random.default_rng(3).integers(0, 2, size=(70, 33)).astype(np.uint8)
    want, _ = _inter(f, X, {}, dev="cpu")
    request.getfixturevalue("no_host_twin")
    got, _ = _inter(f, X, {})
    assert np.abs(got.cpu().numpy() - want.numpy()).max() <= 1e-9 * O.magnitude(f)
    fe = O.chain_forest(33, equal=True)
    ge, _ = _inter(fe, np.ones((3, 33), np.uint8), {})
    off = ge[:, :33, :33, 0].cpu()[:, ~np.eye(33, dtype=bool)]
    assert (off - (1.0 - 0.5 ** 32) / (4 * 32)).abs().max().item() <= 1e-9


def test_kernel_chain64_matches_host_twin(request):
    """The longest path the kernel takes. 64 features x 64 cells a row do not fit one tile, so the conditioning
    features are split into several chunks (the last one partial) and most pairs sit in two different chunks."""
    f = O.chain_forest(64, seed=4)
    X = np.random.default_rng(4).integers(0, 2, size=(5, 64)).astype(np.uint8)
    want, _ = _inter(f, X, {}, dev="cpu")
    request.getfixturevalue("no_host_twin")
    got, _ = _inter(f, X, {})
    assert np.abs(got.cpu().numpy() - want.numpy()).max() <= 1e-9 * O.magnitude(f)


def test_kernel_is_bitwise_reproducible_and_symmetric(no_host_twin):
    forest, Xb, kw, _ = O.case("rf_k3")
    rows = np.arange(257) % Xb.shape[0]
    a, _ = _inter(forest, Xb, dict(kw, rows=rows))
    b, _ = _inter(forest, Xb, dict(kw, rows=rows))
    assert torch.equal(a, b)
    assert torch.equal(a, a.transpose(1, 2))


@pytest.mark.parametrize("what", ["path longer than 64", "tile beyond the LDS limit"])
def test_fallback_to_host_twin(what):
    """A path of 65 elements (-2) and a [17 x 1300] int64 tile of one conditioning feature (177 KB, -3) come back
    on the device with the host twin's values."""
    hip = te.N.hip()
    seen = []
    real = hip.tmog_hip_forest_shap_interactions

    def spy(*a):
        seen.append(real(*a))
        return seen[-1]

    if what == "path longer than 64":
        f = O.chain_forest(65, seed=5)
        X = np.random.default_rng(5).integers(0, 2, size=(9, 65)).astype(np.uint8)
        kw, code = {}, -2
    else:
        f, X, _, _ = O.case("chain17")
        kw, code = dict(tree_out=np.asarray([1299]), n_out=1300), -3
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, "tmog_hip_forest_shap_interactions", spy)
        got, _ = _inter(f, X, kw)
    assert seen == [code]
    want, _ = _inter(f, X, kw, dev="cpu")
    assert got.is_cuda and torch.equal(got.cpu(), want)


def test_learner_interactions_match_the_host():
    """One small XGBoost model: the device's interaction values are within 1e-9 S of the host's."""
    from test_record_insights_shap import _fit_mixed, _magnitude
    scored, vec, model = _fit_mixed("xgb")[:3]
    X = scored[vec.name].values[:200]
    S, _ = _magnitude(model)
    host, used = model.learner.shap_interaction_values(model.state, X)
    with pytest.MonkeyPatch.context() as mp:
        def refuse(*a):
            raise AssertionError("fell back to the host twin")
        mp.setattr(te.N.host(), "tmog_forest_shap_interactions_cpu", refuse)
        dev, used_d = model.learner.shap_interaction_values(model.state, X.cuda())
    assert dev.is_cuda and (used == used_d).all() and dev.shape == host.shape
    assert (dev.cpu() - host).abs().max().item() <= 1e-9 * S
    assert torch.equal(dev, dev.transpose(1, 2))
