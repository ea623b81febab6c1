"""Exact TreeSHAP on the device: ``tmog_hip_forest_shap`` against the brute-force oracle, the host twin, and
itself (bitwise reproducible).

Tolerance: ``1e-9 * S`` as on the host; the kernel's fixed-point accumulation adds at most
``paths * 2^-62 * S`` to a slot, far below it."""
import numpy as np
import pytest
import torch

import tree_shap_oracle as O
from transmogrifai_amd.models import tree_engine as te

pytestmark = pytest.mark.gpu


@pytest.fixture
def no_host_twin(monkeypatch):
    """The device path must not come back through the host fallback in these tests."""
    def refuse(*a):
        raise AssertionError("forest_shap fell back to the host twin")
    monkeypatch.setattr(te.N.host(), "tmog_forest_shap_cpu", refuse)


def _shap(forest, Xb, kw, dev="cuda"):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    phi, used = te.forest_shap(forest, torch.from_numpy(np.ascontiguousarray(Xb)).to(dev),
                               None if rows is None else torch.as_tensor(rows).to(dev), **kw)
    return phi, used


@pytest.mark.parametrize("name", O.CASES)
def test_kernel_matches_bruteforce(name, no_host_twin):
    forest, Xb, kw, want = O.case(name)
    got, _ = _shap(forest, Xb, kw)
    assert got.is_cuda and got.dtype == torch.float64
    S = O.magnitude(forest, kw.get("tree_weight"))
    err = np.abs(got.cpu().numpy() - want).max()
    print(name, "max error / S =", err / S)
    assert err <= 1e-9 * S


@pytest.mark.parametrize("name", ["rf_k1", "rf_k3", "rf_tree_out"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_kernel_row_counts_cross_tile_and_wave_edges(name, n, no_host_twin):
    """n rows (the case's rows repeated) with and without a row list: tiles of 64 rows, groups of 4 rows a wave."""
    forest, Xb, kw, want = O.case(name)
    base = kw["rows"]
    rows = base[np.arange(n) % base.size]
    S = O.magnitude(forest, kw["tree_weight"])
    got, _ = _shap(forest, Xb, dict(kw, rows=rows))
    assert np.abs(got.cpu().numpy() - want[np.arange(n) % base.size]).max() <= 1e-9 * S
    kw2 = {k: v for k, v in kw.items() if k != "rows"}
    got2, _ = _shap(forest, Xb[rows], kw2)                          # no row list
    assert torch.equal(got, got2)


def test_kernel_tile_of_one_row(no_host_twin):
    """17 used features x 700 output columns: 18 x 700 int64 slots (98 KB) fit the LDS once, not twice."""
    forest, Xb, kw, want = O.case("chain17")
    got, _ = _shap(forest, Xb, dict(tree_out=np.asarray([5]), n_out=700))
    got = got.cpu().numpy()
    S = O.magnitude(forest)
    assert got.shape == (4, 18, 700)
    assert np.abs(got[:, :, 5] - want[:, :, 0]).max() <= 1e-9 * S
    got[:, :, 5] = 0
    assert not got.any()


def test_kernel_chain33_matches_host_twin(request):
    f = O.chain_forest(33, seed=3)
    X = np.random.default_rng(3).integers(0, 2, size=(70, 33)).astype(np.uint8)
    want, _ = _shap(f, X, {}, dev="cpu")
    request.getfixturevalue("no_host_twin")
    got, _ = _shap(f, X, {})
    assert np.abs(got.cpu().numpy() - want.numpy()).max() <= 1e-9 * O.magnitude(f)
    fe = O.chain_forest(33, equal=True)
    ge, _ = _shap(fe, np.ones((3, 33), np.uint8), {})
    assert (ge[:, :33, 0] - (1.0 - 0.5 ** 33) / 33).abs().max().item() <= 1e-9


def test_kernel_is_bitwise_reproducible(no_host_twin):
    forest, Xb, kw, _ = O.case("rf_k3")
    rows = np.arange(257) % Xb.shape[0]
    a, _ = _shap(forest, Xb, dict(kw, rows=rows))
    b, _ = _shap(forest, Xb, dict(kw, rows=rows))
    assert torch.equal(a, b)


@pytest.mark.parametrize("what", ["path longer than 64", "tile beyond the LDS limit"])
def test_fallback_to_host_twin(what):
    """A path of 65 elements (-2) and an [18 x 1200] int64 tile (169 KB, -3) come back through the host twin
    with the host twin's values."""
    if what == "path longer than 64":
        f = O.chain_forest(65, seed=5)
        X = np.random.default_rng(5).integers(0, 2, size=(9, 65)).astype(np.uint8)
        kw = {}
    else:
        f, X, _, _ = O.case("chain17")
        kw = dict(tree_out=np.asarray([1199]), n_out=1200)
    got, _ = _shap(f, X, kw)
    want, _ = _shap(f, X, kw, dev="cpu")
    assert got.is_cuda and torch.equal(got.cpu(), want)
    pred = te.forest_predict(f, torch.from_numpy(X), [None], [[0]])[0][:, 0].to(torch.float64)
    assert (want.sum((1, 2)) - pred).abs().max().item() <= 3 * 2.0 ** -24 * O.magnitude(f)
