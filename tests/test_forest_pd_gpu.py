"""``tree_engine.forest_partial_dependence`` on the device: ``tmog_hip_forest_pd`` bitwise equal to the host twin in
both modes (both sum the same int64 fixed-point integers) on the cases of tests/forest_pd_oracle.py, across many
workgroups and column chunks, and through the host-twin fallback of a grid beyond the LDS limit."""
import numpy as np
import pytest
import torch

import forest_pd_oracle as O
import forest_predict_oracle as P
from transmogrifai_amd.models import tree_engine as te

pytestmark = pytest.mark.gpu


@pytest.fixture
def no_host_twin(monkeypatch):
    """The device path must not come back through the host fallback in these tests."""
    def refuse(*a):
        raise AssertionError("forest_partial_dependence fell back to the host twin")
    monkeypatch.setattr(te.N.host(), "tmog_forest_pd_cpu", refuse)


def _pd(forest, Xb, cols, n_grid, kw, ice, dev):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    return te.forest_partial_dependence(forest, torch.from_numpy(Xb).to(dev), cols, n_grid,
                                        None if rows is None else torch.as_tensor(rows).to(dev), ice=ice, **kw)


@pytest.mark.parametrize("name", O.CASES)
def test_kernel_equals_host_twin_bitwise(name, request):
    forest, Xb, cols, NB, kw, want = O.case(name)
    host_ice, host_sum = _pd(forest, Xb, cols, NB, kw, True, "cpu"), _pd(forest, Xb, cols, NB, kw, False, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _pd(forest, Xb, cols, NB, kw, True, "cuda")
    assert got.is_cuda and got.dtype == torch.float64
    assert torch.equal(got.cpu(), host_ice)
    tw, tout = kw.get("tree_weight"), kw.get("tree_out")
    assert np.abs(got.cpu().numpy() - want).max(initial=0.0) <= O.tolerance(forest, tw, tout)
    s = _pd(forest, Xb, cols, NB, kw, False, "cuda")
    assert s.is_cuda and s.dtype == torch.float64
    assert torch.equal(s.cpu(), host_sum)
    assert np.abs(s.cpu().numpy() - want.sum(0)).max(initial=0.0) <= O.tolerance(forest, tw, tout,
                                                                                 n_sum=want.shape[0])


def test_many_workgroups_equal_host_twin(request):
    """4097 rows through a row list into the case's 67 rows: many workgroups and a last tile of one row."""
    forest, Xb, cols, NB, kw, _ = O.case("k3_missing_rows_dup")
    kw = dict(kw, rows=np.arange(4097) % Xb.shape[0])
    host = _pd(forest, Xb, cols, NB, kw, False, "cpu")
    host_ice = _pd(forest, Xb, cols, NB, kw, True, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _pd(forest, Xb, cols, NB, kw, False, "cuda")
    assert torch.equal(got.cpu(), host)
    again = _pd(forest, Xb, cols, NB, kw, False, "cuda")
    assert torch.equal(got, again)
    ice = _pd(forest, Xb, cols, NB, kw, True, "cuda")
    assert ice.shape[0] == 4097 and torch.equal(ice.cpu(), host_ice)


def test_column_chunks_equal_single_column_calls(request):
    """37 columns x C = 3 at 32 bins: 28 KB per row, so the requested columns take several chunks of the grid's
    second dimension; each column's result is bitwise what a call for it alone gives."""
    forest, Xb, cols, NB, kw, _ = O.case("q37_unsplit")
    assert len(cols) * NB * 3 * 8 * 16 > 160 * 1024
    request.getfixturevalue("no_host_twin")
    for ice in (True, False):
        together = _pd(forest, Xb, cols, NB, kw, ice, "cuda")
        for q, c in enumerate(cols):
            alone = _pd(forest, Xb, [c], NB, kw, ice, "cuda")
            assert torch.equal(alone[:, 0] if ice else alone[0], together[:, q] if ice else together[q])


def test_sum_mode_column_chunks_equal_host_twin(request):
    """The sum's shared tile is per workgroup, not per row, so it takes a wide grid to chunk it: 6 columns x 256
    bins x 10 output columns are 120 KB, beyond the 80 KB LDS share."""
    rng = np.random.default_rng(42)
    F, B = 6, 256
    f = P.random_forest(rng, 7, F, B, 1, budget=31, values=lambda n, k: P.rounded_values(rng, n, k))
    P.check_forest(f, F, B)
    Xb = P.random_bins(rng, 131, F, B)
    kw = dict(tree_out=np.asarray([0, 3, 9, 7, 1, 9, 4]), n_out=10, tree_weight=P.rounded_weights(rng, 7))
    cols = [5, 0, 3, 1, 4, 2]
    assert len(cols) * B * 10 * 8 > 80 * 1024
    host = _pd(f, Xb, cols, B, kw, False, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _pd(f, Xb, cols, B, kw, False, "cuda")
    assert torch.equal(got.cpu(), host) and np.ptp(host.numpy(), axis=1).max() > 0
    for q, c in enumerate(cols):
        assert torch.equal(_pd(f, Xb, [c], B, kw, False, "cuda")[0], got[q])


def test_wide_grid_takes_the_host_twin():
    """256 bins x 100 output columns: 204 800 bytes for one row x one column exceed the 160 KiB of LDS; the call
    returns the host twin's result on the device."""
    rng = np.random.default_rng(41)
    F, B = 6, 256
    f = P.random_forest(rng, 4, F, B, 1, budget=15)
    P.check_forest(f, F, B)
    Xb = P.random_bins(rng, 3, F, B)
    kw = dict(tree_out=np.asarray([0, 33, 99, 7]), n_out=100)
    assert B * 100 * 8 > 160 * 1024
    for ice in (True, False):
        host = _pd(f, Xb, [0, 2, 5], B, kw, ice, "cpu")
        got = _pd(f, Xb, [0, 2, 5], B, kw, ice, "cuda")
        assert got.is_cuda and got.shape == host.shape and torch.equal(got.cpu(), host)
    assert np.ptp(host.numpy(), axis=1).max() > 0
