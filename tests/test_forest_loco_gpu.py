"""``tree_engine.forest_loco`` on the device: ``tmog_hip_forest_loco`` bitwise equal to the host twin (both sum
the same int64 fixed-point contributions), on the cases of tests/forest_loco_oracle.py, across many workgroups,
and through the host-twin fallback of a tile beyond the LDS limit."""
import numpy as np
import pytest
import torch

import forest_loco_oracle as O
import forest_predict_oracle as P
from transmogrifai_amd.models import tree_engine as te

pytestmark = pytest.mark.gpu


@pytest.fixture
def no_host_twin(monkeypatch):
    """The device path must not come back through the host fallback in these tests."""
    def refuse(*a):
        raise AssertionError("forest_loco fell back to the host twin")
    monkeypatch.setattr(te.N.host(), "tmog_forest_loco_cpu", refuse)


def _loco(forest, Xb, zb, kw, dev):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    return te.forest_loco(forest, torch.from_numpy(Xb).to(dev), zb,
                          None if rows is None else torch.as_tensor(rows).to(dev), **kw)[0]


@pytest.mark.parametrize("name", O.CASES)
def test_kernel_equals_host_twin_bitwise(name, request):
    forest, Xb, zb, kw, want = O.case(name)
    host = _loco(forest, Xb, zb, kw, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _loco(forest, Xb, zb, kw, "cuda")
    assert got.is_cuda and got.dtype == torch.float64
    assert torch.equal(got.cpu(), host)
    assert np.abs(got.cpu().numpy() - want).max(initial=0.0) <= O.tolerance(forest, kw.get("tree_weight"),
                                                                           kw.get("tree_out"))


def test_many_workgroups_equal_host_twin(request):
    """4097 rows at U = 37 (a row list into the case's 67 rows): tile boundaries across many workgroups, and a last
    tile of one row."""
    forest, Xb, zb, kw, _ = O.case("u37_t9_tree_out_groups")
    kw = dict(kw, rows=np.arange(4097) % Xb.shape[0])
    host = _loco(forest, Xb, zb, kw, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _loco(forest, Xb, zb, kw, "cuda")
    assert got.shape[0] == 4097 and torch.equal(got.cpu(), host)
    again = _loco(forest, Xb, zb, kw, "cuda")
    assert torch.equal(got, again)


def test_wide_output_takes_the_host_twin():
    """7000 used columns x 3 output columns: 7001 x 3 int64 slots (168 KB) for one row exceed the 160 KiB of LDS;
    the call returns the host twin's result on the device."""
    rng = np.random.default_rng(21)
    F, U = 7100, 7000
    f = P.random_forest(rng, 4, F, O.B, 1, budget=3601)
    O._spread(rng, f, U, F)
    P.check_forest(f, F, O.B)
    Xb = P.random_bins(rng, 3, F, O.B)
    zb = rng.integers(0, O.B, F).astype(np.uint8)
    kw = dict(tree_out=np.asarray([0, 1, 2, 0]), n_out=3)
    assert (U + 1) * 3 * 8 > 160 * 1024
    host = _loco(f, Xb, zb, kw, "cpu")
    got = _loco(f, Xb, zb, kw, "cuda")
    assert got.is_cuda and tuple(got.shape) == (3, U + 1, 3) and torch.equal(got.cpu(), host)
    assert host[:, :-1].any()
