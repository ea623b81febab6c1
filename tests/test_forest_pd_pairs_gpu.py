"""``tree_engine.forest_partial_dependence_pairs`` on the device: ``tmog_hip_forest_pd_pairs`` bitwise equal to the
host twin in both modes (both sum the same int64 fixed-point integers) on the cases of
tests/forest_pd_pairs_oracle.py, across many workgroups, pair chunks and chunks of the first grid axis, and through
the host-twin fallback of a grid line beyond the LDS limit."""
import numpy as np
import pytest
import torch

import forest_pd_pairs_oracle as O2
import forest_predict_oracle as P
from transmogrifai_amd.models import tree_engine as te

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024          # hip/row_tile.hpp kTileLdsLimit
LDS_SHARE = 80 * 1024           # kTileLdsShare


@pytest.fixture
def no_host_twin(monkeypatch):
    """The device path must not come back through the host fallback in these tests."""
    def refuse(*a):
        raise AssertionError("forest_partial_dependence_pairs fell back to the host twin")
    monkeypatch.setattr(te.N.host(), "tmog_forest_pd_pairs_cpu", refuse)


def _pd2(forest, Xb, pairs, n_grid, kw, ice, dev):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    return te.forest_partial_dependence_pairs(forest, torch.from_numpy(Xb).to(dev), np.asarray(pairs), n_grid,
                                              None if rows is None else torch.as_tensor(rows).to(dev), ice=ice, **kw)


@pytest.mark.parametrize("name", O2.CASES)
def test_kernel_equals_host_twin_bitwise(name, request):
    forest, Xb, pairs, NB, kw, want = O2.case(name)
    host_ice, host_sum = _pd2(forest, Xb, pairs, NB, kw, True, "cpu"), _pd2(forest, Xb, pairs, NB, kw, False, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _pd2(forest, Xb, pairs, NB, kw, True, "cuda")
    assert got.is_cuda and got.dtype == torch.float64
    assert torch.equal(got.cpu(), host_ice)
    tw, tout = kw.get("tree_weight"), kw.get("tree_out")
    assert np.abs(got.cpu().numpy() - want).max(initial=0.0) <= O2.tolerance(forest, tw, tout)
    s = _pd2(forest, Xb, pairs, NB, kw, False, "cuda")
    assert s.is_cuda and s.dtype == torch.float64
    assert torch.equal(s.cpu(), host_sum)
    assert np.abs(s.cpu().numpy() - want.sum(0)).max(initial=0.0) <= O2.tolerance(forest, tw, tout,
                                                                                  n_sum=want.shape[0])


def test_many_workgroups_equal_host_twin(request):
    """4097 rows through a row list into the case's 67 rows: many workgroups and a last tile of one row."""
    forest, Xb, pairs, NB, kw, _ = O2.case("k3_missing_rows_dup")
    pairs = pairs[:2]
    kw = dict(kw, rows=np.arange(4097) % Xb.shape[0])
    host = _pd2(forest, Xb, pairs, NB, kw, False, "cpu")
    host_ice = _pd2(forest, Xb, pairs, NB, kw, True, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _pd2(forest, Xb, pairs, NB, kw, False, "cuda")
    assert torch.equal(got.cpu(), host)
    again = _pd2(forest, Xb, pairs, NB, kw, False, "cuda")
    assert torch.equal(got, again)
    ice = _pd2(forest, Xb, pairs, NB, kw, True, "cuda")
    assert ice.shape[0] == 4097 and torch.equal(ice.cpu(), host_ice)
    assert torch.equal(ice, _pd2(forest, Xb, pairs, NB, kw, True, "cuda"))


def test_pair_chunks_equal_single_pair_calls(request):
    """7 pairs at K = 3 and 32 bins: 24 KB per surface, so the sum's shared tile (172 KB for all pairs) is chunked
    over the pairs, the per-record tile over pairs and lines; each pair's surface is bitwise what a call for it
    alone gives."""
    forest, Xb, pairs, NB, kw, _ = O2.case("k3_missing_rows_dup")
    pairs = pairs + [(pairs[0][1], pairs[0][0])]
    assert len(pairs) == 7 and len(pairs) * NB * NB * 3 * 8 > LDS_LIMIT
    request.getfixturevalue("no_host_twin")
    for ice in (True, False):
        together = _pd2(forest, Xb, pairs, NB, kw, ice, "cuda")
        for p, pair in enumerate(pairs):
            alone = _pd2(forest, Xb, [pair], NB, kw, ice, "cuda")
            assert torch.equal(alone[:, 0] if ice else alone[0], together[:, p] if ice else together[p])


def test_sum_mode_line_chunks_equal_host_twin(request):
    """256 bins x 10 output columns: one surface is 5.2 MB, so the sum's tile is chunked over the first grid axis
    (a few 20 KB lines per chunk). Bitwise the host twin, and spot-checked against the cell-list oracle."""
    rng = np.random.default_rng(43)
    F, B = 6, 256
    f = P.random_forest(rng, 7, F, B, 1, budget=31, values=lambda n, k: P.rounded_values(rng, n, k))
    P.check_forest(f, F, B)
    Xb = P.random_bins(rng, 131, F, B)
    kw = dict(tree_out=np.asarray([0, 3, 9, 7, 1, 9, 4]), n_out=10, tree_weight=P.rounded_weights(rng, 7))
    pairs = [(5, 0), (1, 3)]
    assert B * B * 10 * 8 > LDS_LIMIT
    host = _pd2(f, Xb, pairs, B, kw, False, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _pd2(f, Xb, pairs, B, kw, False, "cuda")
    assert torch.equal(got.cpu(), host)
    at = [(int(i), int(j)) for i, j in rng.integers(0, B, (64, 2))] + [(0, 0), (0, B - 1), (B - 1, 0), (B - 1, B - 1)]
    at += [(B - 1, j) for j in range(B)] + [(i, B - 1) for i in range(B)]
    tol = O2.tolerance(f, kw["tree_weight"], kw["tree_out"], n_sum=Xb.shape[0])
    moved = 0.0
    for p, pair in enumerate(pairs):
        want = O2.cells(f, Xb, pair, at, **kw).sum(0)                                  # [cells, C]
        have = got.cpu().numpy()[p][tuple(np.asarray(at).T)]
        assert np.abs(have - want).max() <= tol
        moved = max(moved, np.ptp(want, axis=0).max())
    assert moved > 0


def test_per_record_line_chunks_equal_host_twin(request):
    """64 bins and a missing bin, 3 output columns: one record's surface is 101 KB, beyond the 80 KB LDS share, so
    the per-record tile is chunked over the first grid axis; the missing line sits in the last chunk."""
    rng = np.random.default_rng(44)
    F, B = 6, 65
    f = P.random_forest(rng, 9, F, B, 1, budget=31, missing_bin=B - 1,
                        values=lambda n, k: P.rounded_values(rng, n, k))
    P.check_forest(f, F, B)
    Xb = P.random_bins(rng, 37, F, B, B - 1)
    kw = dict(tree_out=np.arange(9) % 3, n_out=3, tree_weight=P.rounded_weights(rng, 9))
    pairs = [(0, 1), (4, 2), (1, 0)]
    assert 65 * 65 * 3 * 8 > LDS_SHARE
    host = _pd2(f, Xb, pairs, B, kw, True, "cpu")
    host_sum = _pd2(f, Xb, pairs, B, kw, False, "cpu")
    request.getfixturevalue("no_host_twin")
    got = _pd2(f, Xb, pairs, B, kw, True, "cuda")
    assert torch.equal(got.cpu(), host)
    assert torch.equal(_pd2(f, Xb, pairs, B, kw, False, "cuda").cpu(), host_sum)
    h = host.numpy()
    assert np.ptp(h[:, 0, :B - 1, 3], axis=1).max() > 0 and (h[:, :, B - 1] != h[:, :, B - 2]).any()
    at = [(0, 0), (B - 1, B - 1), (B - 1, 7), (7, B - 1), (31, 32), (B - 2, B - 2)]
    want = O2.cells(f, Xb, pairs[0], at, **kw)
    assert np.abs(h[:, 0][(slice(None),) + tuple(np.asarray(at).T)] - want).max() <= O2.tolerance(
        f, kw["tree_weight"], kw["tree_out"])


def test_wide_grid_line_takes_the_host_twin():
    """256 bins x 100 output columns: 204 800 bytes for one row x one grid line exceed the 160 KiB of LDS; the call
    returns the host twin's result on the device."""
    rng = np.random.default_rng(45)
    F, B = 6, 256
    f = P.random_forest(rng, 4, F, B, 1, budget=15)
    P.check_forest(f, F, B)
    Xb = P.random_bins(rng, 2, F, B)
    kw = dict(tree_out=np.asarray([0, 33, 99, 7]), n_out=100)
    assert B * 100 * 8 > LDS_LIMIT
    host = _pd2(f, Xb, [(0, 2)], B, kw, False, "cpu")
    got = _pd2(f, Xb, [(0, 2)], B, kw, False, "cuda")
    assert got.is_cuda and got.shape == host.shape and torch.equal(got.cpu(), host)
    assert np.ptp(host.numpy(), axis=(1, 2)).max() > 0
