"""``tree_engine.forest_partial_dependence_pairs`` on the host: the twin ``tmog_forest_pd_pairs_cpu`` against the
brute-force oracle of tests/forest_pd_pairs_oracle.py in both modes, the transposed pair, the tie to the 1-D curves
of ``forest_partial_dependence`` bit for bit, and its argument errors."""
import numpy as np
import pytest
import torch

import forest_pd_pairs_oracle as O2
from transmogrifai_amd.models import tree_engine as te


def _pd2(forest, Xb, pairs, n_grid, kw, ice, dev="cpu"):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    return te.forest_partial_dependence_pairs(forest, torch.from_numpy(Xb).to(dev), np.asarray(pairs), n_grid,
                                              None if rows is None else torch.as_tensor(rows).to(dev), ice=ice, **kw)


def _rows_of(Xb, kw):
    return Xb if kw.get("rows") is None else Xb[np.asarray(kw["rows"])]


@pytest.mark.parametrize("name", O2.CASES)
def test_host_twin_matches_the_oracle(name):
    forest, Xb, pairs, NB, kw, want = O2.case(name)
    got = _pd2(forest, Xb, pairs, NB, kw, True)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    err = np.abs(got.numpy() - want).max(initial=0.0)
    tw, tout = kw.get("tree_weight"), kw.get("tree_out")
    tol = O2.tolerance(forest, tw, tout)
    print(f"{name}: per-record err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    n = want.shape[0]
    s = _pd2(forest, Xb, pairs, NB, kw, False)
    assert s.dtype == torch.float64 and tuple(s.shape) == want.shape[1:]
    stol = O2.tolerance(forest, tw, tout, n_sum=n)
    serr = np.abs(s.numpy() - want.sum(0)).max(initial=0.0)
    print(f"{name}: sum err {serr:.3e} tol {stol:.3e}")
    assert serr <= stol
    # the sum mode against the per-record surfaces of the twin itself
    assert np.abs(s.numpy() - got.numpy().sum(0)).max(initial=0.0) <= stol


def test_the_cases_move():
    """The surfaces of the hand-built cases are not flat where they should not be."""
    _, _, _, NB, _, want = O2.case("split_edges_missing")
    s = want[0, 0, :, :, 0]
    assert s[NB - 1, 3] != s[NB - 2, 3] and s[3, NB - 1] != s[3, NB - 2] and s[NB - 1, NB - 1] != s[NB - 2, NB - 2]
    _, _, _, _, _, want = O2.case("repeat_aba")
    assert 64.0 not in want and set(np.unique(want[:, 0])) == {1.0, 2.0, 4.0}
    _, _, _, _, _, want = O2.case("equal_sides")
    assert np.array_equal(want, np.full_like(want, 2.0))


@pytest.mark.parametrize("name", ["k3_missing_rows_dup", "chain12_missing", "split_edges_missing", "repeat_aba"])
def test_swapped_pair_is_the_transpose_bitwise(name):
    forest, Xb, pairs, NB, kw, _ = O2.case(name)
    swapped = [(b, a) for a, b in pairs]
    for ice in (True, False):
        one, two = _pd2(forest, Xb, pairs, NB, kw, ice), _pd2(forest, Xb, swapped, NB, kw, ice)
        assert torch.equal(one, two.transpose(-3, -2))


@pytest.mark.parametrize("name", ["k3_missing_rows_dup", "tree_out_n3", "chain12_missing", "mixed_depths_k3",
                                  "split_edges_missing", "unsplit_mixed"])
def test_tied_to_the_curves_bitwise(name):
    """With one column of the pair at the row's own bin the surface is the 1-D curve of the other column: the same
    integers, so the same bits. With both at the row's own bins it is the unperturbed sum."""
    forest, Xb, pairs, NB, kw, _ = O2.case(name)
    ice2 = _pd2(forest, Xb, pairs, NB, kw, True)
    cols = sorted({c for p in pairs for c in p})
    kw1 = dict(kw)
    rows = kw1.pop("rows", None)
    rt = None if rows is None else torch.as_tensor(rows)
    ice1 = te.forest_partial_dependence(forest, torch.from_numpy(Xb), cols, NB, rt, ice=True, **kw1)
    X = _rows_of(Xb, kw)
    r = torch.arange(X.shape[0])
    for p, (a, b) in enumerate(pairs):
        xa, xb = (torch.from_numpy(X[:, c].astype(np.int64)) for c in (a, b))
        surf = ice2[:, p]                                  # [n, NB, NB, C]
        assert torch.equal(surf[r, :, xb], ice1[:, cols.index(a)])
        assert torch.equal(surf[r, xa, :], ice1[:, cols.index(b)])
        assert torch.equal(surf[r, xa, xb], ice1[r, cols.index(a), xa])
    assert np.ptp(ice2.numpy()) > 0


def test_repeated_pairs_and_one_pair_at_a_time_give_the_same_bits():
    forest, Xb, pairs, NB, kw, _ = O2.case("k3_missing_rows_dup")
    twice = pairs[:2] + pairs[:1] + [(pairs[0][1], pairs[0][0])]
    for ice in (True, False):
        got = _pd2(forest, Xb, twice, NB, kw, ice)
        for p, pair in enumerate(twice):
            alone = _pd2(forest, Xb, [pair], NB, kw, ice)
            assert torch.equal(alone[:, 0] if ice else alone[0], got[:, p] if ice else got[p])


def test_argument_errors():
    forest, Xb, pairs, NB, kw, _ = O2.case("tree_out_n3")
    X = torch.from_numpy(Xb)
    pd2 = te.forest_partial_dependence_pairs
    with pytest.raises(ValueError, match="uint8"):
        pd2(forest, X.to(torch.int32), pairs, NB, **kw)
    with pytest.raises(ValueError, match="different"):
        pd2(forest, X, [(3, 3)], NB, **kw)
    with pytest.raises(ValueError, match="outside"):
        pd2(forest, X, [(0, Xb.shape[1])], NB, **kw)
    with pytest.raises(ValueError, match="outside"):
        pd2(forest, X, [(-1, 0)], NB, **kw)
    with pytest.raises(ValueError, match=r"\[Pn, 2\]"):
        pd2(forest, X, [(0, 1, 2)], NB, **kw)
    with pytest.raises(ValueError, match="n_out"):
        pd2(forest, X, pairs, NB, **dict(kw, n_out=2))
    with pytest.raises(ValueError, match="n_grid"):
        pd2(forest, X, pairs, 257, **kw)
    with pytest.raises(ValueError, match="n_grid"):
        pd2(forest, X, pairs, 0, **kw)
    with pytest.raises(ValueError, match="rows"):
        pd2(forest, X, pairs, NB, torch.tensor([0, Xb.shape[0]]), **kw)
    fm, Xm, pm, _, kwm, _ = O2.case("chain12_missing")
    with pytest.raises(ValueError, match="missing bin"):
        pd2(fm, torch.from_numpy(Xm), pm, NB + 1, **kwm)
    empty = pd2(forest, X, np.zeros((0, 2), np.int64), NB, **kw)
    assert tuple(empty.shape) == (0, NB, NB, 3)
