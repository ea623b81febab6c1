"""``tree_engine.forest_partial_dependence`` on the host: the twin ``tmog_forest_pd_cpu`` against the brute-force
oracle of tests/forest_pd_oracle.py in both modes, tied bit for bit to ``forest_loco`` (the base slot and the delta
of a column at its zero bin), independent of how the columns are requested together, and its argument errors."""
import numpy as np
import pytest
import torch

import forest_pd_oracle as O
from transmogrifai_amd.models import tree_engine as te


def _pd(forest, Xb, cols, n_grid, kw, ice, dev="cpu"):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    return te.forest_partial_dependence(forest, torch.from_numpy(Xb).to(dev), cols, n_grid,
                                        None if rows is None else torch.as_tensor(rows).to(dev), ice=ice, **kw)


@pytest.mark.parametrize("name", O.CASES)
def test_host_twin_matches_the_oracle(name):
    forest, Xb, cols, NB, kw, want = O.case(name)
    got = _pd(forest, Xb, cols, NB, kw, True)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    err = np.abs(got.numpy() - want).max(initial=0.0)
    tol = O.tolerance(forest, kw.get("tree_weight"), kw.get("tree_out"))
    print(f"{name}: ice err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    n = want.shape[0]
    s = _pd(forest, Xb, cols, NB, kw, False)
    assert s.dtype == torch.float64 and tuple(s.shape) == want.shape[1:]
    serr = np.abs(s.numpy() - want.sum(0)).max(initial=0.0)
    stol = O.tolerance(forest, kw.get("tree_weight"), kw.get("tree_out"), n_sum=n)
    print(f"{name}: sum err {serr:.3e} tol {stol:.3e}")
    assert serr <= stol


def test_single_leaves_give_flat_curves_equal_to_the_base():
    forest, Xb, cols, NB, kw, want = O.case("single_leaf_only")
    got = _pd(forest, Xb, cols, NB, kw, True).numpy()
    base = float(forest.value.astype(np.float64).sum())
    assert np.array_equal(got, np.full_like(got, base))


def test_columns_no_tree_splits_on_are_exactly_constant():
    forest, Xb, cols, NB, kw, _ = O.case("q37_unsplit")
    got = _pd(forest, Xb, cols, NB, kw, True).numpy()
    used = set(te.forest_loco_plan(forest).used.tolist())
    flat = [q for q, c in enumerate(cols) if c not in used]
    assert len(flat) == 7
    for q in flat:
        assert np.array_equal(got[:, q], np.repeat(got[:, q, :1], NB, 1))
    assert any(np.ptp(got[:, q], axis=1).max() > 0 for q in range(len(cols)) if q not in flat)


def test_hand_built_curves():
    forest, Xb, cols, NB, kw, _ = O.case("repeat_unreachable")
    got = _pd(forest, Xb, cols, NB, kw, True).numpy()[..., 0]
    assert np.array_equal(got[0, 0], np.where(np.arange(NB) <= 10, 1.0, 4.0))      # 64 is never reached
    forest, Xb, cols, NB, kw, _ = O.case("equal_sides")
    got = _pd(forest, Xb, cols, NB, kw, True).numpy()
    assert np.array_equal(got, np.full_like(got, 2.0))
    forest, Xb, cols, NB, kw, _ = O.case("split_edges_missing")
    got = _pd(forest, Xb, cols, NB, kw, True).numpy()[..., 0]
    # row 0 has column 0 at bin 0 (left, then column 1 = 7 <= 30: value 1); column 0 elsewhere: right, 7 <= 29: 3
    assert np.array_equal(got[0, 0], np.where(np.arange(NB) == 0, 1.0, 3.0))
    # column 1 of that row: bins 0 .. 30 -> 1, the missing bin follows default_left = 0 -> 2
    assert np.array_equal(got[0, 1], np.where(np.arange(NB) <= 30, 1.0, 2.0))


_EXACT = ("chain12_missing", "repeat_unreachable", "split_edges_missing")      # exact_values, unit weights


@pytest.mark.parametrize("name", ["k3_missing_rows_dup", "tree_out_n3", "mixed_depths_k3"] + list(_EXACT))
def test_tied_to_forest_loco_bitwise(name):
    """``ice`` at the row's own bin is ``forest_loco``'s unperturbed slot bit for bit (the same integer: the
    differences cancel there). ``ice`` at a zero bin is the integer ``base + delta`` where ``forest_loco`` holds
    ``delta``: the fp64 difference ``ice - base`` equals ``forest_loco``'s slot bit for bit where the integers
    convert to fp64 exactly (the cases of few-bit values, ``_EXACT``); with rounded values the integers have up to
    62 bits and the two conversions round, each by at most ``2^-53`` of a value within ``3 S``."""
    forest, Xb, _, NB, kw, _ = O.case(name)
    slack = 0.0 if name in _EXACT else 2 * 2.0 ** -53 * 3 * O.L.magnitude(forest, kw.get("tree_weight"))
    rng = np.random.default_rng(5)
    F = Xb.shape[1]
    zb = rng.integers(0, NB, F).astype(np.uint8)
    kw = dict(kw)
    rows = kw.pop("rows", None)
    rt = None if rows is None else torch.as_tensor(rows)
    loco, used = te.forest_loco(forest, torch.from_numpy(Xb), zb, rt, **kw)
    cols = [int(c) for c in used]
    ice = te.forest_partial_dependence(forest, torch.from_numpy(Xb), cols, NB, rt, ice=True, **kw)
    X = Xb if rows is None else Xb[np.asarray(rows)]
    r = torch.arange(X.shape[0])
    for q, c in enumerate(cols):
        own = ice[r, q, torch.from_numpy(X[:, c].astype(np.int64))]
        assert torch.equal(own, loco[:, -1])
        delta = ice[:, q, int(zb[c])] - loco[:, -1]
        if slack == 0.0:
            assert torch.equal(delta, loco[:, q])
        else:
            assert float((delta - loco[:, q]).abs().max()) <= slack
            assert bool((delta[loco[:, q] == 0] == 0).all())        # nothing moves: exactly zero in both
    assert loco[:, :-1].any()


@pytest.mark.parametrize("name", ["q37_unsplit", "k3_missing_rows_dup"])
def test_one_column_at_a_time_gives_the_same_bits(name):
    forest, Xb, cols, NB, kw, _ = O.case(name)
    for ice in (True, False):
        together = _pd(forest, Xb, cols, NB, kw, ice)
        for q, c in enumerate(cols):
            alone = _pd(forest, Xb, [c], NB, kw, ice)
            assert torch.equal(alone[:, 0] if ice else alone[0], together[:, q] if ice else together[q])


def test_sum_is_the_row_sum_of_ice_at_exact_values():
    """Exactly representable weights and values: the sum equals the fp64 sum of the ICE rows bit for bit."""
    forest, Xb, cols, NB, kw, want = O.case("repeat_unreachable")
    assert np.array_equal(_pd(forest, Xb, cols, NB, kw, False).numpy(), want.sum(0))
    assert np.array_equal(_pd(forest, Xb, cols, NB, kw, True).numpy(), want)


def test_argument_errors():
    forest, Xb, cols, NB, kw, _ = O.case("tree_out_n3")
    X = torch.from_numpy(Xb)
    pd = te.forest_partial_dependence
    with pytest.raises(ValueError, match="uint8"):
        pd(forest, X.to(torch.int32), cols, NB, **kw)
    with pytest.raises(ValueError, match="uint8"):
        pd(forest, X[0], cols, NB, **kw)
    with pytest.raises(ValueError, match="outside"):
        pd(forest, X, [0, Xb.shape[1]], NB, **kw)
    with pytest.raises(ValueError, match="outside"):
        pd(forest, X, [-1], NB, **kw)
    with pytest.raises(ValueError, match="distinct"):
        pd(forest, X, [3, 3], NB, **kw)
    with pytest.raises(ValueError, match="n_out"):
        pd(forest, X, cols, NB, **dict(kw, n_out=2))
    with pytest.raises(ValueError, match="n_grid"):
        pd(forest, X, cols, 257, **kw)
    with pytest.raises(ValueError, match="rows"):
        pd(forest, X, cols, NB, torch.tensor([0, Xb.shape[0]]), **kw)
    with pytest.raises(ValueError, match="the matrix has"):
        pd(forest, X[:, :5].contiguous(), [0], NB, **kw)
    fm, Xm, cm, _, kwm, _ = O.case("chain12_missing")
    with pytest.raises(ValueError, match="missing bin"):
        pd(fm, torch.from_numpy(Xm), cm, NB + 1, **kwm)
    empty = pd(forest, X, [], NB, **kw)
    assert tuple(empty.shape) == (0, NB, 3)
