"""``tree_engine.forest_loco`` on the host: the twin ``tmog_forest_loco_cpu`` against the brute-force oracle of
tests/forest_loco_oracle.py on every slot, base slot included.

Tolerance ``T / scale + T 2^-52 S`` (see the oracle module), computed from each case's forest; slots the oracle
gives as exactly 0 must be exactly 0."""
import numpy as np
import pytest
import torch

import forest_loco_oracle as O
from transmogrifai_amd.models import tree_engine as te


def _loco(forest, Xb, zb, kw, dev="cpu"):
    kw = dict(kw)
    rows = kw.pop("rows", None)
    return te.forest_loco(forest, torch.from_numpy(Xb).to(dev), zb,
                          None if rows is None else torch.as_tensor(rows).to(dev), **kw)


@pytest.mark.parametrize("name", O.CASES)
def test_host_twin_matches_bruteforce(name):
    forest, Xb, zb, kw, want = O.case(name)
    got, used = _loco(forest, Xb, zb, kw)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert np.array_equal(used, O.used_columns(forest))
    got = got.numpy()
    tol = O.tolerance(forest, kw.get("tree_weight"), kw.get("tree_out"))
    err = np.abs(got - want).max() if got.size else 0.0
    print(name, "max error", err, "tolerance", tol)
    assert err <= tol
    assert not got[want == 0].any()
    assert want[:, :-1].any() or name in ("single_leaf_only",)     # the case perturbs something


def test_cases_cover_the_listed_shapes():
    cs = {n: O.case(n) for n in O.CASES}
    n_rows = {(len(c[3]["rows"]) if "rows" in c[3] else c[1].shape[0]) for c in cs.values()}
    assert {1, 67} <= n_rows
    assert {1, 5, 37} <= {O.used_columns(c[0]).size for c in cs.values()} and all(c[1].shape[1] <= 40 for c in cs.values())
    assert {1, 9} <= {c[0].n_trees for c in cs.values()}
    shapes = {n: tuple(_loco(*c[:4])[0].shape) for n, c in cs.items()}                 # what the twin returns
    assert all(shapes[n] == c[4].shape for n, c in cs.items())
    layouts = {(c[0].K, shapes[n][2], "tree_out" in c[3]) for n, c in cs.items()}
    assert {(1, 1, False), (3, 3, False), (1, 3, True)} <= layouts
    assert {-1, O.B - 1} <= {c[0].missing_bin for c in cs.values()}
    f, Xb = cs["u5_t9_k3_missing"][:2]
    assert 0.1 < (Xb == O.B - 1).mean() < 0.2 and set(f.default_left[f.nodes[:, 2] >= 0]) == {0, 1}
    rows = cs["u5_t9_k3_missing"][3]["rows"]
    assert len(set(rows.tolist())) < len(rows) and not np.array_equal(rows, np.sort(rows))
    assert any((np.diff(f.tree_off) == 1).any() for f in (c[0] for c in cs.values()))      # a single-leaf tree


def test_group_members_follow_each_other_and_one_is_never_split_on():
    forest, Xb, zb, kw, want = O.case("u37_t9_tree_out_groups")
    g0, g1 = (g.tolist() for g in kw["groups"])
    nd = forest.nodes
    assert any(nd[k, 2] >= 0 and nd[nd[k, 2], 2] >= 0 and {int(nd[k, 0]), int(nd[nd[k, 2], 0])} == set(g0)
               for k in range(len(nd)))
    assert set(g1) - set(O.used_columns(forest).tolist())
    U = O.used_columns(forest).size
    got = _loco(forest, Xb, zb, kw)[0].numpy()
    assert got[:, U].any() and got[:, U + 1].any()
    assert np.abs(got[:, U:U + 2] - want[:, U:U + 2]).max() <= O.tolerance(forest, kw["tree_weight"], kw["tree_out"])


def test_feature_twice_on_a_path_counts_once():
    forest, Xb, zb, kw, want = O.case("repeat_feature")
    got, used = _loco(forest, Xb, zb, kw)
    assert used.tolist() == [0] and want[0, :, 0].tolist() == [3.0, 1.0]
    assert got[0, :, 0].tolist() == [3.0, 1.0]


def test_group_flips_that_end_on_the_original_value_give_exactly_zero():
    forest, Xb, zb, kw, want = O.case("group_back")
    got, used = _loco(forest, Xb, zb, kw)
    assert used.tolist() == [0, 1] and want[0, :, 0].tolist() == [2.0, 1.0, 0.0, 1.0]
    assert got[0, :, 0].tolist() == [2.0, 1.0, 0.0, 1.0]


def test_argument_checks():
    forest, Xb, zb, kw, _ = O.case("chain12_groups")
    X = torch.from_numpy(Xb)
    with pytest.raises(ValueError, match="zero_bins"):
        te.forest_loco(forest, X, zb[:-1])
    with pytest.raises(ValueError, match="disjoint"):
        te.forest_loco(forest, X, zb, groups=[np.asarray([3, 4]), np.asarray([4, 5])])
    with pytest.raises(ValueError, match="outside"):
        te.forest_loco(forest, X, zb, groups=[np.asarray([40])])
    with pytest.raises(ValueError, match="n_out"):
        te.forest_loco(forest, X, zb, tree_out=np.asarray([2]), n_out=2)
