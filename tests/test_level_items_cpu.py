"""The work-item layout of a tree level (``ops/csrc/common/tree_plan.hpp``, shared by the host planner ``grow_group``
and the device planner ``level_plan_kernel``) against the NumPy oracle of tests/level_items_oracle.py, through the
host seam ``tmog_level_items_cpu``: exact, in values and in order. No GPU."""
import numpy as np
import pytest

import level_items_oracle as O
from transmogrifai_amd.ops import _native as N

B_S = 32 * 2                                                    # histogram words per feature
W64, W8 = (0, 64, O.WIDE), (64, 8, O.WIDE)
TABLES = {                                                      # name -> (groups, features, live_dense in features)
    "wide+wide": ([W64, W8], 72, -1),
    "wide+general+csr": ([W64, (64, 7, 0), (71, 31, O.CSR)], 102, 71),
    "wide+general+csr,no-dense-prefix": ([W64, (64, 7, 0), (71, 31, O.CSR)], 102, -1),
    "general+reg+reg": ([(0, 40, 0), (40, 64, O.REG), (104, 10, O.REG)], 114, 40),
    "general": ([(0, 50, 0)], 50, -1),
}


def _counts(chunk_rows):
    return [0, 1, chunk_rows - 1, chunk_rows, chunk_rows + 1, 1023, 1024, 1025, 3 * 1024 + 7]


def _nodes(chunk_rows):
    """Every count as a built splittable node, a built partner that may not split, the derived node of a pair (as its
    left and as its right node) and a node that needs nothing (a leaf); row ranges back to back."""
    built = O.CAN | O.NEED
    kinds = [built, O.NEED, built | O.PAIR_LEFT | O.DERIVED, built | O.DERIVED, 0, built | O.PAIR_LEFT]
    count = np.array([c for c in _counts(chunk_rows) for _ in kinds], np.int64)
    flags = np.array(kinds * len(_counts(chunk_rows)), np.int32)
    begin = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    return count, begin, flags


def _seam(count, begin, flags, groups, chunk_rows, n_sc, live_dense, hsz):
    lib = N.host()
    g = np.array(groups, O.GROUP)
    assert g.itemsize == 12
    p = lambda a: None if a is None else a.ctypes.data
    tot = np.zeros(7, np.int64)
    args = (len(count), p(count), p(begin), p(flags), p(g), len(g), chunk_rows, n_sc, live_dense, hsz)
    lib.tmog_level_items_cpu(*args, None, None, None, None, None, p(tot))
    nh, nc, nl, nz = (int(x) for x in tot[:4])
    hist, part, leaf = np.zeros(nh, O.HIST_ITEM), np.zeros(nc, O.PART_ITEM), np.zeros(nl, O.LEAF_ITEM)
    z_off, z_size, tot2 = np.zeros(nz, np.int64), np.zeros(nz, np.int64), np.zeros(7, np.int64)
    lib.tmog_level_items_cpu(*args, p(hist), p(part), p(leaf), p(z_off), p(z_size), p(tot2))
    np.testing.assert_array_equal(tot, tot2)
    return dict(hist=hist, part=part, leaf=leaf, zero=np.stack([z_off, z_size], 1), n_zero_whole=int(tot[4]),
                n_wide=int(tot[5]), need_general=int(tot[6]))


def test_oracle_flags_are_the_headers():
    C = N.ABI_CONSTS
    assert [C["TMOG_ITEM_" + k] for k in ("SOLE", "REG", "CSR", "LIVE0", "WIDE", "SC_SHIFT")] == \
        [O.SOLE, O.REG, O.CSR, O.LIVE0, O.WIDE, O.SC_SHIFT]
    assert C["TMOG_CSR_ITEM_ROWS"] == C["TMOG_PART_ITEM_ROWS"] == O.ITEM_ROWS


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("n_sc", [1, 3])
@pytest.mark.parametrize("chunk_rows", [512, 4096])
def test_level_items_match_the_oracle(chunk_rows, n_sc, table):
    groups, F, dense_f = TABLES[table]
    hsz, live_dense = F * B_S, dense_f * B_S if dense_f >= 0 else -1
    count, begin, flags = _nodes(chunk_rows)
    got = _seam(count, begin, flags, groups, chunk_rows, n_sc, live_dense, hsz)
    want = O.level_items(count, begin, flags, np.array(groups, O.GROUP), chunk_rows, n_sc, live_dense, hsz)
    for k in ("hist", "part", "leaf", "zero"):
        assert len(got[k]) == len(want[k]), k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("n_zero_whole", "n_wide", "need_general"):
        assert got[k] == want[k], k
    # the zero segments: whole-node segments first, then the CSR regions at offset + live_dense
    nzw = got["n_zero_whole"]
    assert (got["zero"][:nzw, 1] == hsz).all() and (got["zero"][:nzw, 0] % hsz == 0).all()
    assert (got["zero"][nzw:, 0] % hsz == live_dense).all() and (got["zero"][nzw:, 1] == hsz - live_dense).all()
    assert (len(got["zero"]) > nzw) == (table == "wide+general+csr" and chunk_rows == 4096)
    # wide-load items first, and no derived or unneeded node has histogram items
    wide = (got["hist"]["excl"] & O.WIDE) != 0
    assert wide[:got["n_wide"]].all() and not wide[got["n_wide"]:].any()
    slot_flags = flags[(flags & O.NEED) != 0]
    assert not (slot_flags[got["hist"]["node"]] & O.DERIVED).any()
    assert set(got["part"]["node"]) == set(range(len(slot_flags)))          # derived nodes are still partitioned
    # every row of a built node once per feature group and statistic chunk, of a leaf once
    built = np.flatnonzero((slot_flags & O.DERIVED) == 0)
    per_node = np.bincount(got["hist"]["node"], got["hist"]["count"], len(slot_flags))
    n_lds = sum(1 for g in groups if not g[2] & (O.REG | O.CSR))
    slot_count = count[(flags & O.NEED) != 0]
    np.testing.assert_array_equal(per_node[built], slot_count[built] * (len(groups) + n_lds * (n_sc - 1)))
    assert got["leaf"]["count"].sum() == count[(flags & O.NEED) == 0].sum() and (got["leaf"]["count"] > 0).all()


@pytest.mark.parametrize("chunk_rows", [512, 4096])
def test_item_boundaries_have_no_empty_item(chunk_rows):
    """A node of exactly k * 1024 rows has k partition and k CSR items; of k * chunk_rows rows, k items per other group
    and k leaf items; none of them empty, and an item is marked sole exactly when its group has one."""
    groups, F, dense_f = TABLES["wide+general+csr"]
    for c in (1024, 2048, 4096, 3 * 4096):
        for fl in (O.CAN | O.NEED, 0):
            got = _seam(np.array([c], np.int64), np.array([5], np.int64), np.array([fl], np.int32), groups, chunk_rows,
                        1, dense_f * B_S, F * B_S)
            for k in ("hist", "part", "leaf"):
                assert (got[k]["count"] > 0).all()
            if fl == 0:
                assert len(got["hist"]) == len(got["part"]) == 0
                assert len(got["leaf"]) == -(-c // chunk_rows)                  # = c / chunk_rows at its multiples
                continue
            csr = (got["hist"]["excl"] & O.CSR) != 0
            sole = (got["hist"]["excl"] & O.SOLE) != 0
            assert len(got["part"]) == csr.sum() == c // 1024
            assert (~csr).sum() == 2 * -(-c // chunk_rows)
            assert (sole[csr] == (c == 1024)).all() and (sole[~csr] == (c <= chunk_rows)).all()


def test_empty_root_takes_one_item_of_each_kind():
    groups, F, dense_f = TABLES["wide+general+csr"]
    got = _seam(np.zeros(1, np.int64), np.zeros(1, np.int64), np.array([O.NEED], np.int32), groups, 512, 1,
                dense_f * B_S, F * B_S)
    assert len(got["part"]) == 1 and len(got["hist"]) == 3 and len(got["zero"]) == len(got["leaf"]) == 0
    assert (got["hist"]["count"] == 0).all() and ((got["hist"]["excl"] & O.SOLE) != 0).all()
