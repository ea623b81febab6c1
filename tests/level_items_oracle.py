"""NumPy oracle of a tree level's work-item layout, written from the ``FeatGroup`` / ``HistItem`` / ``PartItem`` /
``LeafItem`` comments of ``ops/csrc/common/tmog_abi.h`` -- not from ``common/tree_plan.hpp``, which it judges through
``tmog_level_items_cpu`` (tests/test_level_items_cpu.py). Plain loops that append items in list order."""
from __future__ import annotations

import numpy as np

from tree_level_oracle import HIST_ITEM, LEAF_ITEM, PART_ITEM

SOLE, REG, CSR, LIVE0, WIDE, SC_SHIFT = 1, 2, 4, 8, 16, 8      # HistItem.excl (the test checks them against the header)
CAN, NEED, PAIR_LEFT, DERIVED = 1, 2, 4, 8                      # per-node bits of tmog_level_items_cpu
ITEM_ROWS = 1024                                                # TMOG_CSR_ITEM_ROWS = TMOG_PART_ITEM_ROWS
GROUP = np.dtype([("f0", "<i4"), ("nf", "<i4"), ("flags", "<i4")])


def _slices(begin, count, step):
    """(begin, count) of the items that cover a node's rows; a node of no rows still takes one (empty) item."""
    return [(begin + o, min(step, count - o)) for o in range(0, count, step)] or [(begin, 0)]


def level_items(count, begin, flags, groups, chunk_rows, n_sc, live_dense, hsz):
    slot, hist, part, leaf, z_whole, z_csr = 0, {True: [], False: []}, [], [], [], []
    leaf_out = 0
    for i, (c, b, fl) in enumerate(zip(map(int, count), map(int, begin), map(int, flags))):
        if not fl & NEED:                                        # collected as a leaf: gid i, buffer 0
            for lb, lc in _slices(b, c, chunk_rows) if c > 0 else []:
                leaf.append((lb, lc, leaf_out + lb - b, i, 0))
            leaf_out += max(c, 0)
            continue
        part += [(slot, 0, pb, pc, 0, 0) for pb, pc in _slices(b, c, ITEM_ROWS)]
        if not fl & DERIVED:
            split_rows = split_csr = False
            for g in groups:
                f0, nf, gf = int(g["f0"]), int(g["nf"]), int(g["flags"])
                rows = _slices(b, c, ITEM_ROWS if gf & CSR else chunk_rows)
                x = gf | (SOLE if len(rows) == 1 else 0) | (LIVE0 if gf & (REG | CSR) and live_dense >= 0 else 0)
                for sc in range(1 if gf & (REG | CSR) else n_sc):
                    hist[bool(gf & WIDE)] += [(slot, f0, nf, x | sc << SC_SHIFT, hb, hc) for hb, hc in rows]
                if len(rows) > 1:
                    split_csr |= bool(gf & CSR)
                    split_rows |= not gf & CSR
            if split_rows or (split_csr and not 0 <= live_dense < hsz):
                z_whole.append((slot * hsz, hsz))
            elif split_csr:
                z_csr.append((slot * hsz + live_dense, hsz - live_dense))
        slot += 1
    n_general = sum(1 for it in hist[False] if not it[3] & CSR)
    return dict(hist=np.array(hist[True] + hist[False], HIST_ITEM), part=np.array(part, PART_ITEM),
                leaf=np.array(leaf, LEAF_ITEM), zero=np.array(z_whole + z_csr, np.int64).reshape(-1, 2),
                n_zero_whole=len(z_whole), n_wide=len(hist[True]), need_general=int(n_general > 0))
