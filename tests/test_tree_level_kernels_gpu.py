"""Kernel-level oracle tests of the per-level tree kernels: ``hist_build_kernel`` (byte gather, register accumulation,
CSR and wide-load items), ``hist_subtract_kernel`` and ``zero_segments_kernel`` of ``ops/csrc/hip/tree_hist_kernels.hip``,
``partition_fused_kernel`` and ``leaf_collect_kernel`` of ``ops/csrc/hip/tree_partition_kernels.hip``, each driven through its C entry point with ctypes on crafted
inputs and compared with the NumPy oracle of tests/tree_level_oracle.py (validated against the host twins in
tests/test_tree_level_oracle.py).

All arithmetic is integer: every comparison is exact and covers the whole output buffer, which starts filled with a
sentinel, so a write outside the contract's words fails the test as surely as a wrong sum. Items are hand-built under
the grower's preconditions (``group_layout`` / ``grow_group`` in ``common/tree_grow.hpp``), quoted where used."""
import numpy as np
import pytest
import torch

import tree_level_oracle as O
from transmogrifai_amd.ops._native import ABI_CONSTS

SENT, SENT32 = O.SENT, O.SENT32
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025, 4096]          # rows per item (chunk_rows = 4096)
# HistItem.excl bits and the statistic-chunk shift, as common/tmog_abi.h names them
X_ONE, X_REG, X_CSR, X_LIVE0, X_WIDE, X_SC = (ABI_CONSTS["TMOG_ITEM_" + k]
                                              for k in ("SOLE", "REG", "CSR", "LIVE0", "WIDE", "SC_SHIFT"))


def test_item_flags_keep_their_values():
    assert (X_ONE, X_REG, X_CSR, X_LIVE0, X_WIDE, X_SC) == (1, 2, 4, 8, 16, 8)


def _lib():
    from transmogrifai_amd.ops import _native
    return _native.hip()


def _st():
    from transmogrifai_amd.ops import _native
    return _native.stream()


_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}


def _d(a):
    """Host array -> device tensor of the same bytes."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    if a.dtype in _SIGNED:                     # same bits: torch has no arithmetic on the unsigned types
        a = a.view(_SIGNED[a.dtype])
    return torch.from_numpy(a).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _items(rows):
    return np.array([tuple(r) for r in rows], O.HIST_ITEM)


def _chunks(begin, count, step):
    return [(begin + o, min(step, count - o)) for o in range(0, count, step)]


# --------------------------------------------------------------------------------------------- build harness
def _zero(lib, hist, z, B, S):
    off, size = np.asarray(z["off"], np.int64), np.asarray(z["size"], np.int64)
    dn = _d(np.asarray(z["dn"], np.int32)) if z.get("dn") is not None else None
    n_host = z.get("n_host", len(off))
    doff, dsize = _d(off), _d(size)
    rc = lib.tmog_hip_zero_segments(_p(hist), _p(doff), _p(dsize), n_host, int(size.max()), z.get("dense", -1),
                                    B * S, S, _st(), z.get("n_dense_host", z.get("n_dense", len(off))), _p(dn))
    torch.cuda.synchronize()
    assert rc == 0


def _zero_expect(buf, z, B, S):
    n, n_dense = len(z["off"]), z.get("n_dense", len(z["off"]))
    if z.get("dn") is not None:
        n, n_dense = z["dn"]
    for j in range(n):
        dj = z.get("dense", -1) if j < n_dense else 0
        buf[int(z["off"][j]) + O.live_region(int(z["size"][j]), dj, B * S, S)] = 0


def _build(L, items, *, skip_bin=-1, csr=None, Sc=0, need_general=1, gh=None, dcount=None, Xh=None, zero=None,
           Xb_dev=None, rc_want=0):
    """Sentinel buffer -> (zero_segments of the atomically accumulated nodes) -> one tmog_hip_hist_build launch ->
    the whole buffer back on the host."""
    lib = _lib()
    hist = _d(np.full(L["hist_words"], SENT, np.int64))
    if zero is not None:
        _zero(lib, hist, zero, L["B"], L["S"])
    keep = [_d(L[k]) for k in ("rows", "node_feat_off", "feat_list", "node_model", "node_hist_off", "y", "t1", "t2",
                               "qscale")]
    rows, nfo, fl, nmd, nho, y, t1, t2, qs = keep
    xb = Xb_dev if Xb_dev is not None else _d(L["Xb"])
    it = _d(items)
    ptr, col = csr if csr is not None else (None, None)
    ghd = _d(None if gh is None else np.asarray(gh, np.int32))
    dc = _d(None if dcount is None else np.array([dcount], np.int32))
    xh = _d(Xh)
    rc = lib.tmog_hip_hist_build(_p(xb), L["F"], _p(rows), _p(it), len(items), _p(nfo), _p(fl), _p(nmd), _p(nho),
                                 _p(hist), L["B"], L["mode"], L["S"], _p(y), _p(t1), _p(t2), L["stride"], _p(qs),
                                 skip_bin, _p(ptr), _p(col), Sc, 0, need_general, _st(), _p(ghd), _p(dc), L["wide"],
                                 _p(xh), 0 if Xh is None else Xh.shape[1])
    torch.cuda.synchronize()
    assert rc == rc_want
    return hist.cpu().numpy()


def _expect(L, items, *, Sc=0, gh=None, dcount=None, zero=None):
    """The buffer the contract prescribes. An item writes, for its features [fg0, fg0 + nf) of its node: bin 0 only
    (CSR items, excl bit 3), its statistic chunk (Sc) or every word; with plain stores (excl bit 0) or by adding to
    what zero_segments left."""
    B, S = L["B"], L["S"]
    buf = np.full(L["hist_words"], SENT, np.int64)
    if zero is not None:
        _zero_expect(buf, zero, B, S)
    cache = {}                                    # the statistic chunks of one row chunk share its histogram
    for it in items[:len(items) if dcount is None else dcount]:
        j, f0, nf, x = int(it["node"]), int(it["fg0"]), int(it["nf"]), int(it["excl"])
        key = (j, int(it["begin"]), int(it["count"]), f0, nf)
        if key not in cache:
            cache[key] = O.level_hist(L, *key[:3], f0, nf, gh)
        H = cache[key]
        idx = int(L["node_hist_off"][j]) + f0 * B * S + np.arange(nf * B * S, dtype=np.int64).reshape(nf, B, S)
        if x & (X_CSR | X_LIVE0):
            idx, H = idx[:, 0, :], H[:, 0, :]
        elif Sc:
            s0 = ((x >> X_SC) & 0xFF) * Sc
            idx, H = idx[:, :, s0:s0 + Sc], H[:, :, s0:s0 + Sc]
        if x & X_ONE:
            buf[idx] = H
        else:
            buf[idx] += H
    return buf


def _node_zero(L, nodes, dense=-1):
    return dict(off=[int(L["node_hist_off"][j]) for j in nodes], size=[L["per_node"]] * len(nodes), dense=dense)


def _std_items(L, f0, nf, excl=0, single=None, multi=None, step=1025):
    """One single-chunk item (excl bit 0) per node of ``single``; ``multi`` nodes are cut into ``step``-row chunks
    that accumulate atomically (bit 0 clear: "nit == 1 ? TMOG_ITEM_SOLE : 0", hist_item_at in common/tree_plan.hpp)."""
    rows = []
    for j in single:
        rows.append((j, f0, nf, excl | X_ONE, L["node_begin"][j], L["node_count"][j]))
    for j in multi:
        for b, c in _chunks(int(L["node_begin"][j]), int(L["node_count"][j]), step):
            rows.append((j, f0, nf, excl, b, c))
    return _items(rows)


# ----------------------------------------------------------------------------------------- byte-gather path
@pytest.mark.gpu
@pytest.mark.parametrize("nf", [1, 3, 21, 32, 33, 64])
@pytest.mark.parametrize("mode,S", [(0, 2), (0, 5), (1, 3), (2, 2)])
def test_hist_byte_gather(mode, S, nf):
    """hist_build_kernel's general path, skip_bin = -1: 64 / nf rows per wave-instruction (64, 21 with an idle lane,
    3, 2, 1, 1), every row count around the 64-row wave chunk and the 256-row pass, nodes of one chunk (plain
    stores) and a node of three chunks, the last one short (atomics onto zero_segments' zeros), two models with
    different scales, weights 0 / 1 / 2 / 255, permuted feature lists at node_feat_off != 0, fg0 = 2."""
    rng = np.random.default_rng(100 * mode + 10 * S + nf)
    B = 5
    counts = COUNTS + [1025 + 1025 + 77]
    L = O.make_level(rng, counts, F=nf + 6, nfeat=nf + 3, B=B, mode=mode, S=S)
    multi = [len(counts) - 1]
    items = _std_items(L, 2, nf, single=range(len(COUNTS)), multi=multi)
    assert len(items) == len(COUNTS) + 3 and items[-1]["count"] == 77
    zero = _node_zero(L, multi)                   # "if (nch > 1) z_off.push_back(hoff[j])": whole node, live_dense
    got = _build(L, items, zero=zero)
    np.testing.assert_array_equal(got, _expect(L, items, zero=zero))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [3, 40, 256])
def test_hist_stat_chunks(S):
    """Mode 0 with B = 256: B x S does not fit the LDS table, so each statistic chunk [c * Sc, c * Sc + Sc) is its
    own item (chunk index from excl bit TMOG_ITEM_SC_SHIFT up, hist_item_at in common/tree_plan.hpp) writing disjoint
    words; the last chunk of S = 3 is narrower than Sc. Every class occurs, so the first and last slot of every chunk is hit."""
    lib = _lib()
    B, nf = 256, 5
    Sc = lib.tmog_hip_hist_stat_chunk(B, S)
    assert 1 <= Sc < S and lib.tmog_hip_hist_stat_chunk(4, 3) == 3
    n_sc = (S + Sc - 1) // Sc
    rng = np.random.default_rng(S)
    counts = [700, 300 + 300 + 50]
    L = O.make_level(rng, counts, F=8, nfeat=7, B=B, mode=0, S=S, N=1400)
    L["y"] = (np.arange(L["N"]) % S).astype(np.float32)
    L["rows"][:700] = O.pack(np.arange(700), rng.choice([1, 2, 255], 700))
    rows = []
    for sc in range(n_sc):
        rows.append((0, 1, nf, X_ONE | (sc << X_SC), 0, 700))
        rows += [(1, 1, nf, sc << X_SC, b, c) for b, c in _chunks(700, 650, 300)]
    items = _items(rows)
    zero = _node_zero(L, [1])
    got = _build(L, items, Sc=Sc, zero=zero)
    want = _expect(L, items, Sc=Sc, zero=zero)
    np.testing.assert_array_equal(got, want)
    H0 = want[int(L["node_hist_off"][0]):][:L["per_node"]].reshape(7, B, S)[1:6]
    assert (H0.sum(axis=(0, 1)) > 0).all()                                 # every class slot received counts


# ------------------------------------------------------------------------------- sparse missing bin, byte path
@pytest.mark.gpu
def test_hist_sparse_missing_bin_byte_path():
    """Mode 2 with skip_bin = B - 1: rows in the missing bin issue no atomic and the word is recovered as chunk total
    minus the other bins. A feature with every row missing, one with none, three mixed; g of both signs."""
    rng = np.random.default_rng(7)
    B, nf = 8, 5
    counts = [1, 65, 257, 4096, 1025 + 1025 + 77]
    L = O.make_level(rng, counts, F=9, nfeat=8, B=B, mode=2, S=2, perm=False)
    L["Xb"][:, 2] = B - 1
    L["Xb"][:, 3] = rng.integers(0, B - 1, L["N"])
    items = _std_items(L, 2, nf, single=range(4), multi=[4])
    zero = _node_zero(L, [4])
    got = _build(L, items, skip_bin=B - 1, zero=zero)
    want = _expect(L, items, zero=zero)
    np.testing.assert_array_equal(got, want)
    H = want[int(L["node_hist_off"][3]):][:L["per_node"]].reshape(8, B, 2)
    assert (H[2, :B - 1] == 0).all() and H[2, B - 1, 0] < 0 < H[2, B - 1, 1]       # all missing, negative g sum
    assert (H[3, B - 1] == 0).all() and (H[4, B - 1] != 0).all()
    # the same histograms without the sparse path
    np.testing.assert_array_equal(_build(L, items, skip_bin=-1, zero=zero), want)


# ------------------------------------------------------------------------------------------- register path
@pytest.mark.gpu
@pytest.mark.parametrize("live0", [0, 1])
@pytest.mark.parametrize("nf", [7, 64])
def test_hist_register_path(nf, live0):
    """excl bit 1 ("FeatGroup{n_multi + g.f0, g.nf, GPU ? TMOG_ITEM_REG : 0}": one-present-bin columns, sparse mode
    only): bins in {0, skip_bin}. With excl bit 3 ("(reg || csr) && live_dense >= 0 ? TMOG_ITEM_LIVE0 : 0") only the
    first S words -- bin 0 -- of each feature are written; without it (no multi-bin column, live_dense = -1) all
    B x S."""
    rng = np.random.default_rng(nf + live0)
    B, n_multi = 8, 2
    counts = [1, 64, 65, 1025, 4096, 1025 + 1025 + 77]
    L = O.make_level(rng, counts, F=n_multi + nf, nfeat=n_multi + nf, B=B, mode=2, S=2, perm=False)
    L["Xb"][:, n_multi:] = np.where(rng.random((L["N"], nf)) < 0.3, 0, B - 1)
    items = _std_items(L, n_multi, nf, excl=X_REG | (X_LIVE0 if live0 else 0), single=range(5), multi=[5])
    zero = _node_zero(L, [5], dense=n_multi * B * 2 if live0 else -1)
    got = _build(L, items, skip_bin=B - 1, zero=zero)
    want = _expect(L, items, zero=zero)
    np.testing.assert_array_equal(got, want)
    per_f = got[int(L["node_hist_off"][4]):][:L["per_node"]].reshape(n_multi + nf, B * 2)[n_multi:]
    assert (per_f[:, 2:] == SENT).all() if live0 else (per_f[:, -2:] != SENT).all()


# ------------------------------------------------------------------------------------------------ CSR items
def _csr_level(rng, B, n_multi, n_one, lengths, counts):
    """Rows whose one-present-bin columns hold bin 0 in exactly ``lengths[r % len(lengths)]`` places (row 0: none, so
    its empty list sits at ptr = 0), the CSR ``tree_engine.onebin_csr`` builds from that matrix, and nodes of
    ``counts`` random entries."""
    from transmogrifai_amd.models import tree_engine as TE
    N, F = 2048, n_multi + n_one
    Xb = rng.integers(0, B, (N, F)).astype(np.uint8)               # multi-bin columns: rows in the missing bin too
    lens = np.asarray(lengths)[np.arange(N) % len(lengths)]
    assert lens[0] == 0
    one = np.full((N, n_one), B - 1, np.uint8)
    for r in range(N):
        one[r, rng.permutation(n_one)[:lens[r]]] = 0
    Xb[:, n_multi:] = one
    L = O.make_level(rng, counts, F=F, nfeat=F, B=B, mode=2, S=2, Xb=Xb, perm=False)
    n_bins = np.array([B] * n_multi + [1] * n_one)
    ptr, col, n_cols = TE.onebin_csr(_d(Xb), n_bins)
    assert n_cols == n_one and int(ptr[1]) == 0 and int(ptr[-1]) == int(lens.sum())
    return L, lens, (ptr, col)


@pytest.mark.gpu
@pytest.mark.parametrize("B,n_one,lengths", [(4, 158, [0, 1, 8, 9, 16, 17, 32, 33, 64, 65, 130]),
                                             (2, 30, [0, 1, 8, 9, 16, 17, 30])], ids=["B4-158", "B2-30"])
def test_hist_csr_items(B, n_one, lengths):
    """excl bit 2: one item covers all one-present-bin columns of a row chunk and walks the rows' CSR lists; only
    bin 0 words are written. n_one is the most the grower's guard "2 * n_one + 4 + 64 * 4 <= 64 * (B * S + 1)" admits
    for this B. List lengths mixed inside a 64-row wave chunk (item sizes 1, 64, 65, 1024) and uniform per chunk
    (every lane-group width W = 8 / 16 / 32 / 64 and the tail of lists longer than 64); a node of three items
    accumulates onto its zeroed one-present-bin region ("zc_off.push_back(hoff[j] + live_dense)")."""
    assert 2 * n_one + 4 + 64 * 4 <= 64 * (B * 2 + 1) < 2 * (n_one + 1) + 4 + 64 * 4
    rng = np.random.default_rng(B)
    n_multi = 4
    counts = [1, 64, 65, 1024] + [64] * len(lengths) + [1024 + 1024 + 100]
    L, lens, csr = _csr_level(rng, B, n_multi, n_one, lengths, counts)
    L["rows"][0] = O.pack([0], [3])[0]                                     # node 0: row 0, the empty list at ptr 0
    for k in range(len(lengths)):                                          # uniform chunks: one list length each
        b = int(L["node_begin"][4 + k])
        cand = np.nonzero(np.arange(L["N"]) % len(lengths) == k)[0]
        L["rows"][b:b + 64] = O.pack(rng.choice(cand, 64), rng.choice([1, 2, 255], 64))
    last = len(counts) - 1
    items = _std_items(L, n_multi, n_one, excl=X_CSR | X_LIVE0, single=range(last), multi=[last], step=1024)
    dense = n_multi * B * 2
    zero = dict(off=[int(L["node_hist_off"][last]) + dense], size=[L["per_node"] - dense], dense=dense, n_dense=0)
    want = _expect(L, items, zero=zero)
    for need_general in (0, 1):
        got = _build(L, items, skip_bin=B - 1, csr=csr, zero=zero, need_general=need_general)
        np.testing.assert_array_equal(got, want)
    k = len(lengths) - 1                                                   # the longest lists: every entry counted
    H = want[int(L["node_hist_off"][4 + k]):][:L["per_node"]].reshape(-1, B, 2)[n_multi:, 0, 1]
    e = L["rows"][int(L["node_begin"][4 + k]):][:64]
    assert H.sum() == (O.stage(2, e, 0, 2, t1=L["t1"][(4 + k) % 2], t2=L["t2"][(4 + k) % 2],
                               qs=L["qscale"][(4 + k) % 2])[:, 1] * lengths[-1]).sum()


# ------------------------------------------------------------------------------------------ wide-load items
WIDE_NF = [1, 3, 4, 5, 8, 9, 17, 33, 63, 64]                  # dwords 1, 1, 1, 2, 2, 3, 5, 9, 16, 16 -> NP 1 .. 16


@pytest.mark.gpu
@pytest.mark.parametrize("xh", [0, 1], ids=["Xb", "Xh"])
@pytest.mark.parametrize("sparse", [0, 1], ids=["dense", "skip"])
@pytest.mark.parametrize("B", [2, 32, 64])
def test_hist_wide_items(B, sparse, xh):
    """excl bit 4 ("wide_ok": mode 2, S = 2, F % 4 == 0, N * F < 2^31 - 64; "perm_feats[g.f0] % 4 == 0" and
    contiguous columns; with a compact matrix "a.Fh % 4 == 0 && perm_feats[g.f0] + g.nf <= a.Fh"): 4 bins per load,
    (g, h) packed into one 64-bit LDS word. Every dword-count padding NP, negative g with h >= 0, skip_bin -1 and
    B - 1. With Xh the items must read the compact matrix only: the Xb argument then holds other bins."""
    rng = np.random.default_rng(4 * B + 2 * sparse + xh)
    F, Fh = 80, 72
    counts = [1, 63, 64, 65, 255, 256, 257, 1025, 4096, 100, 1025 + 1025 + 77]
    L = O.make_level(rng, counts, F=F, nfeat=Fh, B=B, mode=2, S=2, perm=False)
    rows = [(k, 4 * (k % 3), nf, X_WIDE | X_ONE, L["node_begin"][k], L["node_count"][k])
            for k, nf in enumerate(WIDE_NF)]
    rows += [(10, 8, 17, X_WIDE, b, c) for b, c in _chunks(int(L["node_begin"][10]), counts[10], 1025)]
    items = _items(rows)
    zero = _node_zero(L, [10])
    kw = {}
    if xh:
        kw = dict(Xh=np.ascontiguousarray(L["Xb"][:, :Fh]), Xb_dev=_d(B - 1 - L["Xb"]))
    want = _expect(L, items, zero=zero)
    for need_general in (0, 1):
        got = _build(L, items, skip_bin=B - 1 if sparse else -1, zero=zero, need_general=need_general, **kw)
        np.testing.assert_array_equal(got, want)
    assert want[want != SENT].min() < -(1 << 16)


# ------------------------------------------------------------------------ instantiations, mixed lists, staged gh
def _xgb_level():
    """An XGBoost-shaped level, B = 4 with the missing bin 3: columns [0, 8) multi-bin and dword aligned (a wide-load
    group), [8, 13) multi-bin (a byte-gather group), [13, 44) one present bin (the CSR group, or a register group).
    Nodes 0 and 1 fit one chunk; node 2 takes three 1024-row chunks."""
    rng = np.random.default_rng(44)
    L, _, csr = _csr_level(rng, 4, 13, 31, [0, 3, 9, 20, 31], [300, 1025, 1024 + 1024 + 52])
    dense = 13 * 4 * 2
    wide = _std_items(L, 0, 8, excl=X_WIDE, single=[0, 1], multi=[2], step=1024)
    byte = _std_items(L, 8, 5, single=[0, 1], multi=[2], step=1024)
    csri = _std_items(L, 13, 31, excl=X_CSR | X_LIVE0, single=[0], multi=[2], step=1024)
    reg = _std_items(L, 13, 31, excl=X_REG | X_LIVE0, single=[1], multi=[])
    zero = _node_zero(L, [2], dense=dense)
    return L, csr, wide, byte, csri, reg, zero


def _staged(L):
    """The int2 (q(w g), q(w h)) of every entry, in entry order (what the boosting prologue stages as gh_words)."""
    gh = np.zeros((L["rows"].size, 2), np.int32)
    for j in range(len(L["node_count"])):
        b, c, m = int(L["node_begin"][j]), int(L["node_count"][j]), int(L["node_model"][j])
        gh[b:b + c] = O.stage(2, L["rows"][b:b + c], L["wide"], 2, t1=L["t1"][m], t2=L["t2"][m], qs=L["qscale"][m])
    return gh


@pytest.mark.gpu
def test_hist_instantiations_and_mixed_item_list():
    """hist_build_kernel<2, false> (need_general = 0: CSR and wide-load items only) gives the buffer of the general
    instantiation; a list mixing wide-load, byte-gather, CSR and register items runs in one launch."""
    L, csr, wide, byte, csri, reg, zero = _xgb_level()
    two = np.concatenate([wide, csri])
    want = _expect(L, two, zero=zero)
    a = _build(L, two, skip_bin=3, csr=csr, zero=zero, need_general=0)
    b = _build(L, two, skip_bin=3, csr=csr, zero=zero, need_general=1)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, want)
    mixed = np.concatenate([wide[:1], byte[:1], csri[:1], reg, byte[1:], csri[1:], wide[1:]])
    kinds = {int(x) & (X_REG | X_CSR | X_WIDE) for x in mixed["excl"]}
    assert kinds == {0, X_REG, X_CSR, X_WIDE}
    got = _build(L, mixed, skip_bin=3, csr=csr, zero=zero, need_general=1)
    want = _expect(L, mixed, zero=zero)
    np.testing.assert_array_equal(got, want)
    # node 1: the register group recovers what a CSR item would have written for the same columns
    assert (want[int(L["node_hist_off"][1]):][:L["per_node"]] != SENT).sum() == 13 * 4 * 2 + 31 * 2


@pytest.mark.gpu
def test_hist_staged_gh_equals_float_input():
    """Staged ``gh_words`` (the entry's quantised pair rides with the entry) against float t1 / t2 input: the same
    histograms on the byte (sparse and not), register, CSR and wide-load paths."""
    L, csr, wide, byte, csri, reg, zero = _xgb_level()
    gh = _staged(L)
    mixed = np.concatenate([wide, byte, csri, reg])
    want = _expect(L, mixed, zero=zero)
    np.testing.assert_array_equal(_expect(L, mixed, zero=zero, gh=gh), want)
    np.testing.assert_array_equal(_build(L, mixed, skip_bin=3, csr=csr, zero=zero), want)
    np.testing.assert_array_equal(_build(L, mixed, skip_bin=3, csr=csr, zero=zero, gh=gh), want)
    # staged values the float input cannot have produced: the kernels must take them as given
    gh2 = (gh.astype(np.int64) * 3 + 1).astype(np.int32)
    np.testing.assert_array_equal(_build(L, mixed, skip_bin=3, csr=csr, zero=zero, gh=gh2),
                                  _expect(L, mixed, zero=zero, gh=gh2))
    dense_items = np.concatenate([wide, byte])                             # skip_bin = -1: no sparse recovery
    np.testing.assert_array_equal(_build(L, dense_items, zero=zero, gh=gh2), _expect(L, dense_items, zero=zero, gh=gh2))


# --------------------------------------------------------------------------------------- quantisation bound
QMAX = 524286                         # tree_engine.quant_qmax(): (2^31 - 1) // 4096 - 1


@pytest.mark.gpu
@pytest.mark.parametrize("skip_bin", [-1, 3])
def test_hist_quantisation_bound(skip_bin):
    """4096 rows (chunk_rows) with staged q = +-524286 all in one bin of a feature: the int32 LDS word -- and the
    low half of the wide path's packed 64-bit word -- reaches 2 147 475 456 without wrapping or carrying; a 1024-row
    CSR item with q = 4 x 524286 reaches the same. Column c holds bin c % 4 in every row; with skip_bin = 3 a
    quarter of the columns sit wholly in the missing bin, whose word comes from the chunk totals at the bound."""
    from transmogrifai_amd.models import tree_engine as TE
    assert TE.quant_qmax() == QMAX and 4096 * QMAX == 2_147_475_456 < 2 ** 31
    rng = np.random.default_rng(1)
    B, F = 4, 64
    Xb = np.tile((np.arange(F) % B).astype(np.uint8), (4096, 1))
    L = O.make_level(rng, [4096, 4096], F=F, nfeat=F, B=B, mode=2, S=2, Xb=Xb, perm=False)
    gh = np.zeros((8192, 2), np.int32)
    gh[:4096] = [QMAX, QMAX]
    gh[4096:] = [-QMAX, QMAX]
    for excl in (0, X_WIDE):
        items = _std_items(L, 0, 64, excl=excl, single=[0, 1], multi=[])
        want = _expect(L, items, gh=gh)
        np.testing.assert_array_equal(_build(L, items, skip_bin=skip_bin, gh=gh), want)
        live = want[want != SENT]
        assert live.max() == 2_147_475_456 and live.min() == -2_147_475_456
    if skip_bin < 0:
        return
    # CSR: columns [4, 64) as one-present-bin columns whose every row holds bin 0
    Xb2 = Xb[:1024].copy()
    Xb2[:, 4:] = 0
    L2 = O.make_level(rng, [1024, 1024], F=F, nfeat=F, B=B, mode=2, S=2, Xb=Xb2, perm=False)
    ptr, col, _ = TE.onebin_csr(_d(Xb2), np.array([3] * 4 + [1] * 60))
    gh2 = np.zeros((2048, 2), np.int32)
    gh2[:1024] = [4 * QMAX, 4 * QMAX]
    gh2[1024:] = [-4 * QMAX, 4 * QMAX]
    items = _std_items(L2, 4, 60, excl=X_CSR | X_LIVE0, single=[0, 1], multi=[])
    want = _expect(L2, items, gh=gh2)
    np.testing.assert_array_equal(_build(L2, items, skip_bin=3, csr=(ptr, col), gh=gh2, need_general=0), want)
    live = want[want != SENT]
    assert live.max() == 2_147_475_456 and live.min() == -2_147_475_456


# --------------------------------------------------------------------------------------------- row id range
@pytest.mark.gpu
@pytest.mark.parametrize("wide_rows", [0, 1], ids=["packed", "wide_rows"])
def test_hist_row_id_range(wide_rows):
    """Packed entries address rows 0 and 2^24 - 1 of an N = 2^24, F = 4 matrix (the weight byte must not leak into
    the row); wide_rows entries are 32-bit ids >= 2^24 with N * F < 2^31 - 64. Byte-gather and wide-load items."""
    rng = np.random.default_rng(wide_rows)
    N = (1 << 24) + (4096 if wide_rows else 0)
    B, F = 8, 4
    assert N * F < (1 << 31) - 64
    Xb = np.zeros((N, F), np.uint8)
    ids = np.unique(np.concatenate([[N - 1, N - 2, (1 << 24) - 1] + ([1 << 24] if wide_rows else [0, 1]),
                                    rng.integers((1 << 24) if wide_rows else 0, N, 200)]))
    Xb[ids] = rng.integers(1, B, (ids.size, F))
    L = O.make_level(rng, [300, 300], F=F, nfeat=F, B=B, mode=2, S=2, Xb=Xb, wide=bool(wide_rows), perm=False,
                     n_models=1)
    r = rng.choice(ids, 600)
    r[:3] = [N - 1, ids[0], N - 1]
    L["rows"] = r.astype(np.uint32) if wide_rows else O.pack(r, rng.choice([1, 255], 600))
    items = _items([(0, 0, 4, X_ONE, 0, 300), (1, 0, 4, X_ONE | X_WIDE, 300, 300)])
    got = _build(L, items, Xb_dev=_d(Xb))
    want = _expect(L, items)
    np.testing.assert_array_equal(got, want)
    assert (want[int(L["node_hist_off"][0]):][:L["per_node"]].reshape(F, B, 2)[:, 0] == 0).all()   # no row read bin 0


# ------------------------------------------------------------------------------------ device count and guards
@pytest.mark.gpu
def test_hist_device_count():
    """dcount (device-planned levels): the grid is the host's bound, items past *dcount leave their sentinels."""
    rng = np.random.default_rng(5)
    L = O.make_level(rng, [100, 257, 64, 300, 65], F=9, nfeat=9, B=5, mode=2, S=2)
    items = _std_items(L, 0, 9, single=range(5), multi=[])
    got = _build(L, items, dcount=3)
    want = _expect(L, items, dcount=3)
    np.testing.assert_array_equal(got, want)
    assert (got[int(L["node_hist_off"][3]):] == SENT).all()
    np.testing.assert_array_equal(_build(L, items, dcount=0), np.full(L["hist_words"], SENT, np.int64))


@pytest.mark.gpu
def test_hist_launcher_guards():
    """Each guard returns -2 and launches nothing: the sentinel buffer is unchanged."""
    rng = np.random.default_rng(6)
    L = O.make_level(rng, [100], F=8, nfeat=8, B=4, mode=2, S=2, perm=False)
    L["Xb"][:, 4:] = np.where(rng.random((L["N"], 4)) < 0.5, 0, 3)
    items = _std_items(L, 0, 4, single=[0], multi=[])
    from transmogrifai_amd.models import tree_engine as TE
    ptr, col, _ = TE.onebin_csr(_d(L["Xb"]), np.array([3] * 4 + [1] * 4))
    sent = np.full(L["hist_words"], SENT, np.int64)
    gh = np.ones((100, 2), np.int32)
    L0 = dict(L, mode=0, S=257)
    L1 = dict(L, mode=1, S=3)
    cases = [("skip_bin >= B", L, dict(skip_bin=4)),
             ("CSR with skip_bin = 0", L, dict(skip_bin=0, csr=(ptr, col))),
             ("CSR with skip_bin = -1", L, dict(skip_bin=-1, csr=(ptr, col))),
             ("gh with mode 1", L1, dict(gh=gh)),
             ("gh with mode 0", dict(L, mode=0), dict(gh=gh)),
             ("mode 0 with S > 256", L0, dict(Sc=1)),
             ("csr_ptr alone", L, dict(skip_bin=3, csr=(ptr, None))),
             ("csr_col alone", L, dict(skip_bin=3, csr=(None, col)))]
    for name, lv, kw in cases:
        np.testing.assert_array_equal(_build(lv, items, rc_want=-2, **kw), sent, err_msg=name)
    np.testing.assert_array_equal(_build(L, items, skip_bin=3), _expect(L, items))     # the same call, valid


# ------------------------------------------------------------------------------------------ subtract and zero
_SEG_NF = [45000, 1, 7, 50, 43, 11, 3]            # whole columns per node; 45000 * 6 words > 1024 * 256: grid-stride
_PER, _S = 6, 2                                   # B = 3


def _segments(n):
    size = np.array(_SEG_NF[:n], np.int64) * _PER            # 270000, 6, 42, 300, 258, 66, 18: no multiple of 256
    off = np.concatenate([[3], 3 + np.cumsum(size + 7)[:-1]]).astype(np.int64)
    return off, size, int(off[-1] + size[-1] + 5)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("dense", [-1, 0, 12, 10 ** 7])
def test_hist_subtract(dense, n):
    """out = parent - small on the live region only, exact beyond +-2^40; every other word keeps its sentinel.
    dense = 12 exceeds the 6-word node (all of it live) and cuts the others partway."""
    lib = _lib()
    rng = np.random.default_rng(n + max(dense, 0) % 97)
    off, size, words = _segments(n)
    parent = rng.integers(-(1 << 45), 1 << 45, words)
    small_v = rng.integers(-(1 << 45), 1 << 45, words)
    out_off = off + words                                     # small children first, the siblings after them
    hist = np.full(2 * words, SENT, np.int64)
    hist[:words] = small_v
    want = hist.copy()
    for j in range(n):
        w = O.live_region(int(size[j]), dense, _PER, _S)
        want[out_off[j] + w] = parent[off[j] + w] - small_v[off[j] + w]
    h, dp, doff, dout, dsize = _d(hist), _d(parent), _d(off), _d(out_off), _d(size)
    rc = lib.tmog_hip_hist_subtract(_p(h), _p(dp), _p(doff), _p(doff), _p(dout), _p(dsize), n, int(size.max()), dense,
                                    _PER, _S, _st())
    torch.cuda.synchronize()
    assert rc == 0
    got = h.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert np.abs(got[got != SENT]).max() > 1 << 40
    n_live = sum(O.live_region(int(s), dense, _PER, _S).size for s in size)
    assert (got[words:] != SENT).sum() == n_live


@pytest.mark.gpu
@pytest.mark.parametrize("device_counts", [0, 1], ids=["host_n", "dn"])
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("dense", [-1, 0, 12, 10 ** 7])
def test_zero_segments(dense, n, device_counts):
    """The first n_dense segments are whole nodes (dense prefix), the rest start at a one-present-bin region (dense
    prefix 0); with ``dn`` both counts come from the device and the host's are only the grid bound."""
    off, size, words = _segments(n)
    n_dense = 3 if n == 7 else 1
    z = dict(off=off, size=size, dense=dense, n_dense=n_dense)
    if device_counts:
        z.update(dn=(5, 2) if n == 7 else (1, 0), n_host=n, n_dense_host=n)
    h = _d(np.full(words, SENT, np.int64))
    _zero(_lib(), h, z, 3, _S)
    want = np.full(words, SENT, np.int64)
    _zero_expect(want, z, 3, _S)
    got = h.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert (got == 0).sum() > 0 and (got[:3] == SENT).all()


# ------------------------------------------------------------------------------------------------- partition
PART_SIZES = [1, 255, 256, 257, 1024, 1025, 4099]


def _part_case(rng, B, missing_bin, dl, wide):
    """Nodes of every size as one item and as three; then all-left, all-right, split_bin 0 and B - 1, and three
    nodes that do not split (feat < 0, params[7] = 0, gain <= eps)."""
    counts = [c for c in PART_SIZES for _ in (0, 1)] + [300, 300, 257, 257, 200, 200, 200]
    n = len(counts)
    F = 6
    L = O.make_level(rng, counts, F=F, nfeat=F, B=B, mode=2, S=2, wide=wide, weights=(0, 1, 7, 255))
    L["Xb"][:, 5] = 3
    feat = rng.integers(0, 5, n).astype(np.int32)
    sbin = rng.integers(0, B - 1, n).astype(np.int32)
    k = 2 * len(PART_SIZES)
    feat[k], sbin[k] = 5, 3                                   # all left
    feat[k + 1], sbin[k + 1] = 5, 2                           # all right
    sbin[k + 2], sbin[k + 3] = 0, B - 1
    params = np.zeros((n, 8), np.float32)
    params[:, 6], params[:, 7] = 0.25, 1.0
    gain = np.full(n, 0.5, np.float32)
    feat[k + 4] = -1
    params[k + 5, 7] = 0.0
    gain[k + 6] = 0.25                                        # == eps: not above it
    items = []
    for j, c in enumerate(counts):
        b = int(L["node_begin"][j])
        three = j < k and j % 2 == 1 and c >= 3
        cuts = [0, c // 3, 2 * c // 3 + 1, c] if three else [0, c]
        items += [(j, 0, b + lo, hi - lo, 0, 0) for lo, hi in zip(cuts[:-1], cuts[1:])]
    return L, feat, sbin, np.full(n, dl, np.uint8), params, gain, np.array(items, O.PART_ITEM), k


def _partition(L, feat, sbin, dlv, params, gain, items, missing_bin, *, xbt=False, gh=None, dcount=None, rc_want=0,
               gh_out=True):
    lib = _lib()
    n, total = len(feat), L["rows"].size
    xb = _d(L["Xb"])
    xt = _d(np.ascontiguousarray(L["Xb"].T)) if xbt else None
    if xbt:
        xb = _d(np.zeros((1, 1), np.uint8))                   # the transposed path must not read Xb
    rows_in = _d(L["rows"])
    rows_out = _d(np.full(total, SENT32, np.uint32))
    cursors = torch.zeros(2 * n, dtype=torch.int64, device="cuda")       # reset by the split reduction in production
    ghi = _d(None if gh is None else np.asarray(gh, np.int32))
    gho = _d(np.full((total, 2), SENT32, np.uint32)) if (gh is not None and gh_out) else None
    keep = [_d(a) for a in (items, L["node_begin"], L["node_count"], feat, sbin, dlv, params, gain)]
    dc = _d(None if dcount is None else np.array([dcount], np.int32))
    rc = lib.tmog_hip_partition_fused(_p(xb), L["F"], _p(rows_in), _p(rows_out), _p(keep[0]), len(items), _p(keep[1]),
                                      _p(keep[2]), _p(keep[3]), _p(keep[4]), _p(keep[5]), _p(keep[6]), _p(keep[7]),
                                      missing_bin, _p(cursors), _p(xt), L["N"], _st(), _p(ghi), _p(gho), _p(dc),
                                      L["wide"])
    torch.cuda.synchronize()
    assert rc == rc_want
    return (rows_out.cpu().numpy().view(np.uint32), cursors.cpu().numpy(),
            None if gho is None else gho.cpu().numpy().view(np.int32))


def _check_partition(L, feat, sbin, dlv, params, gain, missing_bin, got, gh=None, live_nodes=None):
    rows_out, cursors, gh_out = got
    untouched = np.ones(rows_out.size, bool)
    n_split = 0
    for j in range(len(feat)):
        b, c = int(L["node_begin"][j]), int(L["node_count"][j])
        live = live_nodes is None or j in live_nodes
        if not (live and O.splits(feat[j], params[j], gain[j])):
            assert (cursors[2 * j], cursors[2 * j + 1]) == (0, 0), j
            continue
        n_split += 1
        e = L["rows"][b:b + c]
        row, _ = O.decode(e, L["wide"])
        left, right, nl, nr = O.partition(e, L["Xb"][row, feat[j]], int(sbin[j]), missing_bin, int(dlv[j]),
                                          None if gh is None else gh[b:b + c])
        assert (int(cursors[2 * j]), int(cursors[2 * j + 1])) == (nl, nr), j
        out = rows_out[b:b + c].astype(np.int64)
        if gh is not None:                                     # each pair arrives at its entry's position
            out = np.concatenate([out[:, None], gh_out[b:b + c].astype(np.int64)], axis=1)
        np.testing.assert_array_equal(O.sort_rows(out[:nl]), O.sort_rows(left), err_msg=f"left of node {j}")
        np.testing.assert_array_equal(O.sort_rows(out[nl:]), O.sort_rows(right), err_msg=f"right of node {j}")
        untouched[b:b + c] = False
    assert (rows_out[untouched] == SENT32).all()
    if gh is not None:
        assert (gh_out.view(np.uint32)[untouched] == SENT32).all()
    return n_split


@pytest.mark.gpu
@pytest.mark.parametrize("with_gh", [0, 1], ids=["rows", "rows+gh"])
@pytest.mark.parametrize("wide", [0, 1], ids=["packed", "wide_rows"])
@pytest.mark.parametrize("xbt", [0, 1], ids=["Xb", "XbT"])
@pytest.mark.parametrize("missing_bin,dl", [(-1, 0), (7, 0), (7, 1)])
def test_partition_fused(missing_bin, dl, xbt, wide, with_gh):
    """Left entries fill [nb, nb + nl) and right entries [nb + nl, nend) as multisets (the order inside a child is
    not stable), packed entries keep their weight byte, staged pairs move with their entries, the cursors end at
    (nl, nr), nodes that do not split leave rows_out and their cursors alone."""
    B = 8
    rng = np.random.default_rng(8 * max(missing_bin, 0) + 4 * dl + 2 * xbt + wide)
    L, feat, sbin, dlv, params, gain, items, k = _part_case(rng, B, missing_bin, dl, bool(wide))
    gh = rng.integers(-(1 << 31), 1 << 31, (L["rows"].size, 2)).astype(np.int32) if with_gh else None
    got = _partition(L, feat, sbin, dlv, params, gain, items, missing_bin, xbt=bool(xbt), gh=gh)
    n_split = _check_partition(L, feat, sbin, dlv, params, gain, missing_bin, got, gh)
    assert n_split == len(feat) - 3
    cur = got[1]
    assert (cur[2 * k], cur[2 * k + 1]) == (300, 0) and (cur[2 * k + 2], cur[2 * k + 3]) == (0, 300)


@pytest.mark.gpu
def test_partition_device_count_and_gh_guard():
    """Items past *dcount do nothing (their nodes keep sentinels and zero cursors); one of gh_in / gh_out alone is
    refused with -2 before any launch."""
    rng = np.random.default_rng(9)
    L, feat, sbin, dlv, params, gain, items, k = _part_case(rng, 8, 7, 1, False)
    dcount = int(np.searchsorted(items["node"], 6))            # the items of nodes 0 .. 5
    got = _partition(L, feat, sbin, dlv, params, gain, items, 7, dcount=dcount)
    assert _check_partition(L, feat, sbin, dlv, params, gain, 7, got, live_nodes=set(range(6))) == 6
    gh = np.ones((L["rows"].size, 2), np.int32)
    rows_out, cursors, _ = _partition(L, feat, sbin, dlv, params, gain, items, 7, gh=gh, gh_out=False, rc_want=-2)
    assert (rows_out == SENT32).all() and (cursors == 0).all()


# ---------------------------------------------------------------------------------------------- leaf collect
@pytest.mark.gpu
@pytest.mark.parametrize("alt", [0, 1], ids=["no_alt", "rows_alt"])
def test_leaf_collect(alt):
    """Plain copies with the node id next to each entry: counts 0 / 1 / 256 / 257 / 1000 from both row buffers, gaps
    in the output, items past *dcount; buf = 1 without rows_alt falls back to rows."""
    lib = _lib()
    rng = np.random.default_rng(alt)
    counts = [0, 1, 256, 257, 1000, 257, 1, 300]
    n_in = 3000
    rows = rng.integers(0, 1 << 32, n_in, dtype=np.uint64).astype(np.uint32)
    rows_alt = rng.integers(0, 1 << 32, n_in, dtype=np.uint64).astype(np.uint32)
    items, out = [], 2
    for i, c in enumerate(counts):
        items.append((int(rng.integers(0, n_in - c)), c, out, 1000 + i, i % 2))
        out += c + 3                                           # a gap after every leaf
    items = np.array(items, O.LEAF_ITEM)
    dcount = len(counts) - 1                                   # the last item stays out
    r0, g0 = np.full(out, SENT32, np.uint32), np.full(out, -7, np.int32)
    want_r, want_g = O.leaf_collect(rows, rows_alt if alt else None, items[:dcount], r0.copy(), g0.copy())
    dr, dg = _d(r0), _d(g0)
    keep = [_d(rows), _d(rows_alt) if alt else None, _d(items), _d(np.array([dcount], np.int32))]
    rc = lib.tmog_hip_leaf_collect(_p(keep[0]), _p(keep[2]), len(items), _p(dr), _p(dg), _st(), _p(keep[1]),
                                   _p(keep[3]))
    torch.cuda.synchronize()
    assert rc == 0
    np.testing.assert_array_equal(dr.cpu().numpy().view(np.uint32), want_r)
    np.testing.assert_array_equal(dg.cpu().numpy(), want_g)
    assert (want_g == -7).sum() == out - sum(counts[:dcount])
    # without the device count every item is copied
    want_r, want_g = O.leaf_collect(rows, rows_alt if alt else None, items, r0.copy(), g0.copy())
    dr, dg = _d(r0), _d(g0)
    rc = lib.tmog_hip_leaf_collect(_p(keep[0]), _p(keep[2]), len(items), _p(dr), _p(dg), _st(), _p(keep[1]), None)
    torch.cuda.synchronize()
    assert rc == 0
    np.testing.assert_array_equal(dr.cpu().numpy().view(np.uint32), want_r)
    np.testing.assert_array_equal(dg.cpu().numpy(), want_g)


# ---------------------------------------------------------------------------------------------- a whole level
@pytest.mark.gpu
def test_chained_level():
    """zero -> build the small child -> subtract to the sibling -> partition, then a second build from the children's
    row sets: its histograms equal the oracle's of those sets, the subtraction's sibling equals the direct build, and
    each pair sums to the parent."""
    lib = _lib()
    rng = np.random.default_rng(11)
    B, F = 8, 6
    counts = [3000, 2500]
    L = O.make_level(rng, counts, F=F, nfeat=F, B=B, mode=2, S=2)
    n = len(counts)
    per = L["per_node"]
    parents = _std_items(L, 0, F, single=range(n), multi=[])
    P = _build(L, parents)
    np.testing.assert_array_equal(P, _expect(L, parents))
    feat = np.array([L["feat_list"][L["node_feat_off"][0] + 1], L["feat_list"][L["node_feat_off"][1] + 4]], np.int32)
    sbin = np.array([1, 5], np.int32)
    params = np.zeros((n, 8), np.float32)
    params[:, 7] = 1.0
    gain = np.ones(n, np.float32)
    pit = np.array([(j, 0, int(L["node_begin"][j]) + o, min(1024, counts[j] - o), 0, 0)
                    for j in range(n) for o in range(0, counts[j], 1024)], O.PART_ITEM)
    rows_out, cursors, _ = _partition(L, feat, sbin, np.zeros(n, np.uint8), params, gain, pit, -1)
    _check_partition(L, feat, sbin, np.zeros(n, np.uint8), params, gain, -1, (rows_out, cursors, None))
    # children: node 2j = left of j, 2j + 1 = right of j, rows taken from the partition's output
    nl = cursors[0::2].astype(np.int64)
    cb = np.stack([L["node_begin"], L["node_begin"] + nl], 1).ravel()
    cc = np.stack([nl, np.asarray(counts) - nl], 1).ravel()
    assert (cc > 0).all()
    L2 = dict(L, rows=rows_out, node_begin=cb, node_count=cc, node_model=np.repeat(L["node_model"], 2),
              node_feat_off=np.repeat(L["node_feat_off"], 2), node_nfeat=np.repeat(L["node_nfeat"], 2),
              node_hist_off=np.arange(2 * n, dtype=np.int64) * (per + 5) + 2, hist_words=2 * n * (per + 5) + 2)
    small = [2 * j + int(cc[2 * j] > cc[2 * j + 1]) for j in range(n)]
    big = [4 * j + 1 - s for j, s in enumerate(small)]
    # small children in two chunks each: zeroed, then accumulated atomically
    sit = _items([(s, 0, F, 0, b, c) for s in small
                  for b, c in _chunks(int(cb[s]), int(cc[s]), (int(cc[s]) + 1) // 2)])
    hist = _d(np.full(L2["hist_words"], SENT, np.int64))
    zero = _node_zero(L2, small)
    got_small = _build(L2, sit, zero=zero)
    np.testing.assert_array_equal(got_small, _expect(L2, sit, zero=zero))
    hist.copy_(_d(got_small))
    poff = L["node_hist_off"].astype(np.int64)
    soff, ooff = L2["node_hist_off"][small], L2["node_hist_off"][big]
    keep = [_d(a) for a in (P, poff, soff, ooff, np.full(n, per, np.int64))]
    rc = lib.tmog_hip_hist_subtract(_p(hist), *[_p(t) for t in keep], n, per, -1, B * 2, 2, _st())
    torch.cuda.synchronize()
    assert rc == 0
    level2 = hist.cpu().numpy()
    # the second build: all four children directly from their row sets
    cit = _std_items(L2, 0, F, single=range(2 * n), multi=[])
    direct = _build(L2, cit)
    np.testing.assert_array_equal(direct, _expect(L2, cit))
    np.testing.assert_array_equal(level2, direct)
    for j in range(n):
        a, b = (direct[int(L2["node_hist_off"][2 * j + s]):][:per] for s in (0, 1))
        np.testing.assert_array_equal(a + b, P[int(poff[j]):][:per])
