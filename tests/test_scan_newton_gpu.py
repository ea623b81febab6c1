"""The Newton instantiation of the narrow split scans (pair_scan_kernel / split_scan_kernel with the gain kind
fixed to 3 at compile time and software-pipelined histogram loads) against the generic instantiation
(``TMOG_SCAN_GENERIC=1``: run-time kind, unpipelined loop) and against a NumPy oracle written here.

Kernel level: ``tmog_hip_pair_scan`` then ``tmog_hip_split_find`` (fused reduction) through ctypes on crafted int64
histograms. The scales are powers of two, as in production, so ``(double)lq * q`` is exact and the oracle's float64
gains are the kernel's bit for bit. Tree level: whole XGBoost forests under both settings of the switch."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

S = 2
SENT = np.int64(0x5A5A5A5A5A5A5A5A)          # words of the histogram buffer no kernel may write
P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
_PAIR_SIG = [P, P, P, P, P, I32, P, P, P, P, P, I32, I32, I32, P, I32, P, P, I32, P, I32, P, P]


def _lib():
    from transmogrifai_amd.ops import _native
    lib = _native.hip()
    lib.tmog_hip_pair_scan.argtypes = _PAIR_SIG
    lib.tmog_hip_pair_scan.restype = C.c_int
    lib.tmog_hip_split_cand_bytes.argtypes = [I32, I32, I32, I32]
    lib.tmog_hip_split_cand_bytes.restype = C.c_size_t
    return lib


def _make_case(B, n_multi, n_one, n_pairs, seed):
    """Two unpaired nodes (split_scan) and ``n_pairs`` sibling pairs (pair_scan) over one feature list: local
    features [0, n_multi) have several bins, [n_multi, nf) one present bin. Histograms come from synthetic rows, so
    every feature of a node sums to the node's totals. Only the first ``dnp`` pairs and ``dm`` nodes are live."""
    rng = np.random.default_rng(seed)
    mb = B - 1                                        # the missing bin: past every feature's present bins
    nf = n_multi + n_one
    n_un = 2
    n_nodes = n_un + 2 * n_pairs
    dnp = n_pairs if n_pairs < 3 else n_pairs - max(1, n_pairs // 7)    # device pair count below the grid bound
    dm = n_un + 2 * dnp
    F = nf + 5
    feat_list = rng.permutation(F)[:nf].astype(np.int32)
    nb = np.ones(nf, np.int64)
    nb[:n_multi] = rng.integers(2, B, n_multi)                          # 2 .. B - 1 present bins
    if n_multi >= 5:
        nb[0], nb[1], nb[3] = B - 1, 2, 1                               # widest, narrowest, one bin inside the scan
    dups = [(2, 17)] if n_multi >= 18 else []                           # duplicate columns in different blocks
    if n_multi >= 37:
        dups.append((2, 35))
    for a, b in dups:
        nb[b] = nb[a]
    feat_nbins = rng.integers(1, B, F).astype(np.int32)
    feat_nbins[feat_list] = nb
    p_miss = np.where(np.arange(nf) % 2 == 0, 0.0, 0.3)                 # even features: empty missing bin
    p_miss[n_multi:] = 0.5                                              # one present bin: present or missing
    qinv = np.array([[2.0 ** -30, 2.0 ** -28], [2.0 ** -24, 2.0 ** -26]])

    hists = np.zeros((n_nodes, nf, B, S), np.int64)
    params = np.zeros((n_nodes, 8), np.float32)
    model = np.zeros(n_nodes, np.int32)
    for j in range(n_nodes):
        q = (j - n_un) // 2 if j >= n_un else j
        k = q + seed                                                     # the node cases cycle over pairs and seeds
        model[j] = q % 2
        r = 3 if k % 5 == 4 else int(rng.integers(20, 60))
        big = k % 3 != 1                                                 # |g| sums above 2^40, or small magnitudes
        g = rng.integers(-(1 << 40), 1 << 40, r) if big else rng.integers(-1000, 1000, r)
        h = rng.integers(1, 1 << 38, r) if big else rng.integers(1, 1 << 20, r)
        bins = (rng.random((r, nf)) * nb).astype(np.int64)              # uniform over each feature's bins
        bins[rng.random((r, nf)) < p_miss] = mb
        if n_multi >= 3 and nb[2] >= 2:                                  # a strong column (the duplicated one)
            half = max(1, nb[2] // 2)
            bins[:, 2] = np.where(g > 0, rng.integers(0, half, r), rng.integers(half, nb[2], r))
            if k % 2 == 0:                                               # ... with rows in its missing bin
                bins[rng.random(r) < 0.25, 2] = mb
        for a, b in dups:
            bins[:, b] = bins[:, a]
        fi = np.broadcast_to(np.arange(nf), (r, nf))
        np.add.at(hists[j, :, :, 0], (fi, bins), g[:, None])
        np.add.at(hists[j, :, :, 1], (fi, bins), h[:, None])
        tot_h = float(h.sum()) * qinv[model[j], 1]
        mcw = [1.0, 0.3 * tot_h, 1e30, 0.0][k % 4] if j % 2 == 0 else [0.05 * tot_h, 1.0][k % 2]
        params[j] = [1.0, 0.0, mcw, 1.0, 1.0 if j >= n_un else 0.0, 0.0 if k % 6 == 3 else 1.0, 0.0,
                     0.0 if (j >= n_un and (j + k) % 7 == 5) else 1.0]   # slot 7 = 0: built but not scanned
    # node order inside a pair alternates, so small_j / big_j are not monotone
    small = np.array([n_un + 2 * q + (q % 2) for q in range(n_pairs)], np.int32)
    bigj = np.array([n_un + 2 * q + 1 - (q % 2) for q in range(n_pairs)], np.int32)
    per = nf * B * S
    node_off = (np.arange(n_nodes, dtype=np.int64) * (per + 6))          # a gap between the nodes' histograms
    buf = np.full(n_nodes * (per + 6), SENT, np.int64)
    want_buf = buf.copy()
    parent = np.zeros((n_pairs, nf, B, S), np.int64)
    for j in range(n_un):
        buf[node_off[j]:node_off[j] + per] = hists[j].ravel()
    for q in range(n_pairs):
        parent[q] = hists[small[q]] + hists[bigj[q]]
        buf[node_off[small[q]]:node_off[small[q]] + per] = hists[small[q]].ravel()
    want_buf[:] = buf
    for q in range(dnp):                 # big = parent - small: every bin of a multi-bin column, bin 0 of the others
        w = np.full((nf, B, S), SENT, np.int64)
        w[:n_multi] = hists[bigj[q], :n_multi]
        w[n_multi:, 0] = hists[bigj[q], n_multi:, 0]
        want_buf[node_off[bigj[q]]:node_off[bigj[q]] + per] = w.ravel()
    return dict(B=B, mb=mb, nf=nf, n_multi=n_multi, n_nodes=n_nodes, n_pairs=n_pairs, dnp=dnp, dm=dm,
                feat_list=feat_list, feat_nbins=feat_nbins, nb=nb, qinv=qinv, hists=hists, params=params,
                model=model, small=small, bigj=bigj, node_off=node_off, buf=buf, want_buf=want_buf,
                parent=parent.ravel(), parent_off=np.arange(n_pairs, dtype=np.int64) * per)


def _oracle_node(H, nb, q, prm, mb):
    """Best Newton split of one node: int64 prefix sums, float64 gains in the kernel's operation order, the
    min_child_weight rule, dl = 1 candidates only with a non-empty missing bin on a node that allows missing,
    ties by gain descending, then feature, dl and bin ascending."""
    nf, B, _ = H.shape
    totq = H[0].sum(axis=0)
    tot = totq.astype(np.float64) * q
    none = (-1, -1, 0, np.float32(-np.inf), np.zeros(S, np.float32), tot.astype(np.float32))
    if prm[7] <= 0.5:
        return none
    allow = bool(prm[5] > 0.5) and mb >= 0
    mcw, lam = np.float64(prm[2]), np.float64(prm[3])
    pg = tot[0] * tot[0] / (tot[1] + lam)
    cs = np.cumsum(H, axis=1)
    miss = H[:, mb, :] if allow else np.zeros((nf, S), np.int64)
    any_miss = (miss != 0).any(axis=1)
    b = np.arange(B)[None, :]
    gains = np.full((nf, 2, B), -np.inf)
    for dl in (0, 1):
        lq = cs + (miss[:, None, :] if dl else 0)
        left = lq.astype(np.float64) * q
        right = (totq - lq).astype(np.float64) * q
        ok = b < (nb[:, None] - 1 + (1 if (allow and dl == 0) else 0))
        if dl:
            ok = ok & (allow & any_miss)[:, None]
        ok = ok & ~((left[..., 1] < mcw) | (right[..., 1] < mcw))
        gain = left[..., 0] * left[..., 0] / (left[..., 1] + lam) + \
            right[..., 0] * right[..., 0] / (right[..., 1] + lam) - pg
        gains[:, dl, :] = np.where(ok, gain, -np.inf)
    i = int(np.argmax(gains))                 # first maximum in (feature, dl, bin) order
    f, dl, bb = np.unravel_index(i, gains.shape)
    if gains[f, dl, bb] == -np.inf:
        return none
    lq = cs[f, bb] + (miss[f] if dl else 0)
    return (int(f), int(bb), int(dl), np.float32(gains[f, dl, bb]), (lq.astype(np.float64) * q).astype(np.float32),
            tot.astype(np.float32))


def _run(lib, c, monkeypatch, generic):
    from transmogrifai_amd.ops import _native
    monkeypatch.setenv("TMOG_SCAN_GENERIC", "1" if generic else "0")
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    n = c["n_nodes"]
    hist, parent = t(c["buf"]), t(c["parent"])
    poff, sj, bj = t(c["parent_off"]), t(c["small"]), t(c["bigj"])
    nho = t(c["node_off"])
    nnf = t(np.full(n, c["nf"], np.int32))
    nfo = t(np.zeros(n, np.int32))
    fl, fnb = t(c["feat_list"]), t(c["feat_nbins"])
    prm, mdl, qinv = t(c["params"]), t(c["model"]), t(c["qinv"])
    cand = torch.zeros(lib.tmog_hip_split_cand_bytes(n, c["nf"], c["B"], S), dtype=torch.uint8, device=dev)
    done = torch.zeros(n, dtype=torch.int32, device=dev)
    dnp = t(np.array([c["dnp"]], np.int32))
    dm = t(np.array([c["dm"]], np.int32))
    o_feat = torch.full((n,), -7, dtype=torch.int32, device=dev)
    o_bin = torch.full((n,), -7, dtype=torch.int32, device=dev)
    o_gain = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    o_dl = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    o_left = torch.full((n, S), 7.0, dtype=torch.float32, device=dev)
    o_tot = torch.full((n, S), 7.0, dtype=torch.float32, device=dev)
    st = _native.stream()
    p = _native.ptr
    rc = lib.tmog_hip_pair_scan(p(hist), p(parent), p(poff), p(sj), p(bj), c["n_pairs"], p(nho), p(nnf), p(nfo), p(fl),
                                p(fnb), c["B"], S, 3, p(prm), c["mb"], p(mdl), p(qinv), c["nf"], p(cand), c["n_multi"],
                                st, p(dnp))
    assert rc == 0
    rc = lib.tmog_hip_split_find(p(hist), n, p(nho), p(nnf), p(nfo), p(fl), p(fnb), c["B"], S, 3, p(prm), c["mb"],
                                 p(mdl), p(qinv), c["nf"], p(cand), p(o_feat), p(o_bin), p(o_gain), p(o_dl), p(o_left),
                                 p(o_tot), None, c["n_multi"], None, 0, 0, 0, 0, st, p(done), p(dm))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(done.abs().sum()) == 0                                    # the ticket counters are left zeroed
    return dict(hist=hist.cpu().numpy(), feat=o_feat.cpu().numpy(), bin=o_bin.cpu().numpy(),
                gain=o_gain.cpu().numpy(), dl=o_dl.cpu().numpy(), left=o_left.cpu().numpy(), tot=o_tot.cpu().numpy())


_SHAPES = list(itertools.product([64, 33], [1, 5, 18, 37], [0, 3, 300], [1, 3, 70]))


@pytest.mark.gpu
@pytest.mark.parametrize("B,n_multi,n_one,n_pairs", _SHAPES)
def test_newton_scan_matches_generic_and_oracle(monkeypatch, B, n_multi, n_one, n_pairs):
    lib = _lib()
    c = _make_case(B, n_multi, n_one, n_pairs, seed=_SHAPES.index((B, n_multi, n_one, n_pairs)))
    new = _run(lib, c, monkeypatch, generic=False)
    ref = _run(lib, c, monkeypatch, generic=True)
    # (i) the generic instantiation: every histogram word and every output, bit for bit
    for k in new:
        a, b = new[k], ref[k]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=k)
    # the big children's histograms: parent - small where the kernel writes, untouched elsewhere
    np.testing.assert_array_equal(new["hist"], c["want_buf"])
    # (ii) the NumPy oracle, live nodes only
    n_found = 0
    for j in range(c["dm"]):
        f, bb, dl, gain, left, tot = _oracle_node(c["hists"][j], c["nb"], c["qinv"][c["model"][j]], c["params"][j],
                                                  c["mb"])
        got = (int(new["feat"][j]), int(new["bin"][j]), int(new["dl"][j]))
        assert got == (int(c["feat_list"][f]) if f >= 0 else -1, bb, dl), (j, got, f, bb, dl)
        assert new["gain"][j].view(np.uint32) == gain.view(np.uint32), (j, new["gain"][j], gain)
        np.testing.assert_array_equal(new["left"][j].view(np.uint32), left.view(np.uint32), err_msg=f"left {j}")
        np.testing.assert_array_equal(new["tot"][j].view(np.uint32), tot.view(np.uint32), err_msg=f"total {j}")
        n_found += f >= 0
    for k in ("feat", "bin"):                                            # nodes past the device count: untouched
        assert (new[k][c["dm"]:] == -7).all()
    assert n_found > 0 or c["dm"] <= 4


def test_oracle_tie_break_prefers_lowest_feature():
    """The oracle itself: two identical columns tie, the lower local feature wins; dl = 0 wins an empty missing bin."""
    H = np.zeros((3, 8, S), np.int64)
    H[0, :3] = [[4, 2], [-6, 2], [1, 2]]
    H[1] = H[0]
    H[2, 0] = H[0].sum(axis=0)
    prm = np.array([1, 0, 0.5, 1, 0, 1, 0, 1], np.float32)
    f, bb, dl, gain, _, _ = _oracle_node(H, np.array([3, 3, 2]), np.array([1.0, 1.0]), prm, 7)
    assert (f, dl) == (0, 0) and gain > 0


@pytest.mark.gpu
@pytest.mark.parametrize("learner", ["xgb", "xgbdeep"])
def test_forests_identical_under_generic_switch(monkeypatch, learner):
    """The data and jobs of test_pair_scan_identical_to_subtract_then_scan's XGBoost cases: every forest array is the
    same with the Newton and the generic instantiation."""
    from transmogrifai_amd.models.base import FitJob
    from transmogrifai_amd.models.trees import XGBoostClassifierLearner as L
    from transmogrifai_amd.ops import _native
    g = torch.Generator().manual_seed(6)
    n, d = 30_000, 18
    X = torch.randn(n, d, generator=g)
    X[:, :5] = (X[:, :5] > 0.6).float()
    z = X[:, 5] + X[:, 0] - 0.5 * X[:, 7] + 0.5 * torch.randn(n, generator=g)
    y = (z > 0).float()
    Xd, yd = X.cuda(), y.cuda()
    params = dict(L.defaults, num_round=12, max_depth=7, eta=0.3, missing=0.0) if learner == "xgb" else \
        dict(L.defaults, num_round=6, max_depth=10, eta=0.3, missing=0.0, gamma=0.0)
    jobs = [FitJob(dict(params, min_child_weight=m), torch.arange(k, n, 3, device="cuda"))
            for m in ((1.0, 10.0) if learner == "xgb" else (0.05, 0.5)) for k in range(3)]
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("TMOG_SCAN_GENERIC", flag)
        outs.append(L().fit_batch(Xd, yd, jobs))
    n_arrays = 0
    for a, b in zip(*outs):
        assert a["num_trees"] == b["num_trees"]
        for k in a["forest"]:
            va, vb = a["forest"][k], b["forest"][k]
            if isinstance(va, np.ndarray):
                np.testing.assert_array_equal(va, vb, err_msg=k)
                n_arrays += 1
    assert n_arrays > 0
    assert _native.hip_loaded()
