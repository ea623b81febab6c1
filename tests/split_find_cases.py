"""Crafted split-find levels and a NumPy oracle of the impurity gains, shared by tests/test_split_find_cpu_oracle.py
and tests/test_split_find_twins_gpu.py (a helper module, not a test file).

The histograms are built the way tests/test_scan_newton_gpu.py builds them: synthetic rows are binned per feature, so
every feature of a node sums to the node's totals. Scales are powers of two, so ``(double)lq * q`` is exact.

The oracle follows the rules documented for ``tmog_split_find_cpu``: Gini ``1 - sum p^2`` and variance
``E[t^2] - E[t]^2`` of the scaled statistics, gain = parent impurity minus the children's count-weighted impurities; a
candidate needs both children at ``min_instances`` (and non-empty) and a gain of at least ``min_info_gain``; with a
missing bin the missing rows go right (dl = 0) or left (dl = 1), dl = 0 also tries "every present value left", and
dl = 1 is tried only when the feature's missing bin holds something. The first maximum in (feature, dl, bin) order
wins. Sums over the statistics run in index order (sequential float64 adds, not NumPy's pairwise sum)."""
import numpy as np

N_NODES = 5
NO_SCAN = 1            # node with params slot 7 (may split) = 0
TINY = 2               # node with 3 rows
QINV = {
    0: lambda S: np.array([[2.0 ** -4] * S, [2.0 ** -6] * S]),       # real-valued class weights (k / 16, k / 64)
    1: lambda S: np.array([[2.0 ** -4] * S, [2.0 ** -6] * S]),
    2: lambda S: np.array([[1.0, 2.0 ** -20, 2.0 ** -18], [1.0, 2.0 ** -16, 2.0 ** -22]]),
    3: lambda S: np.array([[2.0 ** -30, 2.0 ** -28], [2.0 ** -24, 2.0 ** -26]]),
}


def _seq_sum(x):
    n = np.zeros(x.shape[:-1])
    for s in range(x.shape[-1]):
        n = n + x[..., s]
    return n


def _impurity(st, kind):
    """(impurity, count) of scaled statistics st[..., S]; kinds 0 (Gini), 1 (entropy), 2 (variance)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == 2:
            n = st[..., 0]
            m = st[..., 1] / n
            imp = st[..., 2] / n - m * m
        else:
            n = _seq_sum(st)
            imp = np.ones(n.shape) if kind == 0 else np.zeros(n.shape)
            for s in range(st.shape[-1]):
                p = st[..., s] / n
                imp = imp - (p * p if kind == 0 else np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0))
    return np.where(n > 0, imp, 0.0), n


def impurity_gains(H, nb, q, prm, mb, kind):
    """Gains [nf][dl][bin] of one node (-inf: no candidate, before the min_info_gain rule), the int64 left sums
    [nf][dl][bin][S] and the node totals."""
    nf, B, S = H.shape
    totq = H[0].sum(axis=0)
    tot = totq.astype(np.float64) * q
    allow = bool(prm[5] > 0.5) and mb >= 0
    min_inst = np.float64(prm[0])
    pimp, tcount = _impurity(tot, kind)
    cs = np.cumsum(H, axis=1)
    miss = H[:, mb, :] if allow else np.zeros((nf, S), np.int64)
    any_miss = (miss != 0).any(axis=1)
    b = np.arange(B)[None, :]
    gains = np.full((nf, 2, B), -np.inf)
    lqs = np.zeros((nf, 2, B, S), np.int64)
    for dl in (0, 1):
        lq = cs + (miss[:, None, :] if dl else 0)
        li, lc = _impurity(lq.astype(np.float64) * q, kind)
        ri, rc = _impurity((totq - lq).astype(np.float64) * q, kind)
        ok = b < (nb[:, None] - 1 + (1 if (allow and dl == 0) else 0))
        if dl:
            ok = ok & (allow & any_miss)[:, None]
        ok = ok & ~((lc < min_inst) | (rc < min_inst) | (lc <= 0) | (rc <= 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            gain = pimp - (lc / tcount) * li - (rc / tcount) * ri
        gains[:, dl, :] = np.where(ok, gain, -np.inf)
        lqs[:, dl] = lq
    return gains, lqs, tot


def oracle_node(H, nb, q, prm, mb, kind):
    """(local feature, bin, dl, gain f32, left f32[S], total f32[S]) of one node; feature -1: no split. The
    may-split slot is not read (the CPU twin scans every node; its caller applies the slot)."""
    if kind == 3:
        from test_scan_newton_gpu import _oracle_node
        return _oracle_node(H, nb, q, np.concatenate([prm[:7], [1.0]]).astype(np.float32), mb)
    gains, lqs, tot = impurity_gains(H, nb, q, prm, mb, kind)
    gains = np.where(gains < np.float64(prm[1]), -np.inf, gains)
    f, dl, bb = np.unravel_index(int(np.argmax(gains)), gains.shape)      # first maximum in (feature, dl, bin) order
    if gains[f, dl, bb] == -np.inf:
        return -1, -1, 0, np.float32(-np.inf), np.zeros(H.shape[2], np.float32), tot.astype(np.float32)
    return (int(f), int(bb), int(dl), np.float32(gains[f, dl, bb]),
            (lqs[f, dl, bb].astype(np.float64) * q).astype(np.float32), tot.astype(np.float32))


def make_case(kind, S, B, n_multi, n_one, seed):
    """Five nodes over two models on one feature list: local features [0, n_multi) have several bins, [n_multi, nf)
    one present bin; the missing bin is B - 1 and stays empty on the even multi-bin features (every one-present-bin
    feature has rows in it: its only candidate is present-left / missing-right). Node NO_SCAN has the may-split slot
    0, node TINY has 3 rows, node 3 does not allow missing. min_instances is 1 or a third of the node's count,
    min_info_gain 0 or the 60th percentile of the node's gains (above the median). Columns ``dup`` are duplicates,
    in different feature blocks of the narrow scan (16 features each) where n_multi allows."""
    rng = np.random.default_rng(seed)
    mb = B - 1
    nf = n_multi + n_one
    F = nf + 3
    feat_list = rng.permutation(F)[:nf].astype(np.int32)
    nb = np.ones(nf, np.int64)
    nb[:n_multi] = rng.integers(2, B, n_multi)
    dup = (1, 16) if n_multi >= 17 else ((0, 2) if n_multi >= 3 else None)
    if dup:
        nb[dup[1]] = nb[dup[0]]
    strong = dup[0] if dup else 0
    feat_nbins = rng.integers(1, B, F).astype(np.int32)
    feat_nbins[feat_list] = nb
    p_miss = np.where(np.arange(nf) % 2 == 0, 0.0, 0.3)
    p_miss[n_multi:] = 0.5
    qinv = QINV[kind](S)
    hists = np.zeros((N_NODES, nf, B, S), np.int64)
    params = np.zeros((N_NODES, 8), np.float32)
    model = (np.arange(N_NODES) % 2).astype(np.int32)
    for j in range(N_NODES):
        r = 3 if j == TINY else int(rng.integers(20, 60))
        st = np.zeros((r, S), np.int64)
        if kind in (0, 1):
            y = rng.integers(0, S, r)
            st[np.arange(r), y] = rng.integers(1, 64, r)
            signal = y / S
        elif kind == 2:
            w, t = rng.integers(1, 4, r), rng.normal(size=r)
            st[:, 0] = w
            st[:, 1] = np.rint(w * t / qinv[model[j], 1])
            st[:, 2] = np.rint(w * t * t / qinv[model[j], 2])
            signal = (np.argsort(np.argsort(t)) + 0.5) / r
        else:
            big = j % 3 != 1
            st[:, 0] = rng.integers(-(1 << 40), 1 << 40, r) if big else rng.integers(-1000, 1000, r)
            st[:, 1] = rng.integers(1, 1 << 38, r) if big else rng.integers(1, 1 << 20, r)
            signal = np.where(st[:, 0] > 0, 0.25, 0.75)
        bins = (rng.random((r, nf)) * nb).astype(np.int64)
        bins[rng.random((r, nf)) < p_miss] = mb
        if nb[strong] >= 2:                                     # a column that follows the target
            bins[:, strong] = np.minimum((signal * nb[strong]).astype(np.int64), nb[strong] - 1)
            if j % 2 == 0 and strong % 2 == 1:
                bins[rng.random(r) < 0.25, strong] = mb
        if dup:
            bins[:, dup[1]] = bins[:, dup[0]]
        fi = np.broadcast_to(np.arange(nf), (r, nf))
        for s in range(S):
            np.add.at(hists[j, :, :, s], (fi, bins), st[:, s][:, None])
        tot = st.sum(axis=0).astype(np.float64) * qinv[model[j]]
        count = tot[1] if kind == 3 else (tot[0] if kind == 2 else tot.sum())
        mcw = [1.0, 0.3 * tot[1], 1e30, 0.0, 0.05 * tot[1]][j] if kind == 3 else 0.0
        params[j] = [1.0 if j % 2 == 0 else count / 3.0, 0.0, mcw, 1.0, 0.0, 0.0 if j == 3 else 1.0, 0.0,
                     0.0 if j == NO_SCAN else 1.0]
        if kind != 3 and j >= 3:
            g = impurity_gains(hists[j], nb, qinv[model[j]], params[j], mb, kind)[0]
            g = g[np.isfinite(g)]
            if g.size:
                params[j, 1] = np.quantile(g, 0.6)
    per = nf * B * S
    node_off = np.arange(N_NODES, dtype=np.int64) * (per + 6)    # a gap between the nodes' histograms
    buf = np.full(N_NODES * (per + 6), np.int64(0x5A5A5A5A5A5A5A5A), np.int64)
    for j in range(N_NODES):
        buf[node_off[j]:node_off[j] + per] = hists[j].ravel()
    return dict(kind=kind, S=S, B=B, mb=mb, nf=nf, n_multi=n_multi, n_nodes=N_NODES, feat_list=feat_list,
                feat_nbins=feat_nbins, nb=nb, qinv=qinv, hists=hists, params=params, model=model, node_off=node_off,
                buf=buf, dup=dup)


def fp_rec_bytes(S):
    return (24 + 4 * S + 7) & ~7


def run_cpu(host, c, rec=None, fp=(0, 0, 0), pad=2):
    """``tmog_split_find_cpu`` on a case; outputs are sentinel-filled and ``pad`` entries longer than the level."""
    import ctypes as C
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    n, S = c["n_nodes"], c["S"]
    o = dict(feat=np.full(n + pad, -7, np.int32), bin=np.full(n + pad, -7, np.int32),
             gain=np.full(n + pad, 7.0, np.float32), dl=np.full(n + pad, 7, np.uint8),
             left=np.full((n + pad, S), 7.0, np.float32), tot=np.full((n + pad, S), 7.0, np.float32))
    buf = c["buf"].copy()
    nnf, nfo = np.full(n, c["nf"], np.int32), np.zeros(n, np.int32)
    rc = host.tmog_split_find_cpu(p(buf), n, p(c["node_off"]), p(nnf), p(nfo), p(c["feat_list"]), p(c["feat_nbins"]),
                                  c["B"], S, c["kind"], p(c["params"]), c["mb"], p(c["model"]), p(c["qinv"]),
                                  p(o["feat"]), p(o["bin"]), p(o["gain"]), p(o["dl"]), p(o["left"]), p(o["tot"]),
                                  p(rec), fp_rec_bytes(S) if rec is not None else 0, *fp)
    assert rc == 0
    np.testing.assert_array_equal(buf, c["buf"])
    return o
