"""NumPy oracle of the per-level tree kernels (histogram build, subtract, zero, partition, leaf collect), written
from the layout contract at the top of ``ops/csrc/hip/tree_hist_kernels.hip`` -- not from the kernel bodies:

  Xb    uint8 [N][F] row-major bins            rows  uint32 entries, ``row | weight << 24`` (``wide``: the row id,
                                                     weight 1)
  hist  int64 fixed point, node j at ``node_hist_off[j]``, word ``((fl * B) + bin) * S + s``

Everything is integer, so every comparison against it is exact. ``tests/test_tree_level_oracle.py`` shows on the
CPU that it agrees bit for bit with the host twins (``tmog_hist_build_cpu`` / ``tmog_partition_cpu``); that is what
entitles it to judge the HIP kernels in ``tests/test_tree_level_kernels_gpu.py``."""
from __future__ import annotations

import numpy as np

SENT = np.int64(0x5A5A5A5A5A5A5A5A)          # int64 words no kernel may write
SENT32 = np.uint32(0x5A5A5A5A)               # the same for 32-bit buffers (entries, node ids, staged statistics)

HIST_ITEM = np.dtype([("node", "<i4"), ("fg0", "<i4"), ("nf", "<i4"), ("excl", "<i4"), ("begin", "<i8"),
                      ("count", "<i8")])
PART_ITEM = np.dtype([("node", "<i4"), ("pad", "<i4"), ("begin", "<i8"), ("count", "<i8"), ("out_left", "<i8"),
                      ("out_right", "<i8")])
LEAF_ITEM = np.dtype([("begin", "<i8"), ("count", "<i8"), ("out", "<i8"), ("gid", "<i4"), ("buf", "<i4")])
assert (HIST_ITEM.itemsize, PART_ITEM.itemsize, LEAF_ITEM.itemsize) == (32, 40, 32)


# ------------------------------------------------------------------------------------------ entry decoding
def decode(entries, wide):
    """``(row, weight)`` of row entries: packed ``row | weight << 24``, or (``wide``) the 32-bit row id, weight 1."""
    e = np.asarray(entries, np.uint32).astype(np.int64)
    if wide:
        return e, np.ones_like(e)
    return e & 0xFFFFFF, e >> 24


def pack(rows, weights):
    return (np.asarray(rows, np.int64) | (np.asarray(weights, np.int64) << 24)).astype(np.uint32)


# --------------------------------------------------------------------------------------------- row staging
def _q(v):
    """``(int)rintf(v)`` of a float32 array."""
    assert v.dtype == np.float32
    return np.rint(v).astype(np.int64)


def stage(mode, entries, wide, S, *, y=None, t1=None, t2=None, qs=None, gh=None):
    """Per-entry integer statistics ``[n, S]``. Every float step is float32, then rint, then the cast.
    mode 0: ``w`` at the entry's class. mode 1: ``(w, q(w t), q(w t t))``. mode 2: ``(q(w g), q(w h))``, or the
    staged pair ``gh[i]`` riding with entry ``i``. ``t1`` / ``t2`` / ``qs`` are the entry's model's."""
    row, wi = decode(entries, wide)
    n = row.size
    out = np.zeros((n, S), np.int64)
    w = wi.astype(np.float32)
    if mode == 0:
        cls = np.asarray(y, np.float32)[row].astype(np.int64)
        out[np.arange(n), cls] = wi
    elif mode == 1:
        qs = np.asarray(qs, np.float32)
        t = np.asarray(t1, np.float32)[row]
        wt = w * t
        out[:, 0] = wi
        out[:, 1] = _q(wt * qs[1])
        out[:, 2] = _q((wt * t) * qs[2])
    elif gh is not None:
        out[:, :] = np.asarray(gh, np.int64).reshape(n, 2)
    else:
        qs = np.asarray(qs, np.float32)
        out[:, 0] = _q((w * np.asarray(t1, np.float32)[row]) * qs[0])
        out[:, 1] = _q((w * np.asarray(t2, np.float32)[row]) * qs[1])
    return out


# ------------------------------------------------------------------------------------------ node histogram
def node_hist(bins, q, B):
    """``[nf, B, S]`` int64 sums: ``bins`` ``[n, nf]`` are the entries' bins of the node's local features, ``q``
    ``[n, S]`` their staged statistics."""
    n, nf = bins.shape
    S = q.shape[1]
    H = np.zeros((nf, B, S), np.int64)
    if n:
        fi = np.broadcast_to(np.arange(nf), (n, nf))
        for s in range(S):
            np.add.at(H[:, :, s], (fi, np.asarray(bins, np.int64)), q[:, s][:, None])
    return H


# --------------------------------------------------------------------------------------------- live region
def live_region(size, dense, per, S):
    """Word offsets of a node's (or segment's) live region. ``dense < 0`` or ``size <= dense``: all ``size`` words.
    Otherwise the first ``dense`` words (multi-bin columns, every bin) and the first ``S`` words -- bin 0 -- of each
    whole ``per = B * S``-word column after them."""
    if dense < 0 or size <= dense:
        return np.arange(size, dtype=np.int64)
    nf = (size - dense) // per
    tail = dense + (np.arange(nf, dtype=np.int64)[:, None] * per + np.arange(S, dtype=np.int64)[None, :]).ravel()
    return np.concatenate([np.arange(dense, dtype=np.int64), tail])


# ------------------------------------------------------------------------------------------- a level's data
def make_level(rng, counts, *, F, nfeat, B, mode, S, wide=False, weights=(0, 1, 1, 2, 255), N=None, n_models=2,
               Xb=None, gap=5, perm=True):
    """Crafted inputs of one tree level: node j owns ``counts[j]`` random entries, model ``j % n_models``, its own
    ``nfeat`` features (a slice of a permutation of the columns at a non-zero ``node_feat_off``) and a histogram
    separated from its neighbours by a gap. Statistics are in (-1, 1) and the per-model scales powers of two with
    ``255 * scale <= 524286`` (the quantisation bound of 4096-row chunks), as the engine picks them."""
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    if Xb is None:
        N = int(N or max(64, 2 * int(counts.max())))
        Xb = rng.integers(0, B, (N, F)).astype(np.uint8)
    N = Xb.shape[0]
    total = int(counts.sum())
    r = rng.integers(0, N, total)
    entries = r.astype(np.uint32) if wide else pack(r, rng.choice(np.asarray(weights), total))
    begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    fl, nfo = [np.full(3, 0, np.int32)], []
    for j in range(n):
        nfo.append(sum(len(x) for x in fl))
        fl.append((rng.permutation(F)[:nfeat] if perm else np.arange(nfeat)).astype(np.int32))
    per = nfeat * B * S
    scales = np.array([[2.0 ** (11 - m - s) for s in range(S)] for m in range(n_models)], np.float32)
    if mode == 0:
        scales[:] = 1
    elif mode == 1:
        scales[:, 0] = 1
    return dict(Xb=Xb, N=N, F=F, B=B, S=S, mode=mode, wide=int(wide), rows=entries, node_begin=begin,
                node_count=counts, node_model=(np.arange(n) % n_models).astype(np.int32),
                feat_list=np.concatenate(fl), node_feat_off=np.asarray(nfo, np.int32),
                node_nfeat=np.full(n, nfeat, np.int32), node_hist_off=np.arange(n, dtype=np.int64) * (per + gap) + 2,
                hist_words=n * (per + gap) + 2, per_node=per,
                y=rng.integers(0, S, N).astype(np.float32),
                t1=rng.uniform(-1, 1, (n_models, N)).astype(np.float32),
                t2=rng.uniform(0, 1, (n_models, N)).astype(np.float32), stride=N, qscale=scales)


def level_hist(L, j, begin, count, f0=0, nf=None, gh=None):
    """``[nf, B, S]`` histogram of entries ``[begin, begin + count)`` over node j's local features ``[f0, f0 + nf)``."""
    nf = int(L["node_nfeat"][j]) - f0 if nf is None else nf
    m = int(L["node_model"][j])
    e = L["rows"][begin:begin + count]
    feats = L["feat_list"][L["node_feat_off"][j] + f0:L["node_feat_off"][j] + f0 + nf]
    row, _ = decode(e, L["wide"])
    q = stage(L["mode"], e, L["wide"], L["S"], y=L["y"], t1=L["t1"][m], t2=L["t2"][m], qs=L["qscale"][m],
              gh=None if gh is None else gh[begin:begin + count])
    return node_hist(L["Xb"][row][:, feats], q, L["B"])


# ----------------------------------------------------------------------------------------------- partition
def splits(feat, params, gain):
    """The split decision: a feature found, a splittable node (params[7]) and a gain above eps (params[6])."""
    p = np.asarray(params, np.float32)
    return bool(feat >= 0 and p[7] > np.float32(0.5) and np.float32(gain) > p[6])


def partition(entries, bins, split_bin, missing_bin, dl, gh=None):
    """``(left, right, nl, nr)`` of a splitting node: ``bins`` are its entries' bins of the split feature. An entry
    goes left when ``bin == missing_bin ? dl : bin <= split_bin``. Order inside a side is not part of the contract:
    compare sorted. With ``gh`` (``[n, 2]``) each side is ``[n_side, 3]`` rows ``(entry, g, h)``."""
    e = np.asarray(entries, np.uint32).astype(np.int64)
    b = np.asarray(bins, np.int64)
    left = np.where((missing_bin >= 0) & (b == missing_bin), bool(dl), b <= split_bin)
    if gh is not None:
        e = np.concatenate([e[:, None], np.asarray(gh, np.int64).reshape(-1, 2)], axis=1)
    return e[left], e[~left], int(left.sum()), int((~left).sum())


def sort_rows(a):
    """Canonical order of a multiset of entries (1-D) or ``(entry, g, h)`` rows (2-D)."""
    a = np.asarray(a)
    if a.ndim == 1:
        return np.sort(a)
    return a[np.lexsort(a.T[::-1])] if a.size else a


# -------------------------------------------------------------------------------------------- leaf collect
def leaf_collect(rows, rows_alt, items, out_rows, out_gid):
    """Plain copies: item ``(begin, count, out, gid, buf)`` copies ``count`` entries of ``rows`` (``rows_alt`` when
    ``buf`` != 0 and it is given) to ``out_rows[out:]`` and writes ``gid`` next to each."""
    for it in items:
        src = rows_alt if (it["buf"] and rows_alt is not None) else rows
        b, c, o = int(it["begin"]), int(it["count"]), int(it["out"])
        out_rows[o:o + c] = src[b:b + c]
        out_gid[o:o + c] = it["gid"]
    return out_rows, out_gid
