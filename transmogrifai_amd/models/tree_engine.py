"""Batched level-wise histogram tree engine.

One engine serves every tree learner of the reference: Spark ``DecisionTree`` / ``RandomForest``
/ ``GBT`` (``OpDecisionTreeClassifier.scala:47-115``, ``OpRandomForestClassifier.scala:59-154``,
``OpGBTClassifier.scala:47-142`` and the regressors) and XGBoost (``OpXGBoostClassifier.scala:47-403``),
i.e. SURVEY.md kernels K23-K25 and K29.

MI355X-first design: instead of training one tree per Spark job, *all* trees of a batch -- every
tree of every (hyper-parameter config x CV fold) -- grow together, level by level. Per level there
is one histogram launch (work items = node row-chunks x feature groups), one split-scan launch,
one partition-count launch, a single device->host sync to collect the split decisions, and one
stable-scatter launch. Rows live in one packed ``uint32`` buffer (row id | bootstrap weight << 24)
partitioned by node, so a level touches only the rows of the nodes still being split. The same
orchestration drives the C++ host kernels when the data lives on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops import _native as N

MODE_CLS, MODE_VAR, MODE_GH = 0, 1, 2
KIND_GINI, KIND_ENTROPY, KIND_VARIANCE, KIND_NEWTON = 0, 1, 2, 3
KINDS = {"gini": KIND_GINI, "entropy": KIND_ENTROPY, "variance": KIND_VARIANCE, "newton": KIND_NEWTON}

ROW_MASK = 0xFFFFFF
CSR_ITEM_ROWS = N.ABI_CONSTS["TMOG_CSR_ITEM_ROWS"]    # rows per CSR histogram item
MAX_ROWS = 1 << 24            # packed entries (row | weight << 24) below this many training rows
MAX_WIDE_ROWS = 1 << 31       # wide entries (32-bit row id, weight 1)


def wide_rows(n_rows: int) -> bool:
    """Entry format of a training set of ``n_rows`` rows: below 2^24 rows the row id and an 8-bit weight share
    one 32-bit entry; from 2^24 rows on (or with ``TMOG_TREE_WIDE_ROWS=1``, for tests) an entry is the row id
    alone and weights become repeated entries (``tree_dev.hpp`` ``ent_row`` / ``ent_w``)."""
    return n_rows >= MAX_ROWS or os.environ.get("TMOG_TREE_WIDE_ROWS") == "1"

# Native per-group resource slots (stream, staging, histogram buffers; tree_grow_hip.hip slots()): grower calls
# running concurrently from several host threads need disjoint slot ranges. A thread running a whole learner next
# to others (tuning/validators.py concurrent learners) takes a lane of SLOT_LANE slots; every grow_forest call of
# that thread -- and of the threads it starts through ``set_slot_lane`` -- offsets its slot_base by the lane.
N_SLOTS, SLOT_LANE = N.ABI_CONSTS["TMOG_N_SLOTS"], N.ABI_CONSTS["TMOG_SLOT_LANE"]
_lane = threading.local()


_lane_lock = threading.Lock()
_quarantined: set = set()       # lane bases held by abandoned fits (maxWait), never handed out until they exit


def slot_lane() -> int:
    """This thread's slot offset: the lane it was given, else the first lane no abandoned fit holds."""
    base = getattr(_lane, "base", None)
    if base is not None:
        return base
    free = free_lanes()
    if not free:
        raise RuntimeError("every native tree-grower slot lane is held by a fit abandoned at its maxWait deadline")
    return free[0]


def set_slot_lane(base: int) -> None:
    if base < 0 or base + SLOT_LANE > N_SLOTS:
        raise ValueError(f"slot lane {base} outside the {N_SLOTS} native slots")
    _lane.base = int(base)


def free_lanes() -> list:
    """Lane bases not held by an abandoned fit, lowest first."""
    with _lane_lock:
        return [b for b in range(0, N_SLOTS, SLOT_LANE) if b not in _quarantined]


def quarantine_lane(base: int, thread: threading.Thread, on_exit=None) -> None:
    """An abandoned fit (tuning/validators.py maxWait) still runs on lane ``base``: its grow-only native buffers
    must not be shared with another grower, so the lane is withheld until ``thread`` exits (a reaper joins it,
    then runs ``on_exit``, e.g. returning the fit's leased stream)."""
    with _lane_lock:
        _quarantined.add(int(base))

    def reap():
        thread.join()
        if on_exit is not None:
            on_exit()
        with _lane_lock:
            _quarantined.discard(int(base))

    threading.Thread(target=reap, name=f"lane-reaper-{base}", daemon=True).start()


def quarantined_lanes() -> set:
    with _lane_lock:
        return set(_quarantined)


@dataclass
class TreeParams:
    max_depth: int = 5
    min_instances: float = 1.0
    min_info_gain: float = 0.0
    min_child_weight: float = 0.0
    reg_lambda: float = 0.0
    gamma: float = 0.0
    eta: float = 1.0
    feature_subset: Optional[int] = None   # features sampled per node (None = all)
    split_eps: float = 0.0                 # split only if gain > split_eps


@dataclass
class TreeJob:
    model: int                      # index into t1/t2 model axis
    params: TreeParams
    rows: torch.Tensor              # int64 row ids of the root (on the engine device)
    weights: Optional[torch.Tensor] = None   # optional integer weights per root row (bootstrap)
    seed: int = 0


@dataclass
class Forest:
    """Flat node arrays for a set of trees (children indices are global into the arrays)."""
    tree_off: np.ndarray            # int64 [T+1]
    nodes: np.ndarray               # int32 [n, 4] (feat, bin, left, right), left < 0 => leaf
    default_left: np.ndarray        # uint8 [n]
    value: np.ndarray               # float32 [n, K]
    gain: np.ndarray                # float32 [n]
    cover: np.ndarray               # float32 [n]  (weighted count / hessian)
    tree_model: np.ndarray          # int32 [T]   job.model for each tree
    missing_bin: int = -1

    @property
    def n_trees(self):
        return len(self.tree_off) - 1

    @property
    def K(self):
        return self.value.shape[1]

    def tree(self, t: int) -> "Forest":
        a, b = int(self.tree_off[t]), int(self.tree_off[t + 1])
        nodes = self.nodes[a:b].copy()
        nodes[:, 2:] = np.where(nodes[:, 2:] >= 0, nodes[:, 2:] - a, -1)
        return Forest(np.array([0, b - a], np.int64), nodes, self.default_left[a:b].copy(),
                      self.value[a:b].copy(), self.gain[a:b].copy(), self.cover[a:b].copy(),
                      self.tree_model[t:t + 1].copy(), self.missing_bin)

    @staticmethod
    def concat(forests: Sequence["Forest"]) -> "Forest":
        offs, nodes, dls, vals, gains, covs, tms = [0], [], [], [], [], [], []
        base = 0
        for f in forests:
            nd = f.nodes.copy()
            nd[:, 2:] = np.where(nd[:, 2:] >= 0, nd[:, 2:] + base, -1)
            nodes.append(nd)
            dls.append(f.default_left)
            vals.append(f.value)
            gains.append(f.gain)
            covs.append(f.cover)
            tms.append(f.tree_model)
            for t in range(f.n_trees):
                offs.append(base + int(f.tree_off[t + 1]))
            base += len(f.nodes)
        return Forest(np.asarray(offs, np.int64), np.concatenate(nodes), np.concatenate(dls),
                      np.concatenate(vals), np.concatenate(gains), np.concatenate(covs),
                      np.concatenate(tms), forests[0].missing_bin if forests else -1)

    def to_state(self) -> dict:
        return {"tree_off": self.tree_off, "nodes": self.nodes, "default_left": self.default_left,
                "value": self.value, "gain": self.gain, "cover": self.cover, "tree_model": self.tree_model,
                "missing_bin": int(self.missing_bin)}

    @staticmethod
    def from_state(d) -> "Forest":
        return Forest(np.asarray(d["tree_off"], np.int64), np.asarray(d["nodes"], np.int32).reshape(-1, 4),
                      np.asarray(d["default_left"], np.uint8), np.asarray(d["value"], np.float32).reshape(
                          len(np.asarray(d["default_left"])), -1),
                      np.asarray(d["gain"], np.float32), np.asarray(d["cover"], np.float32),
                      np.asarray(d["tree_model"], np.int32), int(d.get("missing_bin", -1)))

    def feature_importance(self, n_features: int) -> np.ndarray:
        """Total gain per feature, normalized per tree then averaged (Spark ``featureImportances``)."""
        imp = np.zeros(n_features)
        for t in range(self.n_trees):
            a, b = int(self.tree_off[t]), int(self.tree_off[t + 1])
            ti = np.zeros(n_features)
            nd = self.nodes[a:b]
            internal = nd[:, 2] >= 0
            np.add.at(ti, nd[internal, 0], (self.gain[a:b][internal] * self.cover[a:b][internal]).astype(np.float64))
            s = ti.sum()
            if s > 0:
                imp += ti / s
        s = imp.sum()
        return imp / s if s > 0 else imp


def prune_forest(f: Forest, max_depth: int, min_gain: float) -> Forest:
    """The forest a grower run with a smaller ``max_depth`` and / or a larger ``min_info_gain`` would
    have produced from the same nodes: a node stays split only while its depth is below ``max_depth``
    and its recorded split gain is at least ``min_gain`` (the grower accepts a split exactly when its
    best valid candidate's gain >= min_info_gain, and a larger threshold never changes which candidate
    is best, only whether it is accepted); every other node becomes a leaf with its own statistics,
    which the grower records for internal nodes too. Node order stays BFS per tree, as ``_finalize``
    emits it. Lets the model selector grow one forest per (bootstrap, seed, minInstancesPerNode, ...)
    for all of its maxDepth x minInfoGain grid points (``models/trees.py`` ``_ForestLearner``).
    Thresholds are compared on the stored fp32 gain (a split whose fp64 gain lies within one fp32
    ulp of the threshold may be kept). Leaf statistics: a pruned node keeps the totals of its own
    histogram, where direct growth gives a max-depth right child parent - left (fp32): class counts are
    identical, regression / Newton sums agree to fp32 rounding."""
    n = len(f.nodes)
    if n == 0:
        return f
    left = f.nodes[:, 2].astype(np.int64)
    right = f.nodes[:, 3].astype(np.int64)
    keep = np.zeros(n, bool)
    split = np.zeros(n, bool)
    frontier = f.tree_off[:-1].astype(np.int64)
    frontier = frontier[frontier < f.tree_off[1:]]
    keep[frontier] = True
    mg = np.float32(min_gain)
    d = 0
    while frontier.size:
        ok = (left[frontier] >= 0) & (d < max_depth) & (f.gain[frontier] >= mg)
        sp = frontier[ok]
        split[sp] = True
        frontier = np.sort(np.concatenate([left[sp], right[sp]]))
        keep[frontier] = True
        d += 1
    order = np.nonzero(keep)[0]
    new_id = np.full(n, -1, np.int64)
    new_id[order] = np.arange(order.size)
    tree_off = np.searchsorted(order, f.tree_off).astype(np.int64)
    isint = split[order]
    nodes = np.zeros((order.size, 4), np.int32)
    nodes[:, 0] = np.where(isint, f.nodes[order, 0], 0)
    nodes[:, 1] = np.where(isint, f.nodes[order, 1], 0)
    nodes[:, 2] = np.where(isint, new_id[np.maximum(left[order], 0)], -1)
    nodes[:, 3] = np.where(isint, new_id[np.maximum(right[order], 0)], -1)
    return Forest(tree_off, nodes, np.where(isint, f.default_left[order], 0).astype(np.uint8),
                  f.value[order].copy(), np.where(isint, f.gain[order], 0).astype(np.float32),
                  f.cover[order].copy(), f.tree_model.copy(), f.missing_bin)


def pack_rows(rows: torch.Tensor, weights: Optional[torch.Tensor], wide: bool = False) -> torch.Tensor:
    """Pack ``row | weight << 24`` into an int32 tensor (bit pattern read as uint32 by the kernels). ``wide``:
    entries are the row ids themselves, a weight w > 1 repeating the row w times (zero-weight rows dropped)."""
    if wide:
        r = rows.to(torch.int64)
        if weights is not None:
            r = torch.repeat_interleave(r, weights.to(torch.int64).clamp(0, 255).to(r.device))
        return r.to(torch.int32)
    r = rows.to(torch.int64)
    w = torch.ones_like(r) if weights is None else weights.to(torch.int64).clamp(0, 255)
    e = r | (w << 24)
    e = torch.where(e >= (1 << 31), e - (1 << 32), e)
    return e.to(torch.int32)


def poisson_cdf_table(rate: float) -> List[float]:
    """Inverse-CDF steps of Poisson(rate) exactly as ``trees.bootstrap_weights_multi`` compares them."""
    out = []
    p = math.exp(-rate)
    cdf = p
    for i in range(1, 40):
        out.append(cdf)
        p = p * rate / i
        cdf += p
        if 1.0 - cdf < 1e-12:
            break
    return out


def bootstrap_pack(rows: torch.Tensor, seeds: Sequence[int], rate: float, wide: bool = False):
    """Poisson(``rate``) bootstrap of ``rows`` for one tree per seed, packed as tree-engine root
    entries (``row | w << 24``, zero draws dropped): ``(int32 entries, int64 counts per tree)``.

    Multiplicities are ``trees.bootstrap_weights_multi``'s (same per-row uniform, same CDF steps); on
    the GPU one fused HIP kernel (``boost_kernels.hip: poisson_pack_kernel``) draws and packs."""
    from ..tuning.splitters import row_uniform_multi, _s64
    dev = rows.device
    cdf = poisson_cdf_table(rate)
    rid = rows.to(torch.int64).contiguous()
    k, n = len(seeds), int(rid.numel())
    if dev.type == "cuda" and n and k and not wide:
        offs = np.asarray([_s64(int(sd) * 0x632BE59BD9B4E019 + 23 * 0x2545F4914F6CDD1D) for sd in seeds], np.int64)
        pk = _Pack(dev)
        i_o, i_c = pk.add(offs), pk.add(np.asarray(cdf, np.float64))
        dv = pk.ship()
        cnt = torch.zeros(k, dtype=torch.int64, device=dev)
        lib = N.hip()
        N.check(lib.tmog_hip_poisson_pack(N.ptr(rid), n, N.ptr(dv[i_o]), k, N.ptr(dv[i_c]), len(cdf), N.ptr(cnt),
                                          None, None, N.stream(dev)), "poisson_pack count")
        counts = cnt.cpu().numpy()
        base = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64), device=dev)
        out = torch.empty(max(int(counts.sum()), 1), dtype=torch.int32, device=dev)
        cnt.zero_()
        N.check(lib.tmog_hip_poisson_pack(N.ptr(rid), n, N.ptr(dv[i_o]), k, N.ptr(dv[i_c]), len(cdf), N.ptr(cnt),
                                          N.ptr(base), N.ptr(out), N.stream(dev)), "poisson_pack")
        return out[:int(counts.sum())], counts.astype(np.int64)
    u = row_uniform_multi(rid, seeds, 23)
    w = torch.zeros(u.shape, dtype=torch.int64, device=dev)
    for c in cdf:
        w += (u >= c).to(torch.int64)
    parts, counts = [], []
    for t in range(k):
        keep = w[t] > 0
        parts.append(pack_rows(rid[keep], w[t][keep], wide))
        counts.append(int(parts[-1].numel()))
    out = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int32, device=dev)
    return out, np.asarray(counts, np.int64)


def _root_rows(jobs, dev, wide: bool = False):
    """Packed root entries of every job, zero-weight (out-of-bag) rows dropped for all weighted jobs
    with one compaction (two host syncs per call instead of one per tree). ``wide``: see :func:`pack_rows`."""
    packs: List[Optional[torch.Tensor]] = [None] * len(jobs)
    counts = [0] * len(jobs)
    if wide:
        for k, j in enumerate(jobs):
            packs[k] = pack_rows(j.rows.to(dev), None if j.weights is None else j.weights.to(dev), True)
            counts[k] = int(packs[k].numel())
        rows = torch.cat(packs) if packs else torch.zeros(0, dtype=torch.int32, device=dev)
        return rows, counts
    wj = [k for k, j in enumerate(jobs) if j.weights is not None]
    for k, j in enumerate(jobs):
        if j.weights is None:
            packs[k] = pack_rows(j.rows.to(dev), None)
            counts[k] = int(j.rows.numel())
    if wj:
        sizes = [int(jobs[k].rows.numel()) for k in wj]
        R = torch.cat([jobs[k].rows.to(dev).to(torch.int64) for k in wj])
        W = torch.cat([jobs[k].weights.to(dev).to(torch.int64) for k in wj])
        keep = W > 0
        ends = torch.as_tensor(np.cumsum(sizes) - 1, device=dev)
        csum = keep.to(torch.int64).cumsum(0)
        kc = csum[ends].cpu().numpy()
        kcount = np.diff(np.concatenate([[0], kc]))
        idx = keep.nonzero().squeeze(1)
        packed = pack_rows(R[idx], W[idx])
        for k, part, c in zip(wj, torch.split(packed, kcount.tolist()), kcount):
            packs[k] = part
            counts[k] = int(c)
    rows = torch.cat(packs) if packs else torch.zeros(0, dtype=torch.int32, device=dev)
    return rows, counts


# ctypes mirrors of GrowArgs / ResidentIO, derived from ops/csrc/common/tmog_abi.h; built by keyword only
_GrowArgs, _ResidentIO = N.STRUCTS["GrowArgs"], N.STRUCTS["ResidentIO"]
REC_FIXED = N.ABI_CONSTS["TMOG_REC_FIXED"]     # record words before the S totals: tree feat bin dl gain left right


@dataclass
class ResidentTree:
    """One device-planned ``grow_forest`` call (``resident=True``): the leaf assignment for the boosting
    epilogue is ready on the device, the created-node records ``rec`` (``[1 + cap, 7 + S]`` int64, row 0 =
    (nodes, leaf entries, error bits)) are read back later, in bulk, by :func:`resident_forests`."""
    leaf_assign: "LeafAssign"
    rec: torch.Tensor
    jobs: list
    mode: int
    kind: int
    S: int
    missing_bin: int


def resident_forests(trees: Sequence[ResidentTree]) -> List[Forest]:
    """Host Forests of device-planned trees: ONE device->host copy of all their records, then the native
    finalisation (``tmog_tree_finalize_cpu``, the host twin of the device's ``tree_finalize_kernel``)."""
    if not trees:
        return []
    recs = [t.rec for t in trees]
    host = torch.cat([r.reshape(-1) for r in recs]).cpu().numpy() if len(recs) > 1 else recs[0].reshape(-1).cpu().numpy()
    out, off = [], 0
    for t in trees:
        W = REC_FIXED + t.S
        sz = int(t.rec.numel())
        blk = host[off:off + sz].reshape(-1, W)
        off += sz
        n, err = int(blk[0, 0]), int(blk[0, 2])
        if err:
            raise RuntimeError(f"device-planned tree growth failed (error bits {err}: 1 = partition cursor mismatch, "
                               f"2 = work-list capacity)")
        r = blk[1:1 + n]
        G = _Nodes(n, t.S)
        G.tree[:] = r[:, 0]
        G.feat[:] = r[:, 1]
        G.bin[:] = r[:, 2]
        G.dl[:] = r[:, 3].astype(np.uint8)
        G.gain[:] = r[:, 4].view(np.float64)
        G.left[:] = r[:, 5]
        G.right[:] = r[:, 6]
        G.tot[:] = np.ascontiguousarray(r[:, REC_FIXED:REC_FIXED + t.S]).view(np.float64)
        K = 1
        out.append(_finalize(t.jobs, G, t.mode, t.kind, K, t.S, t.missing_bin))
    return out


def resident_enabled() -> bool:
    """Device-planned level loop for boosting (``TMOG_TREE_RESIDENT``, default on)."""
    return os.environ.get("TMOG_TREE_RESIDENT", "1") != "0"


_ENTRY_MODELS: Dict[tuple, torch.Tensor] = {}


def _entry_models(models: tuple, counts: tuple, dev) -> torch.Tensor:
    """Model id of every root entry (job j's ``counts[j]`` entries carry ``models[j]``), cached: the boosting
    rounds of one active job set reuse it. One fill per job -- ``torch.repeat_interleave`` with a handful
    of repeats runs one thread per repeat on ROCm (~350 us for 2M entries)."""
    key = (models, counts, str(dev), _stream_key(dev))
    t = _ENTRY_MODELS.get(key)
    if t is None:
        if len(_ENTRY_MODELS) >= 32:
            _ENTRY_MODELS.clear()
        parts = [torch.full((c,), m, dtype=torch.int64, device=dev) for m, c in zip(models, counts) if c]
        t = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=dev)
        _ENTRY_MODELS[key] = t
    return t


def _stage_gh(rows: torch.Tensor, counts, jobs, t1f, t2f, qscale, stride: int, wide: bool = False) -> torch.Tensor:
    """``[total, 2]`` int32: each root entry's quantised (q(w g), q(w h)) under its job's model scales -- the
    histogram kernels' ``rintf((w * t) * qscale)`` in the same fp32 operation order (tree_hist_kernels.hip
    stage_row), so the histograms are bit-identical to gathering t1 / t2 per row."""
    dev = rows.device
    e = rows.to(torch.int64) & 0xFFFFFFFF
    r = e if wide else e & 0xFFFFFF
    w = torch.ones_like(e, dtype=torch.float32) if wide else (e >> 24).to(torch.float32)
    model = _entry_models(tuple(int(j.model) for j in jobs), tuple(int(c) for c in counts), dev)
    idx = model * int(stride) + r
    qs = qscale.reshape(-1, qscale.shape[-1])[model]
    g = torch.round((w * t1f.reshape(-1)[idx]) * qs[:, 0]).to(torch.int32)
    h = torch.round((w * t2f.reshape(-1)[idx]) * qs[:, 1]).to(torch.int32)
    return torch.stack([g, h], 1).contiguous()


@dataclass
class FpPlan:
    """This rank's share of a feature-parallel ``grow_forest`` (see parallel/learner_parallel.py):
    positions ``[mlo, mhi)`` of the multi-bin and ``[olo, ohi)`` of the one-present-bin growth-order
    feature lists, and ``one_cols`` = the ``Xb`` columns of that one-present slice (the CSR to build)."""
    par: object                      # parallel.learner_parallel.LearnerParallel
    mlo: int
    mhi: int
    olo: int
    ohi: int
    one_cols: np.ndarray
    sparse: bool = False


def fp_plan(Xb: torch.Tensor, n_bins, par, sparse: bool, force: bool = False) -> Optional[FpPlan]:
    """Split the features of ``Xb`` over ``par``'s ranks for feature-parallel growth (None when not
    possible: one rank, or fewer multi-bin columns than ranks -- then every rank grows everything).
    ``sparse``: MODE_GH with a missing bin, where one-present-bin columns form their own list."""
    from ..parallel.learner_parallel import feature_slices
    if par is None or (par.world <= 1 and not force):
        return None
    nb = np.asarray(n_bins)
    if sparse:
        multi, one = np.nonzero(nb != 1)[0], np.nonzero(nb == 1)[0]
    else:
        multi, one = np.arange(nb.size), np.zeros(0, np.int64)
    if one.size:
        idx = torch.as_tensor(one, dtype=torch.int64, device=Xb.device)
        w = torch.zeros(one.size, dtype=torch.float64, device=Xb.device)
        for r0 in range(0, int(Xb.shape[0]), 1 << 20):
            w += (Xb[r0:r0 + (1 << 20)].index_select(1, idx) == 0).sum(0).to(torch.float64)
        weights = w.cpu().numpy()
    else:
        weights = np.zeros(0)
    sl = feature_slices(int(multi.size), weights, par.world, force=force)
    if sl is None:
        return None
    mlo, mhi, olo, ohi = sl[par.rank]
    return FpPlan(par, mlo, mhi, olo, ohi, one[olo:ohi].astype(np.int64), bool(sparse))


def onebin_csr(Xb: torch.Tensor, n_bins: np.ndarray, block_rows: int = 1 << 20, cols: Optional[np.ndarray] = None):
    """Row-wise CSR of the one-present-bin columns of ``Xb`` (``n_bins == 1``: one-hot / null indicator
    columns under a sparse missing bin), for the histogram kernel's CSR path.

    Returns ``(ptr int64 [N + 1], col int16 [max(nnz, 1)] (read as uint16), n_cols)``: the entries of
    row ``r`` are ``col[ptr[r]:ptr[r + 1]]``, the ids (in ascending column order among the one-bin
    columns) of its columns holding the present bin 0. None when there are none or ids do not fit.
    ``cols``: restrict to these one-present-bin columns (a feature-parallel rank's slice), ids local to
    the subset."""
    nb = np.asarray(n_bins)
    one = np.nonzero(nb == 1)[0] if cols is None else np.asarray(cols, np.int64)
    if one.size == 0 or one.size >= (1 << 16) or Xb.dim() != 2:
        return None
    dev = Xb.device
    idx = torch.as_tensor(one, dtype=torch.int64, device=dev)
    N = int(Xb.shape[0])
    counts, cols = [], []
    for r0 in range(0, N, block_rows):
        nz = Xb[r0:r0 + block_rows].index_select(1, idx) == 0
        counts.append(nz.sum(1))
        cols.append(nz.nonzero()[:, 1].to(torch.int16))    # row-major: sorted by row, then column
    ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if N:
        torch.cumsum(torch.cat(counts), 0, out=ptr[1:])
    col = torch.cat(cols) if cols else torch.empty(0, dtype=torch.int16, device=dev)
    if col.numel() == 0:
        col = torch.zeros(1, dtype=torch.int16, device=dev)
    return ptr, col.contiguous(), int(one.size)


class _Nodes:
    """Created nodes of one job group, in creation order (what ``_finalize`` consumes)."""

    def __init__(self, n, S):
        self.n = n
        self.tree = np.empty(n, np.int64)
        self.feat = np.empty(n, np.int64)
        self.bin = np.empty(n, np.int64)
        self.dl = np.empty(n, np.uint8)
        self.gain = np.empty(n, np.float64)
        self.tot = np.empty((n, S), np.float64)
        self.left = np.empty(n, np.int64)
        self.right = np.empty(n, np.int64)


def grow_forest(Xb: torch.Tensor, n_bins: np.ndarray, jobs: Sequence[TreeJob], *, mode: int, kind: int,
                n_classes: int = 2, y: Optional[torch.Tensor] = None, t1: Optional[torch.Tensor] = None,
                t2: Optional[torch.Tensor] = None, B: int = 32, missing_bin: int = -1,
                subtract: bool = True, chunk_rows: int = 4096, rng_seed: int = 0,
                collect_leaves: bool = False, groups: Optional[int] = None, csr=None, root=None,
                fp: Optional[FpPlan] = None, slot_base: int = 0, XbT: Optional[torch.Tensor] = None,
                quant_amax: Optional[torch.Tensor] = None, quant_wmax: Optional[float] = None,
                resident: bool = False, prestaged=None, Xh: Optional[torch.Tensor] = None):
    """Grow one tree per job, all jobs level-synchronously. ``Xb`` is ``uint8 [N, F]``.

    The level loop runs natively (``ops/csrc/common/tree_grow.hpp``): on the GPU every job group gets
    its own host thread and HIP stream (default 2 groups) so one group's planning overlaps the other's
    kernels; the CPU backend grows the same groups with the same seeds, bit-identically. Per-node
    feature subsets come from a splitmix64 stream seeded with ``rng_seed + 1000003 * group``.

    ``root``: pre-packed root entries ``(int32 tensor, counts per job)`` (e.g. from ``bootstrap_pack``),
    used instead of the jobs' rows / weights; the tensor is consumed (the grower partitions it in place).

    ``csr``: ``onebin_csr(Xb, n_bins)`` (GPU, ``MODE_GH`` with a missing bin): the one-present-bin
    columns' histograms are then built from the rows' CSR lists (identical results, fewer loads).

    ``collect_leaves``: also return, as ``forest.leaf_assign``, the final leaf of every training entry
    (see ``LeafAssign``) so boosting can update margins without re-walking the new trees.

    ``slot_base``: first native per-group resource slot (stream, staging, histogram buffers) of this call;
    calls running concurrently from several host threads must use disjoint slot ranges.

    ``quant_amax`` ``[n_models, 2]`` float32 / ``quant_wmax``: the per-model max |t1|, max |t2| over all N rows
    and the max entry weight, when the caller already knows them (boosting: the round epilogue computes
    them), instead of scanning ``t1`` / ``t2`` / the entries here -- same scales.

    ``fp``: feature-parallel growth (``fp_plan``): every rank calls with the same jobs, rows and ``Xb``;
    each builds histograms of its feature slice only (``csr`` must then be the slice's, from
    ``onebin_csr(..., cols=fp.one_cols)``) and all ranks return the same forest -- the one a single
    rank would grow. Jobs must not use per-node feature subsets.

    ``Xh``: GPU, optional ``uint8 [N, Fh]`` row-major copy of ``Xb[:, :Fh]`` (``Fh`` a multiple of 64) holding the
    multi-bin columns; the wide-load histogram items read it instead of ``Xb`` (aligned row segments, a smaller
    footprint for the Infinity Cache). Same trees.

    ``resident``: on the GPU, for one job group (``groups=1``), no per-node feature subsets and leaves
    collected, grow with the device-planned level loop (``ops/csrc/hip/tree_resident.hip``): nothing is
    read back, and a :class:`ResidentTree` is returned instead of a Forest (same trees; the host Forest is
    built later by :func:`resident_forests`). Other configurations fall back to the host-planned loop.

    ``prestaged``: ``(rows, counts, gh, qscale, qinv)`` already prepared on this stream by the fused round
    prologue (``boost_prologue``): the root entries (consumed), their quantised statistics and the scales."""
    dev = Xb.device
    on_gpu = dev.type == "cuda"
    slot_base = int(slot_base) + slot_lane()
    Nrows, F = int(Xb.shape[0]), int(Xb.shape[1])
    chunk_rows = int(os.environ.get("TMOG_TREE_CHUNK", chunk_rows))
    wide = wide_rows(Nrows)
    if Nrows >= MAX_WIDE_ROWS:
        raise ValueError(f"tree engine supports < 2^31 rows per training set, got {Nrows}")
    S = n_classes if mode == MODE_CLS else (3 if mode == MODE_VAR else 2)
    K = n_classes if mode == MODE_CLS else 1
    if missing_bin >= B:
        raise ValueError("missing_bin must be < B")
    if S > 256:
        raise ValueError("tree engine supports at most 256 statistics per bin (classes)")
    if on_gpu and (S > 16 or B > 64) and B * S > 16384:
        raise ValueError(f"tree engine (GPU) supports bins x classes <= 16384, got {B} x {S}")
    n_bins_t = _const_tensor(np.asarray(n_bins, np.int32), dev)
    stride = int(t1.shape[1]) if (t1 is not None and t1.dim() == 2) else 0
    yf = y.to(device=dev, dtype=torch.float32).contiguous() if y is not None else None
    t1f = t1.to(device=dev, dtype=torch.float32).contiguous() if t1 is not None else None
    t2f = t2.to(device=dev, dtype=torch.float32).contiguous() if t2 is not None else None
    Xb = Xb.contiguous()
    T = len(jobs)
    ng = groups if groups is not None else min(T, max(1, min(8, int(os.environ.get("TMOG_TREE_GROUPS", "2")))))
    ng = max(1, min(ng, T)) if T else 1
    cuts = np.linspace(0, T, ng + 1).astype(np.int32)
    if prestaged is not None:
        rows, counts = prestaged[0], [int(c) for c in prestaged[1]]
        if len(counts) != len(jobs) or sum(counts) != int(rows.numel()):
            raise ValueError("root entries do not match the jobs")
    elif root is not None:
        rows, counts = root[0].to(device=dev, dtype=torch.int32).contiguous(), [int(c) for c in root[1]]
        if len(counts) != len(jobs) or sum(counts) != int(rows.numel()):
            raise ValueError("root entries do not match the jobs")
    else:
        rows, counts = _root_rows(jobs, dev, wide)
    rows_alt = torch.empty_like(rows)
    total = int(rows.numel())
    gh = gh_alt = None
    if prestaged is not None:
        gh, qscale, qinv = prestaged[2], prestaged[3], prestaged[4]
        gh_alt = torch.empty_like(gh)
    else:
        qscale, qinv = _quant_scales(mode, S, jobs, t1f, t2f, rows, chunk_rows, dev, quant_amax,
                                     1.0 if wide else quant_wmax)
    if gh is None and on_gpu and mode == MODE_GH and total and t1f is not None and t2f is not None \
            and os.environ.get("TMOG_GH_STAGE", "1") != "0":
        gh = _stage_gh(rows, counts, jobs, t1f, t2f, qscale, stride, wide)
        gh_alt = torch.empty_like(gh)
    leaf_rows = torch.empty(max(total, 1), dtype=torch.int32, device=dev) if collect_leaves else None
    leaf_gid = torch.empty(max(total, 1), dtype=torch.int32, device=dev) if collect_leaves else None
    host = dict(
        model=np.array([j.model for j in jobs], np.int32), depth=np.array([j.params.max_depth for j in jobs], np.int32),
        inst=np.array([j.params.min_instances for j in jobs], np.float64),
        gain=np.array([j.params.min_info_gain for j in jobs], np.float64),
        mcw=np.array([j.params.min_child_weight for j in jobs], np.float64),
        lam=np.array([j.params.reg_lambda for j in jobs], np.float64),
        eps=np.array([j.params.split_eps for j in jobs], np.float64),
        fsub=np.array([0 if j.params.feature_subset is None else int(j.params.feature_subset) for j in jobs], np.int32),
        count=np.asarray(counts, np.int64), cuts=cuts, nbins=np.ascontiguousarray(np.asarray(n_bins, np.int32)))
    hp = {k: v.ctypes.data for k, v in host.items()}
    use_csr = (csr is not None and on_gpu and mode == MODE_GH and missing_bin > 0
               and os.environ.get("TMOG_TREE_CSR") != "0")
    if use_csr and (int(csr[0].numel()) != Nrows + 1 or csr[0].device != dev or csr[1].dtype != torch.int16):
        raise ValueError("csr does not match Xb")
    fpw = 0 if fp is None else int(fp.par.world)      # 0 = not feature-parallel
    if fpw > 0:
        if fp.sparse != (mode == MODE_GH and missing_bin >= 0):
            raise ValueError("feature-parallel plan was made for another histogram mode")
        if any(j.params.feature_subset is not None and 0 < int(j.params.feature_subset) < F for j in jobs):
            raise ValueError("feature-parallel growth needs jobs without per-node feature subsets")
        if use_csr and int(csr[2]) != fp.ohi - fp.olo:
            raise ValueError("feature-parallel growth needs the CSR of this rank's one-present-bin slice")
        fp_comm = fp.par.fp.comm_array(dev, ng) if on_gpu else None
        fp_cb = None if on_gpu else fp.par.fp.exchange_fn()
    else:
        fp_comm = fp_cb = None
    a = _GrowArgs(
        Xb=N.ptr(Xb), N=Nrows, F=F, mode=mode, kind=kind, S=S, B=B, missing_bin=missing_bin,
        chunk_rows=int(chunk_rows), subtract=int(bool(subtract)), collect_leaves=int(bool(collect_leaves)),
        y=N.ptr(yf), t1=N.ptr(t1f), t2=N.ptr(t2f), stride=stride, qscale=N.ptr(qscale), qinv=N.ptr(qinv),
        n_bins=N.ptr(n_bins_t), T=T, job_model=hp["model"], job_depth=hp["depth"], job_min_inst=hp["inst"],
        job_min_gain=hp["gain"], job_mcw=hp["mcw"], job_lambda=hp["lam"], job_eps=hp["eps"], job_fsub=hp["fsub"],
        job_count=hp["count"], rows=N.ptr(rows), rows_alt=N.ptr(rows_alt), leaf_rows=N.ptr(leaf_rows),
        leaf_gid=N.ptr(leaf_gid), n_groups=ng, group_start=hp["cuts"], rng_seed=int(rng_seed),
        stream=N.stream(dev) if on_gpu else None,
        n_bins_host=hp["nbins"] if (fpw > 0 or os.environ.get("TMOG_TREE_PERM") != "0") else None,
        csr_ptr=N.ptr(csr[0]) if use_csr else None, csr_col=N.ptr(csr[1]) if use_csr else None,
        csr_nf=int(csr[2]) if use_csr else 0,
        fp_rank=int(fp.par.rank) if fpw else 0, fp_world=fpw, fp_mlo=fp.mlo if fpw else 0,
        fp_mhi=fp.mhi if fpw else 0, fp_olo=fp.olo if fpw else 0, fp_ohi=fp.ohi if fpw else 0,
        fp_comm=C.cast(fp_comm, C.c_void_p) if fp_comm is not None else None,
        fp_exchange=C.cast(fp_cb, C.c_void_p) if fp_cb is not None else None, fp_ctx=None,
        slot_base=int(slot_base), XbT=N.ptr(XbT) if (on_gpu and XbT is not None) else None,
        gh=N.ptr(gh) if gh is not None else None, gh_alt=N.ptr(gh_alt) if gh_alt is not None else None,
        n_entries=total, wide_rows=int(wide), Xh=N.ptr(Xh) if (on_gpu and Xh is not None) else None,
        Fh=int(Xh.shape[1]) if (on_gpu and Xh is not None) else 0)
    lib = N.hip() if on_gpu else N.host()
    if resident and on_gpu and ng == 1 and collect_leaves:
        rt = _grow_resident(lib, a, jobs, mode, kind, S, missing_bin, leaf_rows, leaf_gid, dev, total, wide)
        if rt is not None:
            return rt
    fn = (lambda name: getattr(lib, f"tmog_hip_{name}")) if on_gpu else (lambda name: getattr(lib, f"tmog_{name}_cpu"))
    side = []
    if on_gpu and ng > 1 and fpw == 0:
        # groups beyond the first run on side streams of the process-wide set (ops/streams.py), shared when
        # fewer are free; the grouping itself (and so every tree) does not depend on how many were free
        from ..ops import streams as SP
        null_base = int(N.stream(dev) or 0) == 0
        side = SP.lease(dev, ng if null_base else ng - 1)
        for g in range(ng):
            k = g if null_base else g - 1
            if k >= 0:
                lib.tmog_hip_slot_stream(slot_base + g, side[k % len(side)].cuda_stream if side else None,
                                         1 if side else 0)
    try:
        h = fn("grow_forest")(C.byref(a))
    finally:
        if side:
            from ..ops import streams as SP
            SP.release(dev, side)
    try:
        msg = C.create_string_buffer(512)
        if fn("grow_status")(h, msg, 512) != 0:
            raise RuntimeError(f"native tree grower failed: {msg.value.decode(errors='replace')}")
        forests, las = [], []
        entry0 = np.concatenate([[0], np.cumsum(host["count"])])
        for g in range(ng):
            n = int(fn("grow_nodes")(h, g))
            G = _Nodes(n, S)
            fn("grow_copy")(h, g, G.tree.ctypes.data, G.feat.ctypes.data, G.bin.ctypes.data, G.dl.ctypes.data,
                            G.gain.ctypes.data, G.tot.ctypes.data, G.left.ctypes.data, G.right.ctypes.data)
            gj = list(jobs[cuts[g]:cuts[g + 1]])
            f = _finalize(gj, G, mode, kind, K, S, missing_bin, with_gid_values=collect_leaves)
            if collect_leaves:
                lc = int(fn("grow_leaf_count")(h, g))
                e0 = int(entry0[cuts[g]])
                pk = _Pack(dev)
                i_v, i_t = pk.add(f._gid_value), pk.add(f._gid_tree + int(cuts[g]))
                dv = pk.ship()
                las.append((leaf_rows[e0:e0 + lc], leaf_gid[e0:e0 + lc], dv[i_v], dv[i_t]))
                del f._gid_value, f._gid_tree
            forests.append(f)
    finally:
        fn("grow_free")(h)
    forest = forests[0] if ng == 1 else Forest.concat(forests)
    if collect_leaves:
        if ng == 1:
            r_, g_, v_, t_ = las[0]
            forest.leaf_assign = LeafAssign(r_, g_, v_, t_, wide)
        else:
            goff = np.concatenate([[0], np.cumsum([int(x[2].shape[0]) for x in las])[:-1]])
            forest.leaf_assign = LeafAssign(torch.cat([x[0] for x in las]),
                                            torch.cat([x[1] + int(o) for x, o in zip(las, goff)]),
                                            torch.cat([x[2] for x in las]), torch.cat([x[3] for x in las]), wide)
    return forest


def _grow_resident(lib, a, jobs, mode, kind, S, missing_bin, leaf_rows, leaf_gid, dev, total,
                   wide: bool = False) -> Optional[ResidentTree]:
    cap = int(lib.tmog_hip_resident_cap_nodes(C.byref(a)))
    if cap <= 0:
        return None
    rec = torch.empty(1 + cap, REC_FIXED + S, dtype=torch.int64, device=dev)
    gid_value = torch.empty(cap, dtype=torch.float32, device=dev)
    gid_tree = torch.empty(cap, dtype=torch.int64, device=dev)
    eta = np.ascontiguousarray([j.params.eta for j in jobs], np.float64)
    gam = np.ascontiguousarray([j.params.gamma for j in jobs], np.float64)
    io = _ResidentIO(rec=N.ptr(rec), gid_value=N.ptr(gid_value), gid_tree=N.ptr(gid_tree), cap_nodes=cap,
                     job_eta=eta.ctypes.data, job_gamma=gam.ctypes.data)
    rc = int(lib.tmog_hip_grow_resident(C.byref(a), C.byref(io)))
    if rc == 1:
        return None
    if rc != 0:
        msg = C.create_string_buffer(512)
        lib.tmog_hip_resident_error(msg, 512)
        raise RuntimeError(f"device-planned tree growth failed: {msg.value.decode(errors='replace')}")
    la = LeafAssign(leaf_rows[:total], leaf_gid[:total], gid_value, gid_tree, wide)
    return ResidentTree(la, rec, list(jobs), mode, kind, S, missing_bin)


@dataclass
class LeafAssign:
    """Final leaf of every training entry of a ``grow_forest`` call: ``rows`` (packed entries, as
    given to the trees), ``gid`` (node id per entry), ``value[gid]`` (leaf output, pruning applied),
    ``tree[gid]`` (job index). ``per_tree_values`` turns it into margin updates."""
    rows: torch.Tensor
    gid: torch.Tensor
    value: torch.Tensor
    tree: torch.Tensor
    wide: bool = False          # entries are plain row ids (training sets of >= 2^24 rows)

    def row_ids(self) -> torch.Tensor:
        if self.wide:
            return self.rows.to(torch.int64) & 0xFFFFFFFF
        return (self.rows & 0xFFFFFF).to(torch.int64)

    def entry_tree(self) -> torch.Tensor:
        return self.tree[self.gid.to(torch.int64)]

    def entry_value(self) -> torch.Tensor:
        return self.value[self.gid.to(torch.int64)]


from ..ops.staging import Pack as _Pack  # noqa: E402  (re-exported for the learners)


_CONST: dict = {}


def _stream_key(dev) -> int:
    """The calling thread's current stream on ``dev`` (0 on the host). The device-tensor caches below are kept
    per stream: a cached tensor is then only ever read by kernels of the stream it was allocated on, so when an
    eviction frees it the caching allocator can hand its block only to later work of that same stream. Shared
    across streams (the boosting parts, the learner lanes), an evicted tensor's block could be reused on its
    allocation stream while another stream's queued kernels still read it -- stale index tensors, and faults."""
    dev = torch.device(dev)
    return int(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else 0


def _const_tensor(a: np.ndarray, dev) -> torch.Tensor:
    """Device copy of a small constant host array, cached by content and stream (no per-call blocking copy)."""
    key = (str(dev), _stream_key(dev), a.dtype.str, a.shape, a.tobytes())
    t = _CONST.get(key)
    if t is None:
        if len(_CONST) > 256:
            _CONST.clear()
        t = _CONST[key] = torch.as_tensor(a, device=dev)
    return t


def quant_qmax(chunk_rows: int = 4096) -> float:
    """Per-row bound of a quantised statistic: an LDS partial sums at most max(chunk_rows, CSR_ITEM_ROWS) rows
    (CSR items always span 1024 rows, tree_grow.hpp kCsrRows), and must fit int32."""
    chunk_rows = int(os.environ.get("TMOG_TREE_CHUNK", chunk_rows))
    return float(min(1 << 22, (2 ** 31 - 1) // max(1, int(chunk_rows), CSR_ITEM_ROWS) - 1))


def boost_prologue(root: torch.Tensor, counts, act, G: torch.Tensor, H: torch.Tensor, amax: torch.Tensor,
                   comp: torch.Tensor, tam_prev: Optional[torch.Tensor], tam_next: torch.Tensor, out: dict,
                   wide: bool = False):
    """Set-up of one device-resident boosting round in a single launch (ops/csrc/hip/boost_kernels.hip
    boost_prologue_kernel): the quantisation maxima of the active jobs ``act`` (model index = job) from
    ``comp`` and the previous epilogue's ``tam_prev`` (None: first round, ``amax`` as it is), their
    power-of-two scales, a copy of the packed ``root`` entries and their quantised (g, h); zeroes the jobs'
    entries of ``tam_next``. ``out`` holds the reusable buffers; returns grow_forest's ``prestaged``."""
    dev = root.device
    total = int(root.numel())
    P = int(G.shape[0])
    if out.get("rows") is None or out["rows"].numel() < total:
        out["rows"] = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        out["gh"] = torch.empty(max(total, 1), 2, dtype=torch.int32, device=dev)
    if out.get("qscale") is None:
        out["qscale"] = torch.ones(P, 2, dtype=torch.float32, device=dev)
        out["qinv"] = torch.ones(P, 2, dtype=torch.float64, device=dev)
    rows, gh = out["rows"][:total], out["gh"][:total]
    act_t = _const_tensor(np.asarray(act, np.int32), dev)
    off = _const_tensor(np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64), dev)
    rc = N.hip().tmog_hip_boost_prologue(N.ptr(tam_prev) if tam_prev is not None else None, N.ptr(tam_next),
                                         N.ptr(comp), N.ptr(amax), P, N.ptr(act_t), len(act), N.ptr(off),
                                         N.ptr(root), N.ptr(rows), total, N.ptr(G), N.ptr(H), int(G.shape[1]),
                                         N.ptr(gh), N.ptr(out["qscale"]), N.ptr(out["qinv"]), quant_qmax(),
                                         int(bool(wide)), N.stream(dev))
    if rc != 0:
        raise RuntimeError(f"boost prologue launch failed ({rc})")
    return rows, list(counts), gh, out["qscale"], out["qinv"]


def _quant_scales(mode, S, jobs, t1f, t2f, rows, chunk_rows, dev, amax_hint=None, wmax_hint=None):
    """Per-(model, stat) power-of-two fixed-point scales for the int64 histograms (see the
    "Fixed-point statistics" note in ops/csrc/hip/tree_hist_kernels.hip). A row's contribution is
    ``rint(v * scale)`` with ``|v * scale| <= qmax``, so a ``chunk_rows``-row LDS partial fits int32.
    Computed on the device (no host sync); returns (float32 scales, float64 inverses), ``[n_models, S]``."""
    n_models = max([j.model for j in jobs], default=0) + 1
    if mode == MODE_CLS or rows.numel() == 0:
        one = torch.ones(n_models, S, dtype=torch.float32, device=dev)
        return one, one.to(torch.float64)
    qmax = quant_qmax(chunk_rows)
    wmax = torch.tensor(float(wmax_hint), dtype=torch.float32, device=dev) if wmax_hint is not None else \
        ((rows >> 24) & 0xFF).max().to(torch.float32)

    def amax(t, k=0):
        if amax_hint is not None:
            return amax_hint[:n_models, k].to(torch.float32)
        if t is None:
            return torch.zeros(n_models, dtype=torch.float32, device=dev)
        v = t.reshape(t.shape[0], -1) if t.dim() == 2 else t.reshape(1, -1)
        L = v.shape[1]
        if L >= 1 << 16:        # row-wise amax of a few long rows: split each row into 256 segments
            seg = -(-L // 256)
            a = v.abs()
            if seg * 256 != L:
                a = torch.nn.functional.pad(a, (0, seg * 256 - L))
            m = a.view(v.shape[0], 256, seg).amax(2).amax(1)
        else:
            m = v.abs().amax(1)
        return m.expand(n_models) if m.numel() == 1 else m[:n_models]

    def pow2(bound):
        # 2^floor(log2 x) built from the exponent bits of x = qmax / bound (an IEEE division, not torch's
        # reciprocal-times-scalar): exact and identical on every device, and the same bits as the fused round
        # prologue (boost_kernels.hip pow2_scale)
        b = (bound * wmax).to(torch.float32).clamp_min(1e-30)
        x = torch.full_like(b, qmax) / b
        e = ((x.view(torch.int32) >> 23) & 0xFF) - 127
        return ((e.clamp(-60, 60) + 127) << 23).to(torch.int32).view(torch.float32)

    if mode == MODE_VAR:
        m1 = amax(t1f)
        sc = torch.stack([torch.ones_like(m1), pow2(m1), pow2(m1 * m1)], 1)
    else:
        sc = torch.stack([pow2(amax(t1f, 0)), pow2(amax(t2f, 1))], 1)
    sc = sc.to(torch.float32).contiguous()
    return sc, (1.0 / sc.to(torch.float64)).contiguous()


def _finalize(jobs, G: "_Nodes", mode, kind, K, S, missing_bin, with_gid_values: bool = False):
    """Created nodes -> Forest (values, gamma pruning, per-tree regrouping): native
    ``tmog_tree_finalize_cpu`` (ops/csrc/host/tree_cpu.cpp), array-identical to ``_finalize_py``."""
    if os.environ.get("TMOG_FINALIZE_PY") == "1":
        return _finalize_py(jobs, G, mode, kind, K, S, missing_bin, with_gid_values)
    n = G.n
    T = len(jobs)
    lam = np.ascontiguousarray([j.params.reg_lambda for j in jobs], np.float64)
    eta = np.ascontiguousarray([j.params.eta for j in jobs], np.float64)
    gam = np.ascontiguousarray([j.params.gamma for j in jobs], np.float64)
    tree_off = np.empty(T + 1, np.int64)
    nodes = np.empty((max(n, 1), 4), np.int32)
    dl = np.empty(max(n, 1), np.uint8)
    value = np.empty((max(n, 1), K), np.float32)
    gain = np.empty(max(n, 1), np.float32)
    cover = np.empty(max(n, 1), np.float32)
    gid_value = np.empty((max(n, 1), K), np.float32) if with_gid_values else None
    tot = np.ascontiguousarray(G.tot[:n])
    m = int(N.host().tmog_tree_finalize_cpu(
        n, T, G.tree.ctypes.data, G.feat.ctypes.data, G.bin.ctypes.data, G.dl.ctypes.data, G.gain.ctypes.data,
        tot.ctypes.data, S, G.left.ctypes.data, G.right.ctypes.data, mode, kind, K, lam.ctypes.data,
        eta.ctypes.data, gam.ctypes.data, int(bool(with_gid_values)), tree_off.ctypes.data, nodes.ctypes.data,
        dl.ctypes.data, value.ctypes.data, gain.ctypes.data, cover.ctypes.data,
        gid_value.ctypes.data if with_gid_values else None))
    f = Forest(tree_off, nodes[:m].copy(), dl[:m].copy(), value[:m].copy(), gain[:m].copy(), cover[:m].copy(),
               np.array([j.model for j in jobs], np.int32), missing_bin)
    if with_gid_values:
        f._gid_value, f._gid_tree = gid_value[:n], G.tree[:n].astype(np.int64)
    return f


def _finalize_py(jobs, G: "_Nodes", mode, kind, K, S, missing_bin, with_gid_values: bool = False):
    n = G.n
    tot = G.tot[:n]
    left = G.left[:n].copy()
    right = G.right[:n].copy()
    feat = G.feat[:n].copy()
    gain = G.gain[:n]
    tree = G.tree[:n]
    if mode == MODE_CLS:
        s = tot.sum(1, keepdims=True)
        value = np.where(s > 0, tot / np.maximum(s, 1e-300), 0.0)
        cover = s[:, 0]
    elif mode == MODE_VAR:
        value = np.where(tot[:, :1] > 0, tot[:, 1:2] / np.maximum(tot[:, :1], 1e-300), 0.0)
        cover = tot[:, 0]
    else:
        lam = np.array([j.params.reg_lambda for j in jobs])[tree]
        eta = np.array([j.params.eta for j in jobs])[tree]
        value = (-tot[:, 0] / (tot[:, 1] + lam) * eta)[:, None]
        cover = tot[:, 1]
    if kind == KIND_NEWTON:
        gam = np.array([j.params.gamma for j in jobs])[tree]
        while True:
            idx = np.nonzero(left >= 0)[0]
            if idx.size == 0:
                break
            leafy = (left[left[idx]] < 0) & (left[right[idx]] < 0)
            prune = idx[leafy & (gain[idx] < gam[idx])]
            if prune.size == 0:
                break
            left[prune] = -1
            right[prune] = -1
            feat[prune] = -1
    # BFS renumbering per tree (drops pruned descendants); nodes of a tree are created in BFS order
    # already, so a stable filter of reachable nodes preserves it.
    reach = np.zeros(n, bool)
    T = len(jobs)
    roots = np.arange(T, dtype=np.int64)          # roots were created first, one per job
    reach[roots] = True
    # propagate reachability one tree level per vectorized pass (children are created after parents)
    internal = np.nonzero(left >= 0)[0]
    while internal.size:
        hit = internal[reach[internal]]
        fresh = hit[~(reach[left[hit]] & reach[right[hit]])]
        if fresh.size == 0:
            break
        reach[left[fresh]] = True
        reach[right[fresh]] = True
    keep = np.nonzero(reach)[0]
    # group by tree, keeping creation order inside a tree
    order = keep[np.argsort(tree[keep], kind="stable")]
    new_id = np.full(n, -1, np.int64)
    new_id[order] = np.arange(order.size)
    tree_off = np.zeros(T + 1, np.int64)
    tree_off[1:] = np.cumsum(np.bincount(tree[order], minlength=T))
    isint = left[order] >= 0
    nodes = np.zeros((order.size, 4), np.int32)
    nodes[:, 0] = np.where(isint, feat[order], 0)
    nodes[:, 1] = np.where(isint, G.bin[:n][order], 0)
    nodes[:, 2] = np.where(isint, new_id[np.maximum(left[order], 0)], -1)
    nodes[:, 3] = np.where(isint, new_id[np.maximum(right[order], 0)], -1)
    gid_value = None
    if with_gid_values:
        # leaf output per created node id: pruned descendants inherit their kept ancestor's leaf value
        parent = np.full(n, -1, np.int64)
        orig_int = np.nonzero(G.left[:n] >= 0)[0]
        parent[G.left[:n][orig_int]] = orig_int
        parent[G.right[:n][orig_int]] = orig_int
        gid_value = value.astype(np.float32).reshape(n, K).copy()
        resolved = reach.copy()
        un = np.nonzero(~reach)[0]
        while un.size:      # one level below the resolved frontier per pass
            cand = un[resolved[parent[un]]]
            if cand.size == 0:
                break
            gid_value[cand] = gid_value[parent[cand]]
            resolved[cand] = True
            un = un[~resolved[un]]
    f = Forest(tree_off, nodes, np.where(isint, G.dl[:n][order], 0).astype(np.uint8),
                  value[order].astype(np.float32).reshape(order.size, K),
                  np.where(isint, gain[order], 0).astype(np.float32), cover[order].astype(np.float32),
                  np.array([j.model for j in jobs], np.int32), missing_bin)
    if with_gid_values:
        f._gid_value, f._gid_tree = gid_value, tree.astype(np.int64)
    return f


_PM_VK = N.ABI_CONSTS["TMOG_PM_VK"]      # forest_predict_kernels.hip forest_predict_multi_kernel: variants x classes per model
_PM_DEPTHS = 32                          # ... and its s_dmask: per-depth stop masks for depths 0.._PM_DEPTHS


def _pm_lds_bytes(F: int) -> int:
    """The bytes ``tmog_hip_forest_predict_multi`` holds against the LDS limit: 64 staged rows of F bins + 64 x 4 x 32
    fp32 sums + the kernel's static depth table. The kernel keeps its sums in registers and needs less; the figure
    stays as the entry's refusal and as the width from which ``forest_predict_multi`` scores variant by variant."""
    return ((64 * F + 15) & ~15) + 4 * _PM_VK * 64 * 4 + 4 * (_PM_DEPTHS + 1)


def _node_depth(f: Forest) -> np.ndarray:
    """Depth of every node (roots 0), level by level over all trees at once."""
    depth = np.zeros(len(f.nodes), np.int32)
    frontier = f.tree_off[:-1].astype(np.int64)
    frontier = frontier[frontier < f.tree_off[1:]]
    d = 0
    while frontier.size:
        depth[frontier] = d
        kids = f.nodes[frontier, 2:4].astype(np.int64)
        frontier = kids[kids[:, 0] >= 0].ravel()
        d += 1
    return depth


def _lds_limit(dev) -> int:
    """LDS one workgroup may allocate (gfx950: 160 KB; the launcher refuses more with -3)."""
    return 160 * 1024


def predict_v1() -> bool:
    """``TMOG_PREDICT_V1=1`` selects the direct node source: the scoring kernels read ``nodes`` / ``default_left`` /
    ``node_mask`` instead of the packed node image (the A/B switch; read once per process by the native library)."""
    return bool(N.hip().tmog_hip_predict_v1())


def pack_node_image(nodes: np.ndarray, default_left: np.ndarray, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """uint32 ``[n, 4]``: the record ``forest_image_kernel`` (forest_predict_kernels.hip) packs for every node,
    ``(feat | bin << 16 | default_left << 24, variant stop mask, left, right)``: its host twin."""
    nd = np.asarray(nodes, np.int32).reshape(-1, 4)
    img = np.zeros((len(nd), 4), np.uint32)
    img[:, 0] = (nd[:, 0].astype(np.uint32) | (nd[:, 1].astype(np.uint32) << np.uint32(16))
                 | ((np.asarray(default_left) != 0).astype(np.uint32) << np.uint32(24)))
    if mask is not None:
        img[:, 1] = np.asarray(mask, np.uint32)
    img[:, 2:] = nd[:, 2:].view(np.uint32)
    return img


def image_fits(forest: Forest) -> bool:
    """A node record holds 16 bits of feature index and 8 bits of split bin."""
    nd = forest.nodes
    return len(nd) == 0 or (int(nd[:, 0].min()) >= 0 and int(nd[:, 0].max()) < 65536
                            and int(nd[:, 1].min()) >= 0 and int(nd[:, 1].max()) < 256)


def _scoring_image(forest: Forest, dev, mask_key=None, make_mask=None) -> Optional[torch.Tensor]:
    """The forest's node image on ``dev`` (int32 ``[n, 4]``), or None when the forest does not fit one (the caller
    then scores from the direct node source). Built by ``forest_image_kernel`` and kept on the forest object, per
    stream like the other device caches here: a fitted model scores every later batch from the same image. It is
    rebuilt when ``nodes`` or ``default_left`` (or, with variant masks, ``gain`` or the variants: ``mask_key``) is
    another object than the one it was built from; arrays edited in place are not noticed. ``make_mask()`` gives
    the uint32 stop mask per node; without it the mask words are 0."""
    cache = forest.__dict__.setdefault("_images", {})
    slot = ("plain" if make_mask is None else "multi", str(dev), _stream_key(dev))
    e = cache.get(slot)
    src = (forest.nodes, forest.default_left, None if make_mask is None else forest.gain)
    if e is not None and all(a is b for a, b in zip(e[0], src)) and e[1] == mask_key:
        return e[2]
    image = None
    if image_fits(forest):
        pk = _Pack(dev)
        ids = [pk.add(np.ascontiguousarray(forest.nodes)), pk.add(forest.default_left)]
        if make_mask is not None:
            ids.append(pk.add(make_mask().view(np.int32)))
        dv = pk.ship()
        image = torch.empty((len(forest.nodes), 4), dtype=torch.int32, device=dev)
        N.check(N.hip().tmog_hip_forest_image(
            N.ptr(dv[ids[0]]), N.ptr(dv[ids[1]]), N.ptr(dv[ids[2]]) if make_mask is not None else None,
            len(forest.nodes), N.ptr(image), N.stream(dev)), "forest_image")
    if len(cache) >= 8:
        cache.clear()
    cache[slot] = (src, mask_key, image)
    return image


def _batch_tables(Nrows: int, model_rows, model_trees):
    """What a scoring call ships besides the forest: the trees reordered so that each model's are contiguous
    (``order``, their offsets ``mto``) and each model's row count (``counts``, their offsets ``mro``)."""
    order = [t for ts in model_trees for t in ts]
    mto = np.zeros(len(model_trees) + 1, np.int64)
    mto[1:] = np.cumsum([len(ts) for ts in model_trees])
    counts = [Nrows if r is None else int(r.numel()) for r in model_rows]
    mro = np.zeros(len(model_rows) + 1, np.int64)
    mro[1:] = np.cumsum(counts)
    return order, mto, counts, mro


def _row_list(Nrows: int, model_rows, dev) -> torch.Tensor:
    """The models' row ids back to back (int32), all rows for a model without a list."""
    every = torch.arange(Nrows, device=dev, dtype=torch.int32) if any(r is None for r in model_rows) else None
    return torch.cat([every if r is None else r.to(dev).to(torch.int32) for r in model_rows])


def forest_predict_multi(forest: Forest, Xb: torch.Tensor, model_rows: Sequence[Optional[torch.Tensor]],
                         model_trees: Sequence[Sequence[int]],
                         model_variants: Sequence[Sequence[Tuple[int, float]]]) -> List[List[torch.Tensor]]:
    """Predictions of pruned variants of shared trees: model m's trees are grown trees and each of its
    variants ``(max_depth, min_info_gain)`` is the forest ``prune_forest(trees, max_depth, min_info_gain)``
    would give. On the GPU every (row, tree) is walked once for all of a model's variants
    (``forest_predict_multi_kernel``); elsewhere (or for class counts the kernel does not take) each
    variant is pruned and predicted on its own. Returns ``[model][variant] -> float32 [n_m, K]``."""
    dev = Xb.device
    K = forest.K
    F = int(Xb.shape[1]) if Xb.dim() == 2 else 0
    if dev.type != "cuda" or K not in (1, 2, 4, 8) or any(len(v) * K > _PM_VK or len(v) > 32
                                                         for v in model_variants) \
            or _pm_lds_bytes(F) > _lds_limit(dev):
        res = []
        for rows, ts, vs in zip(model_rows, model_trees, model_variants):
            sub = Forest.concat([forest.tree(int(t)) for t in ts])
            res.append([forest_predict(prune_forest(sub, d, g), Xb, [rows], [list(range(sub.n_trees))])[0]
                        for d, g in vs])
        return res
    Xb = Xb.contiguous()
    Nrows, F = int(Xb.shape[0]), int(Xb.shape[1])
    order, mto, counts, mro = _batch_tables(Nrows, model_rows, model_trees)
    voff = np.zeros(len(model_variants) + 1, np.int32)
    voff[1:] = np.cumsum([len(v) for v in model_variants])
    vdep = np.asarray([d for vs in model_variants for d, _ in vs], np.int32)
    vout = np.zeros(max(1, int(voff[-1])), np.int64)
    pos = 0
    for m, vs in enumerate(model_variants):
        for k in range(len(vs)):
            vout[int(voff[m]) + k] = pos
            pos += counts[m] * K
    # per-node variant stop bits of the depth-independent part of prune_forest's rule: a grown leaf stops
    # every variant, an internal node those whose min gain exceeds its split gain (fp32 compare)
    # The kernel's depth table ends at _PM_DEPTHS: a deeper max depth is folded into the node bits here (a tree
    # deeper than that variant would otherwise be walked to its grown leaves)
    def make_mask() -> np.ndarray:
        mask = np.zeros(len(forest.nodes), np.uint32)
        leaf = forest.nodes[:, 2] < 0
        depth = _node_depth(forest) if any(d > _PM_DEPTHS for vs in model_variants for d, _ in vs) else None
        for m, vs in enumerate(model_variants):
            sel = np.zeros(len(forest.nodes), bool)
            for t in model_trees[m]:
                sel[int(forest.tree_off[t]):int(forest.tree_off[t + 1])] = True
            bits = np.zeros(len(forest.nodes), np.uint32)
            for k, (d, g) in enumerate(vs):
                stop = (forest.gain < np.float32(g)) | leaf
                if d > _PM_DEPTHS:
                    stop |= depth >= d
                bits |= stop.astype(np.uint32) << np.uint32(k)
            mask[sel] = bits[sel]
        return mask

    # the node image carries the mask words: one per (trees, variants) of the call, kept for the next such call
    image = None if predict_v1() else _scoring_image(
        forest, dev, (tuple(tuple(int(t) for t in ts) for ts in model_trees),
                      tuple(tuple((int(d), float(g)) for d, g in vs) for vs in model_variants)), make_mask)
    pk = _Pack(dev)
    ids = [pk.add(forest.tree_off[:-1][order].astype(np.int64)), pk.add(np.ones(len(order), np.float32)),
           pk.add(np.ascontiguousarray(forest.value, np.float32))]
    if image is None:
        ids += [pk.add(np.ascontiguousarray(forest.nodes)), pk.add(forest.default_left),
                pk.add(make_mask().view(np.int32))]
    i_v = [pk.add(voff), pk.add(vdep), pk.add(vout), pk.add(mro), pk.add(mto)]
    row_list = _row_list(Nrows, model_rows, dev)
    dv = pk.ship()
    t_off, t_w, lv = (dv[i] for i in ids[:3])
    voff_t, vdep_t, vout_t, mro_t, mto_t = (dv[i] for i in i_v)
    out = torch.empty(max(pos, 1), dtype=torch.float32, device=dev)
    # the two entries differ in how the nodes arrive and in what follows the class count
    if image is not None:
        name, entry, node_args = "forest_predict_multi_image", N.hip().tmog_hip_forest_predict_multi_image, (N.ptr(image),)
        tail = (N.ptr(voff_t), N.ptr(vdep_t), N.ptr(vout_t), max((len(v) for v in model_variants), default=0))
    else:
        nodes, dl, gn = (dv[i] for i in ids[3:])
        name, entry, node_args = "forest_predict_multi", N.hip().tmog_hip_forest_predict_multi, (N.ptr(nodes), N.ptr(dl))
        tail = (N.ptr(gn), N.ptr(voff_t), N.ptr(vdep_t), N.ptr(vout_t))
    N.check(entry(
        N.ptr(Xb), F, len(model_rows), N.ptr(mro_t), N.ptr(row_list), max(counts) if counts else 0,
        N.ptr(mto_t), N.ptr(t_off), N.ptr(t_w), *node_args, forest.missing_bin, N.ptr(lv), K, *tail, N.ptr(out),
        N.stream(dev)), name)
    res = []
    for m, vs in enumerate(model_variants):
        res.append([out[int(vout[int(voff[m]) + k]):int(vout[int(voff[m]) + k]) + counts[m] * K].view(counts[m], K)
                    for k in range(len(vs))])
    return res


def forest_predict(forest: Forest, Xb: torch.Tensor, model_rows: Sequence[Optional[torch.Tensor]],
                   model_trees: Sequence[Sequence[int]], tree_weight: Optional[np.ndarray] = None,
                   n_rows: Optional[int] = None) -> List[torch.Tensor]:
    """Evaluate groups of trees ("models") on row subsets of ``Xb``.

    ``model_rows[m]`` = row ids (or None for all rows); ``model_trees[m]`` = tree indices of the
    forest that form model m. Returns one ``float32 [n_m, K]`` tensor per model: the weighted sum
    of leaf values over the model's trees.
    """
    dev = Xb.device
    Xb = Xb.contiguous()
    Nrows, F = int(Xb.shape[0]), int(Xb.shape[1])
    K = forest.K
    order, mto, counts, mro = _batch_tables(Nrows, model_rows, model_trees)
    tw = np.ones(forest.n_trees, np.float32) if tree_weight is None else np.asarray(tree_weight, np.float32)
    image = None if dev.type != "cuda" or predict_v1() else _scoring_image(forest, dev)
    pk = _Pack(dev)
    ids = [pk.add(forest.tree_off[:-1][order].astype(np.int64)), pk.add(tw[order]),
           pk.add(np.ascontiguousarray(forest.value, np.float32))]
    if image is None:
        ids += [pk.add(np.ascontiguousarray(forest.nodes)), pk.add(forest.default_left)]
    # a single all-rows model needs no list: the kernels compute the row from the block
    single = len(model_rows) <= 1 and all(r is None for r in model_rows)
    row_list = None if single else _row_list(Nrows, model_rows, dev)
    i_mro, i_mto = pk.add(mro), pk.add(mto)
    dv = pk.ship()
    t_off, t_w, lv = (dv[i] for i in ids[:3])
    nodes, dl = (dv[i] for i in ids[3:]) if image is None else (None, None)
    mro_t, mto_t = dv[i_mro], dv[i_mto]
    out = torch.zeros(int(mro[-1]), K, dtype=torch.float32, device=dev)
    if dev.type == "cuda":
        if image is not None:
            name, entry, node_args = "forest_predict_image", N.hip().tmog_hip_forest_predict_image, (N.ptr(image),)
        else:
            name, entry, node_args = "forest_predict", N.hip().tmog_hip_forest_predict, (N.ptr(nodes), N.ptr(dl))
        # the kernel accumulates up to 8 outputs per row in registers: wider K runs in class chunks
        for c0 in range(0, K, 8):
            kc = min(8, K - c0)
            lvc = lv if kc == K else lv[:, c0:c0 + kc].contiguous()
            oc = out if kc == K else torch.empty(int(mro[-1]), kc, dtype=torch.float32, device=dev)
            N.check(entry(
                N.ptr(Xb), F, len(model_rows), N.ptr(mro_t), N.ptr(row_list), max(counts) if counts else 0,
                N.ptr(mto_t), N.ptr(t_off), N.ptr(t_w), *node_args, forest.missing_bin, N.ptr(lvc), kc, N.ptr(oc),
                N.stream(dev)), name)
            if kc != K:
                out[:, c0:c0 + kc] = oc
    else:
        N.check(N.host().tmog_forest_predict_cpu(
            N.ptr(Xb), F, len(model_rows), N.ptr(mro_t), N.ptr(row_list), N.ptr(mto_t), N.ptr(t_off), N.ptr(t_w),
            N.ptr(nodes), N.ptr(dl), forest.missing_bin, N.ptr(lv), K, N.ptr(out)), "forest_predict_cpu")
    return [out[int(mro[m]):int(mro[m + 1])] for m in range(len(model_rows))]


# --------------------------------------------------------------------------------- staged evaluation
EVAL_STAGES = 16            # stages per launch: bounds the aupr tables (16 x 2 x 65536 x 4 B = 8 MiB)
EVAL_BINS = 1 << 16         # score bins of the aupr tables (the boosting epilogue's AUC_BINS)
EVAL_BLOCK = N.ABI_CONSTS["TMOG_EVAL_BLOCK"]
# metric name -> (native code, how the per-stage sum / count / table becomes the value the user reads)
_EVAL_METRICS = {"logloss": ("TMOG_EVAL_LOGLOSS", "mean"), "error": ("TMOG_EVAL_ERROR", "mean"),
                 "aucpr": ("TMOG_EVAL_AUPR", "aupr"), "rmse": ("TMOG_EVAL_SQERR", "rmse"),
                 "mse": ("TMOG_EVAL_SQERR", "mean"), "mae": ("TMOG_EVAL_ABSERR", "mean"),
                 "mlogloss": ("TMOG_EVAL_MLOGLOSS", "mean"), "merror": ("TMOG_EVAL_MERROR", "mean")}
EVAL_MAXIMISED = ("aucpr",)


def forest_staged_eval_raw(forest: Forest, Xb: torch.Tensor, rows: Optional[torch.Tensor], y: torch.Tensor, *,
                           stage_off, tree_col=None, K: int = 1, tree_weight=None, metric: str,
                           margin_scale: float = 1.0, margins: Optional[torch.Tensor] = None, base=0.0):
    """What the staged evaluation accumulates, before :func:`forest_staged_eval` finishes it: ``(raw, margins)`` with
    ``raw`` the per-stage floating sums (float64 ``[S]``), error counts (int64 ``[S]``) or aupr count tables (int32
    ``[S, 2, EVAL_BINS]``), on the device of ``Xb``."""
    if metric not in _EVAL_METRICS:
        raise ValueError(f"unknown staged evaluation metric {metric!r} (one of {sorted(_EVAL_METRICS)})")
    code = N.ABI_CONSTS[_EVAL_METRICS[metric][0]]
    multi = metric in ("mlogloss", "merror")
    K = int(K)
    if K < 1 or (K != 1 and not multi):
        raise ValueError(f"metric {metric} takes one margin per row, got K = {K}")
    dev = Xb.device
    Xb = Xb.contiguous()
    Nrows, F = int(Xb.shape[0]), int(Xb.shape[1])
    T = forest.n_trees
    so = np.asarray(stage_off, np.int64).reshape(-1)
    if so.size < 1 or so[0] < 0 or so[-1] > T or (np.diff(so) < 0).any():
        raise ValueError("stage_off must be non-decreasing tree indices within the forest")
    S = int(so.size) - 1
    tc = np.zeros(T, np.int32) if tree_col is None else np.asarray(tree_col, np.int32).reshape(-1)
    if tc.shape[0] != T or (T and (tc.min() < 0 or tc.max() >= K)):
        raise ValueError("tree_col must give every tree a column in [0, K)")
    tw = np.ones(T, np.float32) if tree_weight is None else np.asarray(tree_weight, np.float32).reshape(-1)
    if tw.shape[0] != T:
        raise ValueError("tree_weight must have one entry per tree")
    if forest.value.shape[1] != 1:
        raise ValueError("staged evaluation takes trees with one value per node")
    toff = np.asarray(forest.tree_off, np.int64)
    if T and (toff[0] < 0 or toff[-1] > len(forest.nodes) or (np.diff(toff) < 1).any()):
        raise ValueError("forest tree offsets out of range")
    row_list = None
    n = Nrows
    if rows is not None:
        row_list = rows.to(dev).to(torch.int32).contiguous()
        n = int(row_list.numel())
        if n and (int(row_list.min()) < 0 or int(row_list.max()) >= Nrows):
            raise ValueError("row ids out of range")
    yf = y.to(dev).to(torch.float32).contiguous()
    if yf.numel() < Nrows:
        raise ValueError("y must hold a label for every row of Xb")
    if margins is None:
        margins = torch.zeros(n, K, dtype=torch.float64, device=dev) + torch.as_tensor(
            np.asarray(base, np.float64), device=dev)
    else:
        margins = margins.to(torch.float64).reshape(n, K).contiguous()
    bins = EVAL_BINS
    if metric == "aucpr":
        raw = torch.zeros(S, 2, bins, dtype=torch.int32, device=dev)
    elif metric in ("error", "merror"):
        raw = torch.zeros(S, dtype=torch.int64, device=dev)
    else:
        raw = torch.zeros(S, dtype=torch.float64, device=dev)
    if n == 0 or S == 0:
        return raw, margins
    pk = _Pack(dev)
    for a in (toff[:-1], tw, np.ascontiguousarray(forest.nodes), forest.default_left,
              np.ascontiguousarray(forest.value[:, 0], np.float32), so, tc):
        pk.add(a)
    t_off, t_w, nodes, dl, lv, so_t, tc_t = pk.ship()
    on_gpu = dev.type == "cuda"
    nblk = (n + EVAL_BLOCK - 1) // EVAL_BLOCK
    slab = torch.empty(nblk * min(S, EVAL_STAGES), dtype=torch.float64, device=dev) \
        if on_gpu and raw.dtype == torch.float64 else None
    for s0 in range(0, S, EVAL_STAGES):
        sc = min(EVAL_STAGES, S - s0)
        part = raw[s0:s0 + sc]
        args = (N.ptr(Xb), F, N.ptr(row_list), n, N.ptr(yf), N.ptr(nodes), N.ptr(dl), N.ptr(lv), N.ptr(t_off),
                N.ptr(t_w), int(forest.missing_bin), N.ptr(so_t[s0:]), sc, N.ptr(tc_t), K, code, float(margin_scale),
                bins, N.ptr(margins), N.ptr(part) if raw.dtype == torch.float64 else None,
                N.ptr(part) if raw.dtype == torch.int64 else None, N.ptr(part) if raw.dtype == torch.int32 else None)
        if on_gpu:
            N.check(N.hip().tmog_hip_forest_staged_eval(*args, N.ptr(slab), N.stream(dev)), "forest_staged_eval")
        else:
            N.check(N.host().tmog_forest_staged_eval_cpu(*args), "forest_staged_eval_cpu")
    return raw, margins


def staged_eval_finish(raw: torch.Tensor, n: int, metric: str) -> np.ndarray:
    """The metric values (float64 ``[S]``, as the user reads them) of :func:`forest_staged_eval_raw`'s ``raw``."""
    how = _EVAL_METRICS[metric][1]
    if how == "aupr":
        from ..evaluators.metrics import binned_aupr_from_counts
        return binned_aupr_from_counts(raw).cpu().numpy().astype(np.float64)
    v = raw.cpu().numpy().astype(np.float64) / max(n, 1)
    return np.sqrt(v) if how == "rmse" else v


def forest_staged_eval(forest: Forest, Xb: torch.Tensor, rows: Optional[torch.Tensor], y: torch.Tensor, *,
                       stage_off, tree_col=None, K: int = 1, tree_weight=None, metric: str,
                       margin_scale: float = 1.0, margins: Optional[torch.Tensor] = None, base=0.0):
    """The metric of a boosted model after each of its stages, in one pass over the trees.

    Stage ``s`` is the trees ``stage_off[s]..stage_off[s + 1]`` of ``forest``; tree ``t`` adds ``tree_weight[t]`` times
    its leaf value to column ``tree_col[t]`` of the rows' fp64 margins (``[n, K]``, started at ``base`` or at
    ``margins``, the margins an earlier call returned). ``rows`` are row ids into ``Xb`` (None: every row), ``y`` the
    labels by row id. ``metric``: ``logloss`` / ``error`` / ``aucpr`` of the probability ``1 / (1 + exp(-margin_scale
    * margin))``, ``rmse`` / ``mse`` / ``mae``, or ``mlogloss`` / ``merror`` over K margins. Returns ``(values, margins)``:
    the metric after each stage (numpy float64 ``[S]``) and the margins after the last one. At most ``EVAL_STAGES``
    stages go into one launch. CUDA tensors run ``staged_eval_kernel``, others the host twin."""
    raw, margins = forest_staged_eval_raw(forest, Xb, rows, y, stage_off=stage_off, tree_col=tree_col, K=K,
                                          tree_weight=tree_weight, metric=metric, margin_scale=margin_scale,
                                          margins=margins, base=base)
    return staged_eval_finish(raw, int(margins.shape[0]), metric), margins


# ------------------------------------------------------------- forest explanations: what the four engines share
def _pow2_scale(S: float, bits: int) -> float:
    """The power of two with ``S * scale < 2^bits`` (1.0 for a forest without magnitude): the kernels' fixed point."""
    if not (S > 0 and math.isfinite(S)):
        return 1.0
    return 2.0 ** max(-1000, min(1000, bits - math.frexp(S)[1]))


def _split_columns(forest: Forest) -> Tuple[np.ndarray, np.ndarray]:
    """``(internal, used)``: which nodes split, and the distinct columns they split on, sorted (int32)."""
    internal = forest.nodes[:, 2] >= 0
    return internal, np.unique(forest.nodes[internal, 0]).astype(np.int32)


def _columns_needed(forest: Forest, tout: np.ndarray) -> int:
    """The output columns the trees write: tree ``t`` fills ``tout[t] .. tout[t] + K - 1``."""
    return (int(tout.max()) if forest.n_trees else 0) + forest.K


def _magnitude_bound(forest: Forest, tw: np.ndarray, value: np.ndarray) -> float:
    """``S = sum_t |w_t| max_node |value_t|`` in the precision of the caller's weights and values."""
    S = 0.0
    for t in range(forest.n_trees):
        a, b = int(forest.tree_off[t]), int(forest.tree_off[t + 1])
        if b > a and value[a:b].size:
            S += abs(float(tw[t])) * float(np.abs(value[a:b]).max())
    return float(S)


class _Resident:
    """The arrays ``_shipped`` names, resident on a device (shipped once per device)."""
    _shipped: Tuple[str, ...] = ()

    def on(self, dev):
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(getattr(self, a))).to(dev)
                                   for a in self._shipped)
        return self._dev[key]


def _explain_rows(plan, Xb: torch.Tensor, rows: Optional[torch.Tensor], n_out: Optional[int]):
    """What every explanation engine derives first: ``(Xb contiguous, Nrows, F, C output columns, row_list int32 on
    the matrix's device or None, n rows served, the plan's used columns as int64)``."""
    C = int(n_out) if n_out is not None else plan.n_out
    if C < plan.n_out:
        raise ValueError(f"n_out = {C} but the trees write {plan.n_out} columns")
    Xb = Xb.contiguous()
    Nrows, F = int(Xb.shape[0]), int(Xb.shape[1])
    if plan.used.size and int(plan.used[-1]) >= F:
        raise ValueError(f"the forest splits on column {int(plan.used[-1])}, the matrix has {F}")
    row_list = None if rows is None else rows.to(Xb.device).to(torch.int32).contiguous()
    n = Nrows if rows is None else int(row_list.numel())
    return Xb, Nrows, F, C, row_list, n, plan.used.astype(np.int64)


def _on_host_twin(Xb: torch.Tensor, row_list: Optional[torch.Tensor], run) -> torch.Tensor:
    """The answer for a launch the device entry refused: ``run`` on the CPU copy of the rows, moved back."""
    sub = Xb if row_list is None else Xb.index_select(0, row_list.to(torch.long))
    return run(sub.cpu()).to(Xb.device)


# ------------------------------------------------------------------------------------------ TreeSHAP
@dataclass
class ForestPaths(_Resident):
    """One merged path per leaf (:func:`forest_paths`), ordered by length bin (m <= 16, <= 32, <= 64, longer),
    then by tree. Element arrays are indexed ``p_off[p] .. p_off[p + 1]``."""
    used: np.ndarray                # int32 [U]   distinct split features, sorted
    p_off: np.ndarray               # int64 [P+1] element offsets
    p_out: np.ndarray               # int32 [P]   first output column of the path
    p_val: np.ndarray               # float64 [P, KV]  leaf value x tree weight
    bias: np.ndarray                # float64 [n_out]  sum over paths of value x product of zero fractions
    e_feat: np.ndarray              # int32 [E]   compact used-feature index
    e_rng: np.ndarray               # int32 [E]   lo | hi << 12 | (missing bin satisfies) << 24
    e_z: np.ndarray                 # float64 [E] zero fraction
    bin_off: np.ndarray             # int64 [4]   path index bounds of the three kernel length bins
    n_out: int                      # output columns the paths need
    S: float                        # sum_t |w_t| max_node |value_t|: the attribution's magnitude bound
    missing_bin: int = -1
    _dev: dict = field(default_factory=dict, repr=False)
    _shipped = ("used", "p_off", "p_out", "p_val", "e_feat", "e_rng", "e_z")

    @property
    def scale(self) -> float:
        """``S * scale < 2^62``: a row's partial sums stay below ``2 S`` (``ops/csrc/hip/shap_kernels.hip``)."""
        return _pow2_scale(self.S, 62)


def forest_paths(forest: Forest, tree_weight: Optional[np.ndarray] = None,
                 tree_out: Optional[np.ndarray] = None) -> ForestPaths:
    """Unroll a forest into the leaf paths exact TreeSHAP works on. A feature that repeats on a path is merged
    into one element: a row satisfies it iff it satisfies every merged node, i.e. its bin lies in the
    intersection ``[lo, hi]`` of the nodes' ranges, or it is the missing bin and every merged node sends
    missing rows along the path; the element's zero fraction is the product of the merged nodes' cover
    ratios ``cover[child] / cover[node]`` (0 where ``cover[node] == 0``). A path carries its leaf's value
    vector times the tree weight and the output column ``tree_out[t]`` (default 0) its first value goes to."""
    T = forest.n_trees
    KV = forest.K
    tw = np.ones(T, np.float64) if tree_weight is None else np.asarray(tree_weight, np.float64)
    tout = np.zeros(T, np.int32) if tree_out is None else np.asarray(tree_out, np.int32)
    nd = forest.nodes
    used = _split_columns(forest)[1]
    cover = forest.cover.astype(np.float64)
    value = forest.value.astype(np.float64)
    dl = forest.default_left
    paths = []                       # (m, tree, feats, los, his, miss, zs, leaf)
    for t in range(T):
        a, b = int(forest.tree_off[t]), int(forest.tree_off[t + 1])
        if b <= a:
            continue
        stack = [(a, ())]            # (node, elements: tuple of (feat, lo, hi, miss_ok, z) in order of first use)
        while stack:
            k, els = stack.pop()
            f, sb, lc, rc = (int(v) for v in nd[k])
            if lc < 0:
                paths.append((len(els), t, els, k))
                continue
            ck = cover[k]
            for child, left in ((rc, False), (lc, True)):
                ratio = cover[child] / ck if ck != 0 else 0.0
                lo, hi = (0, sb) if left else (sb + 1, 4095)
                ok = bool(dl[k]) == left
                for i, (ef, elo, ehi, eok, ez) in enumerate(els):
                    if ef == f:
                        ne = els[:i] + ((f, max(elo, lo), min(ehi, hi), eok and ok, ez * ratio),) + els[i + 1:]
                        break
                else:
                    ne = els + ((f, lo, hi, ok, ratio),)
                stack.append((child, ne))
    lens = np.asarray([p[0] for p in paths], np.int64)
    bins = np.searchsorted(np.asarray([16, 32, 64]), lens, side="left")
    order = np.argsort(bins, kind="stable")                    # within a bin: tree order, as generated
    P = len(paths)
    p_off = np.zeros(P + 1, np.int64)
    p_off[1:] = np.cumsum(lens[order])
    E = int(p_off[-1])
    p_out = np.zeros(P, np.int32)
    p_val = np.zeros((P, KV), np.float64)
    p_zprod = np.ones(P, np.float64)
    e_feat = np.zeros(E, np.int32)
    e_rng = np.zeros(E, np.int32)
    e_z = np.zeros(E, np.float64)
    for i, j in enumerate(order):
        m, t, els, leaf = paths[j]
        p_out[i] = tout[t]
        p_val[i] = value[leaf] * tw[t]
        o = int(p_off[i])
        for e, (f, lo, hi, ok, z) in enumerate(els):
            if lo > hi:
                lo, hi = 1, 0                                  # contradictory repeats: no bin satisfies
            e_feat[o + e] = f
            e_rng[o + e] = lo | (hi << 12) | (int(ok) << 24)
            e_z[o + e] = z
            p_zprod[i] *= z
    e_feat = np.searchsorted(used, e_feat).astype(np.int32)
    sb = bins[order]
    bin_off = np.asarray([0, np.sum(sb <= 0), np.sum(sb <= 1), np.sum(sb <= 2)], np.int64)
    n_out = _columns_needed(forest, tout)
    bias = np.zeros(n_out, np.float64)
    for c in range(KV):
        np.add.at(bias, p_out + c, p_val[:, c] * p_zprod)
    return ForestPaths(used, p_off, p_out, p_val, bias, e_feat, e_rng, e_z, bin_off, n_out,
                       _magnitude_bound(forest, tw, value), int(forest.missing_bin))


def forest_shap(forest: Forest, Xb: torch.Tensor, rows: Optional[torch.Tensor] = None,
                tree_weight: Optional[np.ndarray] = None, tree_out: Optional[np.ndarray] = None,
                n_out: Optional[int] = None, paths: Optional[ForestPaths] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """Exact path-dependent TreeSHAP of the forest's ``tree_weight``-weighted leaf-value sum on rows ``rows``
    (None = all) of the binned matrix: ``(phi float64 [n, U + 1, C], used_features int64 [U])``. Slot ``u < U``
    is the attribution of column ``used_features[u]``, slot ``U`` the bias; tree ``t``'s ``K`` leaf values go to
    columns ``tree_out[t] .. tree_out[t] + K - 1`` of ``C = n_out`` (default: as many as the trees need), and
    ``phi.sum(1)`` equals the forest's prediction. Device matrices run ``tmog_hip_forest_shap``; paths longer
    than 64 elements or a tile beyond the LDS limit, and host matrices, run the host twin. ``paths``: the
    prepared :func:`forest_paths` of the same forest / weights / columns (callers cache them)."""
    fp = paths if paths is not None else forest_paths(forest, tree_weight, tree_out)
    dev = Xb.device
    Xb, _, F, C, row_list, n, used64 = _explain_rows(fp, Xb, rows, n_out)
    U, P, KV = int(fp.used.size), int(fp.p_out.size), int(fp.p_val.shape[1])
    out = torch.empty(n, U + 1, C, dtype=torch.float64, device=dev)
    bo = fp.bin_off
    bias = np.zeros(C, np.float64)
    bias[:fp.n_out] = fp.bias
    if dev.type == "cuda":
        d = fp.on(dev)
        bias_d = torch.from_numpy(bias).to(dev)
        rc = N.hip().tmog_hip_forest_shap(
            N.ptr(Xb), F, n, N.ptr(row_list), U, N.ptr(d[0]), P, N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]), KV,
            N.ptr(bias_d), N.ptr(d[4]), N.ptr(d[5]), N.ptr(d[6]), bo.ctypes.data, fp.missing_bin, C, fp.scale,
            N.ptr(out), N.stream(dev))
        if rc in (-2, -3):           # a path longer than 64 elements / one row's tile beyond the LDS limit
            return _on_host_twin(Xb, row_list, lambda sub: forest_shap(forest, sub, None, n_out=C, paths=fp)[0]), used64
        N.check(rc, "forest_shap")
        return out, used64
    N.check(N.host().tmog_forest_shap_cpu(
        N.ptr(Xb), F, n, N.ptr(row_list), U, fp.used.ctypes.data, P, fp.p_off.ctypes.data, fp.p_out.ctypes.data,
        fp.p_val.ctypes.data, KV, bias.ctypes.data, fp.e_feat.ctypes.data, fp.e_rng.ctypes.data,
        fp.e_z.ctypes.data, bo.ctypes.data, fp.missing_bin, C, fp.scale, N.ptr(out)), "forest_shap_cpu")
    return out, used64


def forest_shap_interactions(forest: Forest, Xb: torch.Tensor, rows: Optional[torch.Tensor] = None,
                             tree_weight: Optional[np.ndarray] = None, tree_out: Optional[np.ndarray] = None,
                             n_out: Optional[int] = None,
                             paths: Optional[ForestPaths] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """Exact SHAP interaction values of the score :func:`forest_shap` attributes (same arguments):
    ``(Phi float64 [n, U + 1, U + 1, C], used_features int64 [U])``. ``Phi[:, i, j]`` with ``i != j < U`` is the
    interaction of columns ``used_features[i]`` and ``used_features[j]`` (half the Shapley interaction index, so
    the pair's whole effect is ``Phi[:, i, j] + Phi[:, j, i]``), ``Phi[:, i, i]`` the main effect, ``Phi[:, U, U]``
    the bias and the rest of row and column ``U`` zero. ``Phi`` is exactly symmetric, ``Phi.sum(2)`` is
    :func:`forest_shap`'s ``phi`` and ``Phi.sum((1, 2))`` the forest's prediction.

    Device matrices run ``tmog_hip_forest_shap_interactions``; paths longer than 64 elements or a tile beyond the
    LDS limit, and host matrices, run the host twin. Either fills the pair sums (each unordered pair once); the
    transpose, the diagonal (``phi`` minus the row's pair sums) and the bias are added in torch on the matrix's
    device. Memory: the result takes ``n * (U + 1)^2 * C * 8`` bytes and the pair sums as much again while it
    is put together, so callers block their rows."""
    fp = paths if paths is not None else forest_paths(forest, tree_weight, tree_out)
    dev = Xb.device
    Xb, _, F, C, row_list, n, used64 = _explain_rows(fp, Xb, rows, n_out)
    U, P, KV = int(fp.used.size), int(fp.p_out.size), int(fp.p_val.shape[1])
    tri = torch.empty(n, U, U, C, dtype=torch.float64, device=dev)
    bo = fp.bin_off
    if dev.type == "cuda":
        d = fp.on(dev)
        rc = N.hip().tmog_hip_forest_shap_interactions(
            N.ptr(Xb), F, n, N.ptr(row_list), U, N.ptr(d[0]), P, N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]), KV,
            None, N.ptr(d[4]), N.ptr(d[5]), N.ptr(d[6]), bo.ctypes.data, fp.missing_bin, C, fp.scale,
            N.ptr(tri), N.stream(dev))
        if rc in (-2, -3):           # a path longer than 64 elements / one row x one column beyond the LDS limit
            return _on_host_twin(
                Xb, row_list, lambda sub: forest_shap_interactions(forest, sub, None, n_out=C, paths=fp)[0]), used64
        N.check(rc, "forest_shap_interactions")
    else:
        N.check(N.host().tmog_forest_shap_interactions_cpu(
            N.ptr(Xb), F, n, N.ptr(row_list), U, fp.used.ctypes.data, P, fp.p_off.ctypes.data,
            fp.p_out.ctypes.data, fp.p_val.ctypes.data, KV, None, fp.e_feat.ctypes.data, fp.e_rng.ctypes.data,
            fp.e_z.ctypes.data, bo.ctypes.data, fp.missing_bin, C, fp.scale, N.ptr(tri)),
            "forest_shap_interactions_cpu")
    phi = forest_shap(forest, Xb, row_list, n_out=C, paths=fp)[0]
    Phi = torch.zeros(n, U + 1, U + 1, C, dtype=torch.float64, device=dev)
    off = Phi[:, :U, :U]
    torch.add(tri, tri.transpose(1, 2), out=off)
    del tri
    diag = phi[:, :U] - off.sum(2)
    off.diagonal(dim1=1, dim2=2).copy_(diag.transpose(1, 2))
    Phi[:, U, U] = phi[:, U]
    return Phi, used64


# ------------------------------------------------------------------------------------- path-perturbation LOCO
@dataclass
class ForestLoco(_Resident):
    """What :func:`forest_loco` reads of one forest / weights / output columns (:func:`forest_loco_plan`)."""
    used: np.ndarray                # int32 [U]   distinct split columns, sorted
    nodes: np.ndarray               # int32 [n, 4] (slot u, bin | default_left << 16, left, right), left < 0 => leaf
    tree_off: np.ndarray            # int64 [T + 1]
    value: np.ndarray               # float32 [n, KV]
    tree_weight: np.ndarray         # float32 [T]
    tree_out: np.ndarray            # int32 [T]   first output column of the tree
    n_out: int                      # output columns the trees need
    S: float                        # sum_t |w_t| max_node |value_t|: the magnitude bound of the base sum
    missing_bin: int = -1
    _dev: dict = field(default_factory=dict, repr=False)
    _shipped = ("used", "tree_off", "nodes", "value", "tree_weight", "tree_out")

    @property
    def scale(self) -> float:
        """``S * scale < 2^61``: a delta slot's partial sums stay within ``2 S`` (``ops/csrc/hip/loco_kernels.hip``
        has the bound), so the int64 fixed-point sums cannot overflow."""
        return _pow2_scale(self.S, 61)


def forest_loco_plan(forest: Forest, tree_weight: Optional[np.ndarray] = None,
                     tree_out: Optional[np.ndarray] = None) -> ForestLoco:
    """The node records of :func:`forest_loco`: the forest's nodes with each split column replaced by its index in
    the sorted distinct split columns and the default direction folded into the bin word. Tree weights are taken
    as fp32, as the predictors take them."""
    T = forest.n_trees
    tw = np.ones(T, np.float32) if tree_weight is None else np.ascontiguousarray(tree_weight, np.float32)
    tout = np.zeros(T, np.int32) if tree_out is None else np.ascontiguousarray(tree_out, np.int32)
    if tw.shape != (T,) or tout.shape != (T,):
        raise ValueError("tree_weight / tree_out must have one entry per tree")
    if T and int(tout.min()) < 0:
        raise ValueError("tree_out must not be negative")
    nd = forest.nodes
    internal, used = _split_columns(forest)
    if internal.any() and (int(nd[internal, 1].min()) < 0 or int(nd[internal, 1].max()) > 0xFFFF):
        raise ValueError("split bins must fit 16 bits")
    nodes = np.zeros((len(nd), 4), np.int32)
    nodes[:, 0] = np.where(internal, np.searchsorted(used, nd[:, 0]), 0)
    nodes[:, 1] = np.where(internal, nd[:, 1] | (forest.default_left.astype(np.int32) != 0) << 16, 0)
    nodes[:, 2] = np.where(internal, nd[:, 2], -1)
    nodes[:, 3] = np.where(internal, nd[:, 3], -1)
    value = np.ascontiguousarray(forest.value, np.float32).reshape(len(nd), -1)
    return ForestLoco(used, nodes, np.ascontiguousarray(forest.tree_off, np.int64), value, tw, tout,
                      _columns_needed(forest, tout), _magnitude_bound(forest, tw, value), int(forest.missing_bin))


def forest_loco(forest: Forest, Xb: torch.Tensor, zero_bins, rows: Optional[torch.Tensor] = None,
                groups: Optional[Sequence] = None, tree_weight: Optional[np.ndarray] = None,
                tree_out: Optional[np.ndarray] = None, n_out: Optional[int] = None,
                plan: Optional[ForestLoco] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """Exact leave-one-column-out sums of the forest's ``tree_weight``-weighted leaf-value sum on rows ``rows``
    (None = all) of the binned matrix, by perturbing tree paths instead of rescoring rows:
    ``(out float64 [n, U + G + 1, C], used int64 [U])``. ``zero_bins`` (uint8 ``[F]``) is the bin the value 0.0 falls
    into per column; ``groups`` an optional list of G disjoint arrays of column ids, each zeroed as a whole (members
    the forest does not split on are allowed). Slot ``u < U`` is the sum with column ``used[u]`` replaced by its zero
    bin minus the unperturbed sum (exactly 0.0 when nothing changes), slot ``U + g`` the same with every column of
    group ``g`` replaced at once, the last slot the unperturbed sum. Tree ``t``'s ``K`` leaf values go to columns
    ``tree_out[t] .. tree_out[t] + K - 1`` of ``C = n_out``. Device matrices run ``tmog_hip_forest_loco``; host
    matrices, and a launch whose one-row tile is beyond the LDS limit, run the host twin -- both sum in the same
    int64 fixed point, so they agree bit for bit. ``plan``: the prepared :func:`forest_loco_plan` of the same
    forest / weights / columns (callers cache it)."""
    lp = plan if plan is not None else forest_loco_plan(forest, tree_weight, tree_out)
    if Xb.dtype != torch.uint8 or Xb.dim() != 2:
        raise ValueError("Xb must be a uint8 [N, F] matrix")
    dev = Xb.device
    Xb, _, F, C, row_list, n, used64 = _explain_rows(lp, Xb, rows, n_out)
    zb = zero_bins.cpu().numpy() if isinstance(zero_bins, torch.Tensor) else np.asarray(zero_bins)
    zb = zb.reshape(-1).astype(np.int32)
    if zb.size != F:
        raise ValueError(f"zero_bins has {zb.size} entries, the matrix {F} columns")
    U, T, KV = int(lp.used.size), int(lp.tree_weight.size), int(lp.value.shape[1])
    glist = [np.asarray(g.cpu() if isinstance(g, torch.Tensor) else g, np.int64).reshape(-1) for g in (groups or [])]
    G = len(glist)
    group_of = np.full(F, -1, np.int32)
    for g, cols in enumerate(glist):
        if cols.size and (int(cols.min()) < 0 or int(cols.max()) >= F):
            raise ValueError(f"group {g} names a column outside the matrix")
        if (group_of[cols] >= 0).any() or np.unique(cols).size != cols.size:
            raise ValueError("groups must be disjoint")
        group_of[cols] = g
    meta = ((zb[lp.used] & 0xFF) | ((group_of[lp.used] + 1) << 8)).astype(np.int32)
    out = torch.empty(n, U + G + 1, C, dtype=torch.float64, device=dev)
    if dev.type == "cuda":
        d = lp.on(dev)
        meta_d = _const_tensor(meta, dev)
        rc = N.hip().tmog_hip_forest_loco(
            N.ptr(Xb), F, n, N.ptr(row_list), U, N.ptr(d[0]), N.ptr(meta_d), G, T, N.ptr(d[1]), N.ptr(d[2]),
            int(lp.nodes.shape[0]), N.ptr(d[3]), KV, N.ptr(d[4]), N.ptr(d[5]), lp.missing_bin, C, lp.scale,
            N.ptr(out), N.stream(dev))
        if rc == -3:                 # one row's tile beyond the LDS limit
            return _on_host_twin(
                Xb, row_list, lambda sub: forest_loco(forest, sub, zb, None, glist, n_out=C, plan=lp)[0]), used64
        N.check(rc, "forest_loco")
        return out, used64
    N.check(N.host().tmog_forest_loco_cpu(
        N.ptr(Xb), F, n, N.ptr(row_list), U, lp.used.ctypes.data, meta.ctypes.data, G, T, lp.tree_off.ctypes.data,
        lp.nodes.ctypes.data, lp.value.ctypes.data, KV, lp.tree_weight.ctypes.data, lp.tree_out.ctypes.data,
        lp.missing_bin, C, lp.scale, N.ptr(out)), "forest_loco_cpu")
    return out, used64


# ------------------------------------------------------------------------------- partial dependence / ICE curves
def forest_partial_dependence(forest: Forest, Xb: torch.Tensor, cols, n_grid: int,
                              rows: Optional[torch.Tensor] = None, tree_weight: Optional[np.ndarray] = None,
                              tree_out: Optional[np.ndarray] = None, n_out: Optional[int] = None,
                              plan: Optional[ForestLoco] = None, ice: bool = False,
                              _walks: Optional[np.ndarray] = None) -> torch.Tensor:
    """Exact partial dependence of the forest's ``tree_weight``-weighted leaf-value sum on rows ``rows`` (None = all)
    of the binned matrix, over the complete bin grid of the columns ``cols`` (Q distinct matrix columns; ones no
    tree splits on are allowed, their curves are constant): float64 ``pd_sum [Q, NB, C]`` on the matrix's device,
    ``pd_sum[q, b] = sum_r s(x_r with column cols[q] replaced by bin b)``, ``NB = n_grid`` the model's histogram
    width (``BinSpec.B``, at most 256, the missing bin -- its last point -- included). With ``ice=True`` the
    per-record curves ``ice [n, Q, NB, C]`` instead. Tree ``t``'s ``K`` leaf values go to columns
    ``tree_out[t] .. tree_out[t] + K - 1`` of ``C = n_out``, as in :func:`forest_loco`, whose plan this reads
    (``plan``: the prepared :func:`forest_loco_plan`, callers cache it).

    The ICE result takes ``n * Q * NB * C * 8`` bytes (20 000 rows x 20 columns x 256 bins: 819 MB per output
    column): callers that only reduce it should pass their rows in blocks.

    Device matrices run ``tmog_hip_forest_pd``; host matrices, and a launch whose one row x one column is beyond
    the LDS limit, run the host twin -- both sum the same int64 fixed-point integers, so they agree bit for bit.
    ``_walks`` (host matrices only): an int64 ``[2]`` array that the host twin adds its counts of base walks and of
    step-function walks to (``benchmarks/bench_partial_dependence.py``)."""
    lp = plan if plan is not None else forest_loco_plan(forest, tree_weight, tree_out)
    if Xb.dtype != torch.uint8 or Xb.dim() != 2:
        raise ValueError("Xb must be a uint8 [N, F] matrix")
    dev = Xb.device
    Xb, Nrows, F, C, row_list, n, used64 = _explain_rows(lp, Xb, rows, n_out)
    NB = int(n_grid)
    if not 1 <= NB <= 256:
        raise ValueError(f"n_grid = {NB}: the grid is the model's histogram width, 1 .. 256")
    if 0 <= lp.missing_bin < NB - 1:
        raise ValueError(f"the missing bin {lp.missing_bin} must be the last point of the grid of {NB}")
    cq = np.asarray(cols.cpu() if isinstance(cols, torch.Tensor) else cols, np.int64).reshape(-1)
    Q = int(cq.size)
    if Q and (int(cq.min()) < 0 or int(cq.max()) >= F):
        raise ValueError("cols names a column outside the matrix")
    if np.unique(cq).size != Q:
        raise ValueError("cols must be distinct")
    slot_of = np.full(F, -1, np.int32)
    slot_of[cq] = np.arange(Q, dtype=np.int32)
    slot_of_used = np.ascontiguousarray(slot_of[lp.used], np.int32)
    if row_list is not None and n and not (0 <= int(row_list.min()) and int(row_list.max()) < Nrows):
        raise ValueError("rows names a row outside the matrix")
    U, T, KV = int(lp.used.size), int(lp.tree_weight.size), int(lp.value.shape[1])
    # the sum of n rows at a scale smaller by 2^ceil(log2 n): the same bound as one row's curve
    scale = lp.scale if ice else lp.scale / 2.0 ** max(0, (n - 1).bit_length())
    shape = (n, Q, NB, C) if ice else (Q, NB, C)
    if dev.type == "cuda":
        d = lp.on(dev)
        slot_d = _const_tensor(slot_of_used, dev)
        out = torch.empty(shape, dtype=torch.float64, device=dev) if ice else \
            torch.zeros(shape, dtype=torch.int64, device=dev)
        rc = N.hip().tmog_hip_forest_pd(
            N.ptr(Xb), F, n, N.ptr(row_list), U, N.ptr(d[0]), N.ptr(slot_d), Q, NB, T, N.ptr(d[1]), N.ptr(d[2]),
            int(lp.nodes.shape[0]), N.ptr(d[3]), KV, N.ptr(d[4]), N.ptr(d[5]), lp.missing_bin, C, scale,
            0 if ice else 1, N.ptr(out), N.stream(dev))
        if rc == -3:                 # one row x one column beyond the LDS limit
            return _on_host_twin(Xb, row_list, lambda sub: forest_partial_dependence(
                forest, sub, cq, NB, None, n_out=C, plan=lp, ice=ice))
        N.check(rc, "forest_pd")
        return out if ice else out.to(torch.float64) * (1.0 / scale)
    out = torch.empty(shape, dtype=torch.float64)
    N.check(N.host().tmog_forest_pd_cpu(
        N.ptr(Xb), F, n, N.ptr(row_list), U, lp.used.ctypes.data, slot_of_used.ctypes.data, Q, NB, T,
        lp.tree_off.ctypes.data, lp.nodes.ctypes.data, lp.value.ctypes.data, KV, lp.tree_weight.ctypes.data,
        lp.tree_out.ctypes.data, lp.missing_bin, C, scale, 0 if ice else 1, N.ptr(out),
        None if _walks is None else _walks.ctypes.data), "forest_pd_cpu")
    return out


# ------------------------------------------------------------------------------- two-way partial dependence surfaces
def forest_partial_dependence_pairs(forest: Forest, Xb: torch.Tensor, pairs, n_grid: int,
                                    rows: Optional[torch.Tensor] = None, tree_weight: Optional[np.ndarray] = None,
                                    tree_out: Optional[np.ndarray] = None, n_out: Optional[int] = None,
                                    plan: Optional[ForestLoco] = None, ice: bool = False,
                                    _walks: Optional[np.ndarray] = None) -> torch.Tensor:
    """Exact two-way partial dependence of the forest's ``tree_weight``-weighted leaf-value sum on rows ``rows``
    (None = all) of the binned matrix, over the complete bin grid of the column pairs ``pairs`` (int ``[Pn, 2]``
    matrix columns, the two of a pair different; columns no tree splits on are allowed, and the same pair may occur
    again, in either order): float64 ``sum2 [Pn, NB, NB, C]`` on the matrix's device, ``sum2[p, i, j] = sum_r s(x_r
    with column pairs[p, 0] replaced by bin i and column pairs[p, 1] by bin j)``. ``NB``, ``tree_out`` / ``n_out`` /
    ``tree_weight`` / ``rows`` / ``plan`` are those of :func:`forest_partial_dependence`. With ``ice=True`` the
    per-record surfaces ``ice2 [n, Pn, NB, NB, C]`` instead (``n * Pn * NB^2 * C * 8`` bytes: callers that only
    reduce them pass their rows in blocks).

    Device matrices run ``tmog_hip_forest_pd_pairs``; host matrices, and a launch whose one row x one grid line is
    beyond the LDS limit, run the host twin -- both sum the same int64 fixed-point integers, so they agree bit for
    bit. ``_walks`` (host matrices only): an int64 ``[3]`` array that the host twin adds its counts of base walks,
    anchor searches and rectangle walks to (``benchmarks/bench_partial_dependence_pairs.py``)."""
    lp = plan if plan is not None else forest_loco_plan(forest, tree_weight, tree_out)
    if Xb.dtype != torch.uint8 or Xb.dim() != 2:
        raise ValueError("Xb must be a uint8 [N, F] matrix")
    dev = Xb.device
    Xb, Nrows, F, C, row_list, n, used64 = _explain_rows(lp, Xb, rows, n_out)
    NB = int(n_grid)
    if not 1 <= NB <= 256:
        raise ValueError(f"n_grid = {NB}: the grid is the model's histogram width, 1 .. 256")
    if 0 <= lp.missing_bin < NB - 1:
        raise ValueError(f"the missing bin {lp.missing_bin} must be the last point of the grid of {NB}")
    pq = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, np.int64)
    if pq.size == 0:
        pq = pq.reshape(0, 2)
    if pq.ndim != 2 or pq.shape[1] != 2:
        raise ValueError("pairs must be an int [Pn, 2] array of matrix columns")
    Pn = int(pq.shape[0])
    if Pn and (int(pq.min()) < 0 or int(pq.max()) >= F):
        raise ValueError("pairs names a column outside the matrix")
    if (pq[:, 0] == pq[:, 1]).any():
        raise ValueError("the two columns of a pair must be different")
    slot_of = np.full(F, -1, np.int32)
    slot_of[lp.used] = np.arange(lp.used.size, dtype=np.int32)
    pair_slots = np.ascontiguousarray(slot_of[pq], np.int32)
    if row_list is not None and n and not (0 <= int(row_list.min()) and int(row_list.max()) < Nrows):
        raise ValueError("rows names a row outside the matrix")
    U, T, KV = int(lp.used.size), int(lp.tree_weight.size), int(lp.value.shape[1])
    # the sum of n rows at a scale smaller by 2^ceil(log2 n): the same bound as one row's surface
    scale = lp.scale if ice else lp.scale / 2.0 ** max(0, (n - 1).bit_length())
    shape = (n, Pn, NB, NB, C) if ice else (Pn, NB, NB, C)
    if dev.type == "cuda":
        d = lp.on(dev)
        slot_d = _const_tensor(pair_slots.reshape(-1), dev)
        out = torch.empty(shape, dtype=torch.float64, device=dev) if ice else \
            torch.zeros(shape, dtype=torch.int64, device=dev)
        rc = N.hip().tmog_hip_forest_pd_pairs(
            N.ptr(Xb), F, n, N.ptr(row_list), U, N.ptr(d[0]), N.ptr(slot_d), Pn, NB, T, N.ptr(d[1]), N.ptr(d[2]),
            int(lp.nodes.shape[0]), N.ptr(d[3]), KV, N.ptr(d[4]), N.ptr(d[5]), lp.missing_bin, C, scale,
            0 if ice else 1, N.ptr(out), N.stream(dev))
        if rc == -3:                 # one row x one grid line beyond the LDS limit
            return _on_host_twin(Xb, row_list, lambda sub: forest_partial_dependence_pairs(
                forest, sub, pq, NB, None, n_out=C, plan=lp, ice=ice))
        N.check(rc, "forest_pd_pairs")
        return out if ice else out.to(torch.float64) * (1.0 / scale)
    out = torch.empty(shape, dtype=torch.float64)
    N.check(N.host().tmog_forest_pd_pairs_cpu(
        N.ptr(Xb), F, n, N.ptr(row_list), U, lp.used.ctypes.data, pair_slots.ctypes.data, Pn, NB, T,
        lp.tree_off.ctypes.data, lp.nodes.ctypes.data, lp.value.ctypes.data, KV, lp.tree_weight.ctypes.data,
        lp.tree_out.ctypes.data, lp.missing_bin, C, scale, 0 if ice else 1, N.ptr(out),
        None if _walks is None else _walks.ctypes.data), "forest_pd_pairs_cpu")
    return out
