"""Benchmark of the build of the sparse designs: ``SparseDesign(X)`` and ``DocTermCSR(X)`` from
``ops/csrc/hip/sparse_build_kernels.hip`` (``TMOG_SPARSE_BUILD=1``) against the torch build (``=0``).

Shape of the multi-class text configuration's design matrix, as ``bench_sparse_gram.py``: ``--rows`` x ``--cols`` at
``--density`` non-zeros plus ``--dense`` dense columns; and the smallest shape ``SparseDesign.worthwhile`` accepts
(``--small-rows`` x ``--small-cols``). Per shape, with the switch on and at 0 in the same process and in alternation
(``--rounds`` rounds; median, minimum and maximum are reported; every window follows two warm-up calls, runs for at least
``--window`` seconds and ends in a device synchronise):

* ``SparseDesign(X)`` and ``DocTermCSR(X)``, and the peak of ``torch.cuda.max_memory_allocated`` over one build above
  what was allocated before it (``X`` stays resident);
* at the large shape one binary ``OpLogisticRegression.fit_batch`` of 24 problems (``--max-iter`` iterations).

The two builds' fields are compared on the timed inputs. Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from transmogrifai_amd.models.base import FitJob, learner_class  # noqa: E402
from transmogrifai_amd.ops import lda as LDA  # noqa: E402
from transmogrifai_amd.ops import linear as LK  # noqa: E402

SWITCH = "TMOG_SPARSE_BUILD"
FIELDS = {"design": ("idx_d", "idx_s", "Xd", "row_ptr", "col", "val", "csc_row", "csc_val", "csc_val_sq", "col_seg",
                     "seg_begin"),
          # row_sum apart: the torch build adds it with index_add_, in no fixed order
          "doc_term": ("row_ptr", "col", "val", "csc_row", "csc_pos", "col_seg", "seg_begin")}


def _design(rows, cols, density, dense, dev, chunk=1 << 16):
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.zeros(rows, cols, device=dev)
    for a in range(0, rows, chunk):
        n = min(chunk, rows - a)
        hit = torch.rand(n, cols, device=dev, generator=g) < density
        X[a:a + n] = torch.where(hit, torch.rand(n, cols, device=dev, generator=g) * 3, X[a:a + n])
    X[:, :dense] = torch.randn(rows, dense, device=dev, generator=g)
    return X, g


def _timed(fn, window_s):
    """Milliseconds per call over a window of at least ``window_s`` seconds; the call count comes from the second of two
    warm-up calls, timed on its own."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(3, math.ceil(window_s / max(time.perf_counter() - t0, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0) / reps


def _peak_mb(fn):
    """Peak device memory of one call above what was allocated before it, in MB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak / 1e6


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def _shape(X, a, fit):
    builds = {"design": lambda: LK.SparseDesign(X), "doc_term": lambda: LDA.DocTermCSR(X)}
    res = {"rows": X.shape[0], "cols": X.shape[1]}
    for k, fn in builds.items():                   # the two builds on the timed input
        made = {}
        for sw in ("1", "0"):
            os.environ[SWITCH] = sw
            made[sw] = fn()
            res[f"{k}_peak_mb_{sw}"] = _peak_mb(fn)
        res[k + "_equal"] = all(torch.equal(getattr(made["1"], f), getattr(made["0"], f)) for f in FIELDS[k]) \
            and made["1"].nnz == made["0"].nnz and made["1"].n_seg == made["0"].n_seg
        res["nnz_per_row"] = made["1"].nnz / X.shape[0]
        del made
    timed = dict(builds, **({"fit": fit} if fit is not None else {}))
    t = {k: {"1": [], "0": []} for k in timed}
    for rnd in range(a.rounds):
        print(f"{X.shape[0]} x {X.shape[1]}: round {rnd + 1} / {a.rounds}", file=sys.stderr, flush=True)
        for k, fn in timed.items():
            for sw in ("1", "0"):
                os.environ[SWITCH] = sw
                t[k][sw].append(_timed(fn, a.window))
    for k, v in t.items():
        res[k + "_ms_1"], res[k + "_ms_0"] = _stats(v["1"]), _stats(v["0"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1352)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--dense", type=int, default=8)
    ap.add_argument("--small-rows", type=int, default=4096)
    ap.add_argument("--small-cols", type=int, default=256)
    ap.add_argument("--problems", type=int, default=24)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_build needs a GPU")
    dev = torch.device("cuda")
    res = {"bench": "sparse_build", "density": a.density, "dense_cols": a.dense, "window_s": a.window,
           "rounds": a.rounds, "problems": a.problems, "max_iter": a.max_iter}
    Xs, _ = _design(a.small_rows, a.small_cols, a.density, a.dense, dev)
    res["small"] = _shape(Xs, a, None)
    del Xs
    X, g = _design(a.rows, a.cols, a.density, a.dense, dev)
    beta = torch.zeros(a.cols, device=dev)
    beta[:16] = torch.randn(16, device=dev, generator=g)
    y = (torch.rand(a.rows, device=dev, generator=g) < torch.sigmoid(X @ beta)).float()
    folds = 3
    fold = torch.randint(0, folds, (a.rows,), device=dev, generator=g)
    rows_of = [torch.nonzero(fold != c).reshape(-1) for c in range(folds)]
    lr = learner_class("OpLogisticRegression")()
    jobs = [FitJob(dict(lr.defaults, reg_param=0.001 * 2 ** (p // folds), max_iter=a.max_iter), rows_of[p % folds])
            for p in range(a.problems)]
    res["large"] = _shape(X, a, lambda: lr.fit_batch(X, y, jobs))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
