"""Benchmark of the binary linear learners on a sparse design: the fused HIP pass (``ops/csrc/hip/sparse_lr_kernels.hip``)
against the unfused pass (CSR product + dense-block GEMM + torch elementwise epilogue, ``TMOG_LR_SPARSE_FUSED=0``).

Shape of the multi-class text configuration's design matrix: ``--rows`` x ``--cols`` at ``--density`` non-zeros plus
``--dense`` dense columns, ``--problems`` = 8 grid points x 3 folds. Times, with the switch on and off in the same process
and in alternation (``--rounds`` rounds, the median is reported; every window follows two warm-up calls, runs for at least
``--window`` seconds and ends in a device synchronise):

* the objective's value pass and value + gradient pass alone (``BatchedObjective`` on one ``SparseDesign``);
* one binary ``OpLogisticRegression.fit_batch`` of the 24 problems (``--max-iter`` iterations).

Both paths' objective values and gradients are compared on the timed inputs. Prints one JSON line."""
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

from transmogrifai_amd.models import linear as ML  # noqa: E402
from transmogrifai_amd.models.base import FitJob, learner_class  # noqa: E402
from transmogrifai_amd.ops import linear as LK  # noqa: E402

SWITCH = "TMOG_LR_SPARSE_FUSED"


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1352)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--dense", type=int, default=4)
    ap.add_argument("--problems", type=int, default=24)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_linear needs a GPU")
    dev = torch.device("cuda")
    X, g = _design(a.rows, a.cols, a.density, a.dense, dev)
    beta = torch.zeros(a.cols, device=dev)
    beta[:16] = torch.randn(16, device=dev, generator=g)
    y = (torch.rand(a.rows, device=dev, generator=g) < torch.sigmoid(X @ beta)).float()
    P, folds = a.problems, 3
    fold = torch.randint(0, folds, (a.rows,), device=dev, generator=g)
    wcols = [p % folds for p in range(P)]                      # the grid points of a fold share its rows
    W = torch.stack([(fold != c).float() for c in wcols], 1).contiguous()
    D = LK.SparseDesign(X)
    inv_std = torch.ones(a.cols, P, dtype=torch.float64, device=dev)
    l2 = torch.full((P,), 0.01, dtype=torch.float64, device=dev)
    fi = torch.ones(P, dtype=torch.bool, device=dev)
    U = 0.05 * torch.randn(a.cols + 1, P, dtype=torch.float64, device=dev, generator=g)

    obj = {}
    for sw in ("1", "0"):
        os.environ[SWITCH] = sw
        obj[sw] = ML.BatchedObjective(D, y, W, inv_std, "logistic", l2, fi, wcols=wcols)
        assert obj[sw].fused == (sw == "1")
    f1, g1 = obj["1"].value_grad(U)
    f0, g0 = obj["0"].value_grad(U)
    lr = learner_class("OpLogisticRegression")()
    rows_of = [torch.nonzero(fold != c).reshape(-1) for c in range(folds)]
    jobs = [FitJob(dict(lr.defaults, reg_param=0.001 * 2 ** (p // folds), max_iter=a.max_iter), rows_of[p % folds])
            for p in range(P)]

    def fit():
        lr.fit_batch(X, y, jobs)

    t = {k: {"1": [], "0": []} for k in ("value_ms", "value_grad_ms", "fit_ms")}
    for rnd in range(a.rounds):
        print(f"round {rnd + 1} / {a.rounds}", file=sys.stderr, flush=True)
        for sw in ("1", "0"):
            os.environ[SWITCH] = sw
            t["value_ms"][sw].append(_timed(lambda: obj[sw].value(U), a.window))
            t["value_grad_ms"][sw].append(_timed(lambda: obj[sw].value_grad(U), a.window))
            t["fit_ms"][sw].append(_timed(fit, a.window))
    res = {"bench": "sparse_binary_objective", "rows": a.rows, "cols": a.cols, "nnz_per_row": D.nnz / a.rows,
           "dense_cols": int(D.idx_d.numel()), "problems": P, "window_s": a.window, "rounds": a.rounds,
           "max_iter": a.max_iter,
           "f_max_rel_diff": float(((f1 - f0).abs() / f0.abs()).max()),
           "g_max_abs_diff": float((g1 - g0).abs().max()), "g_max_abs": float(g0.abs().max())}
    for k, v in t.items():
        res["fused_" + k] = statistics.median(v["1"])
        res["unfused_" + k] = statistics.median(v["0"])
        res[k + "_all"] = v
    print(json.dumps(res))


if __name__ == "__main__":
    main()
