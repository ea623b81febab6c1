"""Benchmark of the regression learners' weighted Grams on a sparse design: ``SparseDesign.wgram``
(``ops/csrc/hip/sparse_gram_kernels.hip``) against the dense fp64 matrix-core ``ops.stats.weighted_gram``, and the two
learners with the sparse path on and off (``TMOG_LINREG_SPARSE``).

Shape of the multi-class text configuration's design matrix: ``--rows`` x ``--cols`` at ``--density`` non-zeros plus
``--dense`` dense columns. Times, with the switch on and off in the same process and in alternation (``--rounds`` rounds,
the median is reported; every window follows two warm-up calls, runs for at least ``--window`` seconds and ends in a
device synchronise):

* the Grams alone for K = 3 fold weights with a shared ``y`` (linear regression) and for K = 24 weights with a response
  each (one IRLS iteration), ``wgram`` on a built design against ``weighted_gram``; and the build of the design;
* one ``OpLinearRegression.fit_batch`` of 8 grid points x 3 folds;
* one Poisson / log ``OpGeneralizedLinearRegression.fit_batch`` of 2 grid points x 3 folds.

Both paths' Grams are compared on the timed inputs. ``--fits-only`` times the two ``fit_batch`` calls alone, as the
environment has them (a tree without the sparse path: the parent's figures). Prints one JSON line."""
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
from transmogrifai_amd.ops import linear as LK  # noqa: E402
from transmogrifai_amd.ops.stats import weighted_gram  # noqa: E402

SWITCH = "TMOG_LINREG_SPARSE"


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
    reps = max(1, math.ceil(window_s / max(time.perf_counter() - t0, 1e-6)))
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
    ap.add_argument("--dense", type=int, default=8)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fits-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_gram needs a GPU")
    dev = torch.device("cuda")
    X, g = _design(a.rows, a.cols, a.density, a.dense, dev)
    beta = torch.zeros(a.cols, device=dev)
    beta[:16] = 0.1 * torch.randn(16, device=dev, generator=g)
    eta = X @ beta
    y = eta + torch.randn(a.rows, device=dev, generator=g)
    y_poi = torch.poisson(torch.exp(0.5 * eta.clamp(-4, 4)), generator=g)
    folds = 3
    fold = torch.randint(0, folds, (a.rows,), device=dev, generator=g)
    rows_of = [torch.nonzero(fold != c).reshape(-1) for c in range(folds)]
    lin = learner_class("OpLinearRegression")()
    glm = learner_class("OpGeneralizedLinearRegression")()
    lin_jobs = [FitJob(dict(lin.defaults, reg_param=0.001 * 2 ** q), rows_of[f]) for q in range(8) for f in range(folds)]
    glm_jobs = [FitJob(dict(glm.defaults, family="poisson", reg_param=0.01 * 10 ** q), rows_of[f])
                for q in range(2) for f in range(folds)]
    fits = {"linreg_fit_ms": lambda: lin.fit_batch(X, y, lin_jobs), "glm_fit_ms": lambda: glm.fit_batch(X, y_poi, glm_jobs)}
    res = {"bench": "sparse_wgram", "rows": a.rows, "cols": a.cols, "density": a.density, "dense_cols": a.dense,
           "window_s": a.window, "rounds": a.rounds, "linreg_problems": len(lin_jobs), "glm_problems": len(glm_jobs)}
    if a.fits_only:
        t = {k: [] for k in fits}
        for rnd in range(a.rounds):
            print(f"round {rnd + 1} / {a.rounds}", file=sys.stderr, flush=True)
            for k, fn in fits.items():
                t[k].append(_timed(fn, a.window))
        res.update({SWITCH: os.environ.get(SWITCH), "sparse_path": hasattr(LK.SparseDesign, "wgram")})
        res.update({k: statistics.median(v) for k, v in t.items()})
        res.update({k + "_all": v for k, v in t.items()})
        print(json.dumps(res))
        return

    D = LK.SparseDesign(X)
    assert LK.sparse_wgram_supported(D)
    W3 = torch.stack([(fold != c).double() for c in range(folds)], 1).contiguous()
    W24 = (W3.repeat(1, 8) * (0.5 + torch.rand(a.rows, 24, device=dev, generator=g).double())).contiguous()
    Y24 = torch.randn(a.rows, 24, device=dev, generator=g).double()
    yd = y.double()
    grams = {"gram_k3_shared_y_ms": {"1": lambda: D.wgram(W3, yd), "0": lambda: weighted_gram(X, W3, yd)},
             "gram_k24_per_weight_y_ms": {"1": lambda: D.wgram(W24, Y24), "0": lambda: weighted_gram(X, W24, Y24)}}
    for k, pair in grams.items():                  # the two paths on the timed inputs
        Gs, Gd = pair["1"](), pair["0"]()
        res[k[:-3] + "_max_abs_diff"] = float((Gs - Gd).abs().max())
        res[k[:-3] + "_max_abs"] = float(Gd.abs().max())
        res[k[:-3] + "_symmetric"] = bool(torch.equal(Gs, Gs.transpose(1, 2)))
        del Gs, Gd
    res.update({"nnz_per_row": D.nnz / a.rows, "design_dense_cols": int(D.idx_d.numel())})
    t = {k: {"1": [], "0": []} for k in list(grams) + list(fits)}
    build = []
    for rnd in range(a.rounds):
        print(f"round {rnd + 1} / {a.rounds}", file=sys.stderr, flush=True)
        build.append(_timed(lambda: LK.SparseDesign(X), 0.0))
        for sw in ("1", "0"):
            os.environ[SWITCH] = sw
            for k, pair in grams.items():
                t[k][sw].append(_timed(pair[sw], a.window))
            for k, fn in fits.items():
                t[k][sw].append(_timed(fn, a.window))
    res["design_build_ms"] = statistics.median(build)
    for k, v in t.items():
        res["sparse_" + k] = statistics.median(v["1"])
        res["dense_" + k] = statistics.median(v["0"])
        res[k + "_all"] = v
    print(json.dumps(res))


if __name__ == "__main__":
    main()
