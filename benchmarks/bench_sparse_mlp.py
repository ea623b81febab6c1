"""Benchmark of the MLP classifier on a sparse design: the whole-network HIP pass (``ops/csrc/hip/sparse_mlp_kernels.hip``,
``TMOG_MLP_SPARSE_FUSED=1``) against the dense layer products on the densified matrix (``TMOG_MLP_SPARSE_FUSED=0``).

Shape of the multi-class text configuration's design matrix: ``--rows`` x ``--cols`` at ``--density`` non-zeros plus
``--dense`` dense columns, ``--classes`` classes, ``--problems`` = 2 grid points x 3 folds, for the layer sizes
``[cols, 32, classes]`` and ``[cols, 64, 16, classes]``. Times, both paths in the same process and in alternation
(``--rounds`` rounds, the median is reported; every window follows two warm-up calls, runs for at least ``--window``
seconds and ends in a device synchronise):

* the objective's value pass and value + gradient pass alone (``MLPObjective``, the fused one on one ``SparseDesign``);
* one ``OpMultilayerPerceptronClassifier.fit_batch`` of the problems (``--max-iter`` iterations), the ``SparseDesign``
  build included.

Both paths' objective values and gradients are compared on the timed inputs. Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from benchmarks.bench_sparse_linear import _design, _timed  # noqa: E402
from transmogrifai_amd.models import mlp as MM  # noqa: E402
from transmogrifai_amd.models.base import FitJob, learner_class  # noqa: E402
from transmogrifai_amd.ops import linear as LK  # noqa: E402

SWITCH = "TMOG_MLP_SPARSE_FUSED"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1352)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--dense", type=int, default=8)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--problems", type=int, default=6)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_mlp needs a GPU")
    dev = torch.device("cuda")
    X, g = _design(a.rows, a.cols, a.density, a.dense, dev)
    beta = torch.zeros(a.cols, a.classes, device=dev)
    beta[:64] = torch.randn(64, a.classes, device=dev, generator=g)
    y = torch.argmax(X @ beta + torch.randn(a.rows, a.classes, device=dev, generator=g), 1).double()
    P, folds = a.problems, 3
    fold = torch.randint(0, folds, (a.rows,), device=dev, generator=g)
    W = torch.stack([(fold != p % folds).float() for p in range(P)], 1).contiguous()
    rows_of = [torch.nonzero(fold != c).reshape(-1) for c in range(folds)]
    D = LK.SparseDesign(X)
    lr = learner_class("OpMultilayerPerceptronClassifier")()
    res = {"bench": "sparse_mlp", "rows": a.rows, "cols": a.cols, "nnz_per_row": D.nnz / a.rows,
           "dense_cols": int(D.idx_d.numel()), "classes": a.classes, "problems": P, "window_s": a.window,
           "rounds": a.rounds, "max_iter": a.max_iter, "layers": {}}
    for layers in ([a.cols, 32, a.classes], [a.cols, 64, 16, a.classes]):
        assert LK.sparse_mlp_supported(D, layers)
        obj = {"1": MM.MLPObjective(D, y, W, layers), "0": MM.MLPObjective(X, y, W, layers)}
        U = torch.as_tensor(MM._init_params(layers, 0), device=dev)[:, None].repeat(1, P) + \
            0.05 * torch.randn(obj["1"].n_params, P, dtype=torch.float64, device=dev, generator=g)
        (f1, g1), (f0, g0) = obj["1"].value_grad(U), obj["0"].value_grad(U)
        jobs = [FitJob(dict(lr.defaults, layers=layers, max_iter=a.max_iter, seed=p // folds), rows_of[p % folds])
                for p in range(P)]
        t = {k: {"1": [], "0": []} for k in ("value_ms", "value_grad_ms", "fit_ms")}
        for rnd in range(a.rounds):
            print(f"{layers[1:]} round {rnd + 1} / {a.rounds}", file=sys.stderr, flush=True)
            for sw in ("1", "0"):
                os.environ[SWITCH] = sw
                t["value_ms"][sw].append(_timed(lambda: obj[sw].value(U), a.window))
                t["value_grad_ms"][sw].append(_timed(lambda: obj[sw].value_grad(U), a.window))
                t["fit_ms"][sw].append(_timed(lambda: lr.fit_batch(X, y, jobs), a.window))
        r = {"f_max_rel_diff": float(((f1 - f0).abs() / f0.abs()).max()),
             "g_max_abs_diff": float((g1 - g0).abs().max()), "g_max_abs": float(g0.abs().max())}
        for k, v in t.items():
            r["fused_" + k] = statistics.median(v["1"])
            r["unfused_" + k] = statistics.median(v["0"])
            r[k + "_all"] = v
        res["layers"]["-".join(map(str, layers[1:]))] = r
        del obj
    print(json.dumps(res))


if __name__ == "__main__":
    main()
