"""Benchmark of multinomial logistic regression on a sparse design: the fused HIP pass
(``ops/csrc/hip/sparse_mnl_kernels.hip``, ``TMOG_MNL_SPARSE_FUSED=1``) against the unfused pass (dense-block GEMM + CSR
product into ``M [N, P*K]`` + ``softmax_objective`` over it, ``TMOG_MNL_SPARSE_FUSED=0``).

Shape of the multi-class text configuration's design matrix: ``--rows`` x ``--cols`` at ``--density`` non-zeros plus
``--dense`` dense columns, ``--classes`` classes, ``--problems`` = 8 grid points x 3 folds. Every setting of the switch is
timed in a fresh child process (the objective decides its path once, and a process keeps its allocator and library state),
the settings in alternation for ``--rounds`` rounds; the median is reported. Every window follows two warm-up calls, runs
for at least ``--window`` seconds and ends in a device synchronise. A child times

* the objective's value pass and value + gradient pass alone (``MultinomialObjective`` on one ``SparseDesign``);
* one multinomial ``OpLogisticRegression.fit_batch`` of the problems (``--max-iter`` iterations), the ``SparseDesign``
  build included,

and compares both paths' objective values and gradients on the timed inputs. With ``--bf16`` one more child per round times
the same fit under ``TMOG_LINEAR_DTYPE=bf16`` (the dense bf16 design; no ``SparseDesign``). Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCH = "TMOG_MNL_SPARSE_FUSED"


def child(a):
    import torch

    from benchmarks.bench_sparse_linear import _design, _timed
    from transmogrifai_amd.models import linear as ML
    from transmogrifai_amd.models.base import FitJob, learner_class
    from transmogrifai_amd.ops import linear as LK
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_mnl needs a GPU")
    dev = torch.device("cuda")
    K, P, folds = a.classes, a.problems, 3
    X, g = _design(a.rows, a.cols, a.density, a.dense, dev)
    beta = torch.zeros(a.cols, K, device=dev)
    beta[:64] = torch.randn(64, K, device=dev, generator=g)
    y = torch.argmax(X @ beta + torch.randn(a.rows, K, device=dev, generator=g), 1).float()
    fold = torch.randint(0, folds, (a.rows,), device=dev, generator=g)
    lr = learner_class("OpLogisticRegression")()
    rows_of = [torch.nonzero(fold != c).reshape(-1) for c in range(folds)]
    jobs = [FitJob(dict(lr.defaults, reg_param=0.001 * 2 ** (p // folds), max_iter=a.max_iter), rows_of[p % folds])
            for p in range(P)]
    res = {"setting": a.child, "fit_ms": _timed(lambda: lr.fit_batch(X, y, jobs), a.window)}
    if a.child != "bf16":
        wcols = [p % folds for p in range(P)]                  # the grid points of a fold share its rows
        W = torch.stack([(fold != c).float() for c in wcols], 1).contiguous()
        D = LK.SparseDesign(X)
        inv_std = torch.ones(a.cols, P, dtype=torch.float64, device=dev)
        l2 = torch.full((P,), 0.01, dtype=torch.float64, device=dev)
        fi = torch.ones(P, dtype=torch.bool, device=dev)
        U = 0.05 * torch.randn((a.cols + 1) * K, P, dtype=torch.float64, device=dev, generator=g)
        obj = {}
        for sw in (a.child, "1", "0"):                         # the timed one first: the others are for the comparison
            os.environ[SWITCH] = sw
            obj.setdefault(sw, ML.MultinomialObjective(D, y, W, inv_std, l2, fi, K, wcols=wcols))
        os.environ[SWITCH] = a.child
        (f1, g1), (f0, g0) = obj["1"].value_grad(U), obj["0"].value_grad(U)
        res.update(sparse=bool(getattr(obj[a.child], "sparse", False)), nnz_per_row=D.nnz / a.rows,
                   dense_cols=int(D.idx_d.numel()),
                   value_ms=_timed(lambda: obj[a.child].value(U), a.window),
                   value_grad_ms=_timed(lambda: obj[a.child].value_grad(U), a.window),
                   f_max_rel_diff=float(((f1 - f0).abs() / f0.abs()).max()),
                   g_max_abs_diff=float((g1 - g0).abs().max()), g_max_abs=float(g0.abs().max()))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1352)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--dense", type=int, default=8)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--problems", type=int, default=24)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--bf16", action="store_true", help="also time the fit under TMOG_LINEAR_DTYPE=bf16")
    ap.add_argument("--child", choices=("1", "0", "bf16"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    settings = ("1", "0") + (("bf16",) if a.bf16 else ())
    runs = {s: [] for s in settings}
    for rnd in range(a.rounds):
        for s in settings:
            print(f"round {rnd + 1} / {a.rounds}, setting {s}", file=sys.stderr, flush=True)
            env = dict(os.environ, **({"TMOG_LINEAR_DTYPE": "bf16"} if s == "bf16" else {SWITCH: s}))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", s] +
                                 [x for x in sys.argv[1:] if x != "--bf16"], env=env, check=True,
                                 stdout=subprocess.PIPE, text=True).stdout
            runs[s].append(json.loads(out.strip().splitlines()[-1]))
    res = {"bench": "sparse_mnl", "rows": a.rows, "cols": a.cols, "classes": a.classes, "problems": a.problems,
           "window_s": a.window, "rounds": a.rounds, "max_iter": a.max_iter}
    for k in ("nnz_per_row", "dense_cols", "f_max_rel_diff", "g_max_abs_diff", "g_max_abs"):
        res[k] = runs["1"][0][k]
    res["fused_takes_sparse_pass"] = [r["sparse"] for r in runs["1"]]
    for s, name in (("1", "fused_"), ("0", "unfused_"), ("bf16", "bf16_")):
        for k in ("value_ms", "value_grad_ms", "fit_ms"):
            v = [r[k] for r in runs.get(s, ()) if k in r]
            if v:
                res[name + k] = statistics.median(v)
                res[name + k + "_all"] = v
    print(json.dumps(res))


if __name__ == "__main__":
    main()
