"""The validation curve of a boosted model: the staged evaluation kernel against one ``forest_predict`` per round.

Trains one ``OpXGBoostClassifier`` (``--rounds`` rounds, depth ``--depth``) on ``--train-rows`` rows of a synthetic
``--rows`` x ``--cols`` table, then computes the logloss after every round on all ``--rows`` binned rows two ways:

* ``staged``: ``tree_engine.forest_staged_eval`` (ops/csrc/hip/staged_eval_kernels.hip), one pass over the trees;
* ``per_round``: what the package offered before it: one ``forest_predict`` launch on each round's tree (the
  single-tree forests are cut out beforehand), the fp32 leaf values accumulated into an fp64 margin and the logloss
  taken with torch ops.

Both are timed with device events in one process, alternating, ``--runs`` times after one warm-up each; the result
(medians, every run, the largest difference between the two curves) goes to ``--out`` and is printed as one JSON line.
Not part of any gate: no threshold, the file records what was found.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _event_ms(fn, dev):
    if dev.type != "cuda":                      # a dry run on the host backend: wall time
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=200)
    ap.add_argument("--train-rows", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "staged_eval_vs_per_round.txt"))
    a = ap.parse_args()
    from transmogrifai_amd.models import tree_engine as te
    from transmogrifai_amd.models.base import FitJob
    from transmogrifai_amd.models.trees import XGBoostClassifierLearner

    dev = torch.device(a.device)
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn(a.rows, a.cols, generator=g, device=dev, dtype=torch.float32)
    score = X[:, :8].sum(1) + 0.5 * X[:, 8] * X[:, 9]
    y = ((score + 2.0 * torch.randn(a.rows, generator=g, device=dev)) > 0).to(torch.float32)
    L = XGBoostClassifierLearner()
    params = dict(L.defaults, num_round=a.rounds, max_depth=a.depth, eta=0.1)
    st = L.fit_batch(X, y, [FitJob(params, torch.arange(min(a.train_rows, a.rows), device=dev))])[0]
    forest, Xb = L._binned_for(st, X, None)
    del X
    T = forest.n_trees
    tw = np.asarray(st["tree_weights"], np.float32)
    base = float(st["base_margin"])
    yd = y.to(torch.float64)

    def staged():
        return te.forest_staged_eval(forest, Xb, None, y, stage_off=np.arange(T + 1), tree_weight=tw,
                                     metric="logloss", base=base)[0]

    singles = [forest.tree(t) for t in range(T)]

    def per_round():
        m = torch.full((a.rows,), base, dtype=torch.float64, device=dev)
        out = []
        for t in range(T):
            m += te.forest_predict(singles[t], Xb, [None], [[0]], tw[t:t + 1])[0][:, 0].to(torch.float64)
            out.append((torch.log1p(torch.exp(-m.abs())) + m.clamp_min(0) - yd * m).mean())
        return torch.stack(out).cpu().numpy()

    times = {"staged": [], "per_round": []}
    curves = {}
    for name, fn in (("staged", staged), ("per_round", per_round)):
        curves[name] = _event_ms(fn, dev)[1]                     # warm-up
    for _ in range(a.runs):
        for name, fn in (("staged", staged), ("per_round", per_round)):
            times[name].append(_event_ms(fn, dev)[0])
    res = {"model": f"OpXGBoostClassifier num_round={a.rounds} max_depth={a.depth} ({T} trees, "
                    f"{int((forest.nodes[:, 2] < 0).sum())} leaves)",
           "rows": a.rows, "cols": a.cols, "train_rows": min(a.train_rows, a.rows), "metric": "logloss",
           "gpu": torch.cuda.get_device_name(dev) if dev.type == "cuda" else None, "runs": a.runs}
    for name, ts in times.items():
        res[f"{name}_median_ms"] = round(statistics.median(ts), 2)
        res[f"{name}_min_ms"], res[f"{name}_max_ms"] = round(min(ts), 2), round(max(ts), 2)
        res[f"{name}_runs_ms"] = [round(t, 2) for t in ts]
    res["per_round_over_staged"] = round(res["per_round_median_ms"] / res["staged_median_ms"], 2)
    res["curve_max_abs_diff"] = float(np.abs(curves["staged"] - curves["per_round"]).max())
    res["curve_first_last"] = [float(curves["staged"][0]), float(curves["staged"][-1])]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("Validation curve: forest_staged_eval vs one forest_predict per round (benchmarks/bench_staged_eval.py): "
                f"device-event times of {a.runs} alternating runs after one warm-up each\n")
        for k, v in res.items():
            f.write(f"{k}: {v}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
