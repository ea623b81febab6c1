"""RecordInsightsLOCO on linear-margin learners: the rescore mode against the margins mode.

Two shapes, each one fitted model explained on the same ``--records`` records in both modes:

* ``dense``: binary ``OpLogisticRegression`` on a dense design of 200 columns;
* ``sparse``: multinomial ``OpLogisticRegression`` with 6 classes on 1352 columns at about 40 non-zeros a row, 1024 of
  the columns being two hashed-text groups of 512.

``perturbation="rescore"`` scores one perturbed copy of the record per non-zero column through the model's predict;
``perturbation="margins"`` runs the HIP kernel of ``loco_linear_kernels.hip``. The two modes alternate in one process,
every run is device-synchronised wall time, and the median of ``--runs`` runs after one warm-up each is reported with
all runs and the ratio, as is the share of records whose insights name the same columns in both modes. Writes the
result to ``--out`` and prints it as one JSON line. Not part of any gate: no threshold, the file records what was
found.
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


def _timed(fn, dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _design(shape, rows, dev):
    """(X fp32 [rows, d], y, column histories): the dense or the sparse design, labels from a random linear model."""
    g = torch.Generator(device="cpu").manual_seed(7)
    if shape == "dense":
        d, classes, text = 200, 2, range(0)
        X = torch.randn(rows, d, generator=g)
    else:
        d, classes, text = 1352, 6, range(328, 1352)
        X = torch.zeros(rows, d)
        cols = torch.randint(0, d, (rows, 40), generator=g)
        X.scatter_(1, cols, torch.rand(rows, 40, generator=g) + 0.5)
    z = X @ torch.randn(d, classes, generator=g) + torch.randn(rows, classes, generator=g)
    y = (z[:, 1] > z[:, 0]).float() if classes == 2 else z.argmax(1).float()
    hist = [{"columnName": f"c{j}", "index": j, "parentFeatureType": ["Text" if j in text else "Real"],
             "parentFeatureName": [f"t{(j - 328) // 512}" if j in text else f"r{j}"]} for j in range(d)]
    return X.to(dev), y.to(dev), hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--records", type=int, default=5_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loco_margins.txt"))
    a = ap.parse_args()
    from transmogrifai_amd.data.columns import VectorColumn
    from transmogrifai_amd.models.base import OpPredictorModel
    from transmogrifai_amd.models.linear import LogisticRegressionLearner
    from transmogrifai_amd.stages.insights.record_insights import RecordInsightsLOCO

    dev = torch.device(a.device if torch.cuda.is_available() else "cpu")
    res = {"records": a.records, "train_rows": a.rows, "top_k": a.top_k, "device": str(dev),
           "gpu": torch.cuda.get_device_name(dev) if dev.type == "cuda" else None}
    modes = ("rescore", "margins")
    for shape in ("dense", "sparse"):
        X, y, hist = _design(shape, a.rows, dev)
        state = LogisticRegressionLearner(reg_param=0.01, max_iter=30).fit(X, y)
        model = OpPredictorModel("OpLogisticRegression", state, {})
        sub = VectorColumn(X[:a.records].contiguous())
        stages = {m: RecordInsightsLOCO(model, top_k=a.top_k, perturbation=m) for m in modes}
        for st in stages.values():
            st.histories = hist
        run = {m: (lambda st=stages[m]: st.transform_columns(sub)) for m in modes}
        out = {m: _timed(run[m], dev)[1] for m in modes}                 # warm-up
        times = {m: [] for m in modes}
        for _ in range(a.runs):                  # alternating: both modes see the same neighbours on the machine
            for m in modes:
                times[m].append(_timed(run[m], dev)[0])
        res[f"{shape}_columns"] = X.shape[1]
        res[f"{shape}_nonzeros_per_row"] = round(float((X[:a.records] != 0).sum(1).float().mean()), 1)
        for m in modes:
            res[f"{shape}_{m}_median_s"] = round(statistics.median(times[m]), 5)
            res[f"{shape}_{m}_runs_s"] = [round(t, 5) for t in times[m]]
        res[f"{shape}_rescore_over_margins"] = round(res[f"{shape}_rescore_median_s"] /
                                                     res[f"{shape}_margins_median_s"], 2)
        res[f"{shape}_margins_faster"] = bool(max(times["margins"]) < min(times["rescore"]))
        same = (np.sort(out["rescore"].cols.cpu().numpy(), 1) == np.sort(out["margins"].cols.cpu().numpy(), 1)).all(1)
        res[f"{shape}_same_columns_share"] = round(float(same.mean()), 4)
        print(f"{shape}: rescore {res[f'{shape}_rescore_median_s']} s, margins {res[f'{shape}_margins_median_s']} s",
              file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("RecordInsightsLOCO rescore vs margins mode (benchmarks/bench_loco_linear.py): median of "
                f"{a.runs} device-synchronised runs, alternating, after one warm-up each\n")
        for k, v in res.items():
            f.write(f"{k}: {v}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
