"""Partial dependence: ``tree_engine.forest_partial_dependence`` against brute-force rescoring on one XGBoost model
of a headline grid point.

Trains the model of ``bench_loco.py`` (one ``OpXGBoostClassifier``, ``--rounds`` rounds, depth ``--depth``, on
``--rows`` synthetic rows of the headline table), takes its ``--top-k`` columns by feature contribution and
``--records`` records, and times the sum over the records of the margin with each column at each of its bins:

* ``pd``: one ``forest_partial_dependence`` call (HIP kernel ``pd_kernels.hip``, in-kernel sum), and the ICE mode
  in row blocks reduced in torch (``ice``);
* ``brute``: the binned column overwritten with one grid value and ``forest_predict`` on all records, once per
  valid grid point and column.

The paths alternate in one process, every run is device-synchronised wall time, and the median of ``--runs`` runs
after one warm-up each is reported with all runs and the ratios, with the counted tree walks of each (the new
path's from the host twin's counters) and the largest difference of the two results. Writes the result to ``--out``
and prints it as one JSON line. Not part of any gate: no threshold, the file records what was found.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--records", type=int, default=20_000)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial_dependence.txt"))
    a = ap.parse_args()
    from transmogrifai_amd import config as CFG
    from transmogrifai_amd.dsl import transmogrify
    from transmogrifai_amd.models import tree_engine as TE
    from transmogrifai_amd.models.trees import OpXGBoostClassifier
    from transmogrifai_amd.readers.base import InMemoryReader
    from transmogrifai_amd.testkit.synthetic import binary_table
    from transmogrifai_amd.workflow.workflow import OpWorkflow

    dev = torch.device(a.device if torch.cuda.is_available() else "cpu")
    CFG.set_default_device(dev)
    ds, label, preds = binary_table(a.rows, device=dev)
    vec = transmogrify(preds)
    pred = OpXGBoostClassifier(num_round=a.rounds, max_depth=a.depth, eta=0.1).set_input(label, vec).get_output()
    t_train, wf = _timed(lambda: OpWorkflow().set_result_features(pred, vec).set_reader(InMemoryReader(ds)).train(),
                         dev)
    print(f"trained in {t_train:.1f} s", file=sys.stderr, flush=True)
    model = wf.get_origin_stage_of(pred)
    learner, state = model.learner, model.state
    X = wf.score(keep_intermediate_features=True).take(torch.arange(min(a.records, a.rows)))[vec.name].values
    n, d = int(X.shape[0]), int(X.shape[1])
    forest, Xb = learner._binned_for(state, X, None)
    Xb = Xb.contiguous()
    spec = learner._forest(state)[1]
    NB = int(spec.B)
    tw = np.asarray(state["tree_weights"], np.float32)
    plan = TE.forest_loco_plan(forest, tw)
    contrib = np.abs(np.asarray(learner.feature_contributions(state, d), np.float64))
    cols = [int(i) for i in np.argsort(-contrib, kind="stable")[:a.top_k] if contrib[i] > 0]
    bins = [list(range(int(spec.n_bins[c]))) + ([int(spec.missing_bin)] if spec.missing_bin >= 0 else [])
            for c in cols]
    T = forest.n_trees
    res = {"model": f"OpXGBoostClassifier num_round={a.rounds} max_depth={a.depth} ({T} trees, "
                    f"{int((forest.nodes[:, 2] < 0).sum())} leaves)",
           "train_rows": a.rows, "vector_columns": d, "records": n, "columns": len(cols), "grid_width": NB,
           "grid_points": int(sum(len(b) for b in bins)), "device": str(dev),
           "gpu": torch.cuda.get_device_name(dev) if dev.type == "cuda" else None, "train_s": round(t_train, 2)}

    def pd_sum():
        return TE.forest_partial_dependence(forest, Xb, cols, NB, plan=plan)

    def ice_sum():
        block = max(1, (256 << 20) // (len(cols) * NB * 8))
        tot = torch.zeros(len(cols), NB, 1, dtype=torch.float64, device=dev)
        for s in range(0, n, block):
            r = torch.arange(s, min(n, s + block), device=dev)
            tot += TE.forest_partial_dependence(forest, Xb, cols, NB, r, plan=plan, ice=True).sum(0)
        return tot

    all_trees = [list(range(T))]

    def brute():
        Xw = Xb.clone()
        out = torch.zeros(len(cols), NB, 1, dtype=torch.float64, device=dev)
        for q, c in enumerate(cols):
            keep = Xw[:, c].clone()
            for b in bins[q]:
                Xw[:, c] = b
                out[q, b, 0] = TE.forest_predict(forest, Xw, [None], all_trees, tw)[0][:, 0].to(torch.float64).sum()
            Xw[:, c] = keep
        return out

    paths = {"pd": pd_sum, "ice": ice_sum, "brute": brute}
    out = {}
    for m, fn in paths.items():
        t, out[m] = _timed(fn, dev)
        res[f"{m}_warmup_s"] = round(t, 4)
    times = {m: [] for m in paths}
    for _ in range(a.runs):                      # alternating: every path sees the same neighbours on the machine
        for m, fn in paths.items():
            times[m].append(_timed(fn, dev)[0])
    for m in paths:
        res[f"{m}_median_s"] = round(statistics.median(times[m]), 5)
        res[f"{m}_runs_s"] = [round(t, 5) for t in times[m]]
        print(f"{m}: median {res[f'{m}_median_s']} s", file=sys.stderr, flush=True)
    res["brute_over_pd"] = round(res["brute_median_s"] / res["pd_median_s"], 2)
    res["pd_slowest_beats_brute_fastest"] = bool(max(times["pd"]) < min(times["brute"]))
    res["ice_sum_max_abs_diff"] = float((out["ice"] - out["pd"]).abs().max())
    mask = torch.zeros(len(cols), NB, dtype=torch.bool, device=dev)
    for q, b in enumerate(bins):
        mask[q, b] = True
    res["brute_fp32_max_abs_diff_per_record"] = float(((out["brute"] - out["pd"])[mask]).abs().max()) / max(n, 1)
    walks = np.zeros(2, np.int64)                 # counted by the host twin on the same rows
    TE.forest_partial_dependence(forest, Xb.cpu(), cols, NB, plan=plan, _walks=walks)
    res["pd_base_walks"], res["pd_step_walks"] = int(walks[0]), int(walks[1])
    res["brute_walks"] = int(res["grid_points"]) * n * T
    res["brute_walks_over_pd_walks"] = round(res["brute_walks"] / max(1, int(walks.sum())), 1)
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        res["commit"] = os.environ.get("TMOG_COMMIT", "unknown")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("Partial dependence: forest_partial_dependence vs brute-force rescoring "
                f"(benchmarks/bench_partial_dependence.py): median of {a.runs} device-synchronised runs, "
                "alternating, after one warm-up each\n")
        for k, v in res.items():
            f.write(f"{k}: {v}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
