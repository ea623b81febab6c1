"""RecordInsightsLOCO: the rescore mode against the paths mode on one XGBoost model of a headline grid point.

Trains the model of ``bench_shap.py`` (one ``OpXGBoostClassifier``, ``--rounds`` rounds, depth ``--depth``, on
``--rows`` synthetic rows of the headline table), then times ``RecordInsightsLOCO`` on the same ``--records``
records with ``perturbation="rescore"`` (one perturbed copy of the record per non-zero column through the model's
predict) and ``perturbation="paths"`` (``tree_engine.forest_loco``, HIP kernel ``loco_kernels.hip``): the two modes
alternate in one process, every run is device-synchronised wall time, and the median of ``--runs`` runs after one
warm-up each is reported with all runs and the ratio. Also reports the share of records whose rendered maps have
the same key set in both modes. Writes the result to ``--out`` and prints it as one JSON line. Not part of any
gate: no threshold, the file records what was found.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loco_paths.txt"))
    a = ap.parse_args()
    from transmogrifai_amd import config as CFG
    from transmogrifai_amd.dsl import transmogrify
    from transmogrifai_amd.models.trees import OpXGBoostClassifier
    from transmogrifai_amd.readers.base import InMemoryReader
    from transmogrifai_amd.stages.insights.record_insights import RecordInsightsLOCO
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
    sub = wf.score(keep_intermediate_features=True).take(torch.arange(min(a.records, a.rows))).select([vec.name])
    n, d = sub[vec.name].values.shape
    forest = model.learner._forest(model.state)[0]
    res = {"model": f"OpXGBoostClassifier num_round={a.rounds} max_depth={a.depth} ({forest.n_trees} trees, "
                    f"{int((forest.nodes[:, 2] < 0).sum())} leaves)",
           "train_rows": a.rows, "vector_columns": d, "records": n, "top_k": a.top_k, "device": str(dev),
           "gpu": torch.cuda.get_device_name(dev) if dev.type == "cuda" else None, "train_s": round(t_train, 2)}
    modes = ("rescore", "paths")
    stages = {m: RecordInsightsLOCO(model, top_k=a.top_k, perturbation=m).set_input(vec) for m in modes}
    run = {m: (lambda st=stages[m]: st.transform(sub)[st.get_output().name]) for m in modes}
    out = {}
    for m in modes:
        t, out[m] = _timed(run[m], dev)
        res[f"{m}_warmup_s"] = round(t, 3)
    times = {m: [] for m in modes}
    for _ in range(a.runs):                      # alternating: both modes see the same neighbours on the machine
        for m in modes:
            times[m].append(_timed(run[m], dev)[0])
    for m in modes:
        res[f"{m}_median_s"] = round(statistics.median(times[m]), 4)
        res[f"{m}_runs_s"] = [round(t, 4) for t in times[m]]
        print(f"{m}: median {res[f'{m}_median_s']} s", file=sys.stderr, flush=True)
    res["used_columns"] = int(model.state["_loco_plan"].used.size)
    res["rescore_over_paths"] = round(res["rescore_median_s"] / res["paths_median_s"], 2)
    res["paths_slowest_beats_rescore_fastest"] = bool(max(times["paths"]) < min(times["rescore"]))
    keys = [[set(m or {}) for m in out[mode].to_list()] for mode in modes]
    res["same_key_set_share"] = round(sum(x == y for x, y in zip(*keys)) / max(n, 1), 4)
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        res["commit"] = os.environ.get("TMOG_COMMIT", "unknown")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("RecordInsightsLOCO rescore vs paths mode (benchmarks/bench_loco.py): median of "
                f"{a.runs} device-synchronised runs, alternating, after one warm-up each\n")
        for k, v in res.items():
            f.write(f"{k}: {v}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
