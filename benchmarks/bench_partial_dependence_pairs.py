"""Two-way partial dependence: ``tree_engine.forest_partial_dependence_pairs`` against brute-force rescoring on one
XGBoost model of a headline grid point.

Trains the model of ``bench_partial_dependence.py`` (one ``OpXGBoostClassifier``, ``--rounds`` rounds, depth
``--depth``, on ``--rows`` synthetic rows of the headline table), takes the pairs of its ``--top-k`` columns by
feature contribution and ``--records`` records, and times the sum over the records of the margin with the two
columns of each pair at each cell of the product of their bins:

* ``pairs``: one ``forest_partial_dependence_pairs`` call (HIP kernel ``pd_pair_kernels.hip``, in-kernel sum), and
  the per-record mode in row blocks reduced in torch (``per_record``);
* ``brute``: the two binned columns overwritten with one cell's bins and ``forest_predict`` on ``--brute-records``
  records, once per valid cell and pair; with fewer records than ``--records`` its times are scaled by the ratio
  of the two and the output says so.

The paths alternate in one process, every run is device-synchronised wall time, and the median of ``--runs`` runs
after one warm-up each is reported with all runs and the ratios, with the counted tree walks of each (the new
path's from the host twin's counters) and the largest difference of the two results. Writes the result to ``--out``
and prints it as one JSON line. Not part of any gate: no threshold, the file records what was found.
"""
from __future__ import annotations

import argparse
import itertools
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
    ap.add_argument("--top-k", type=int, default=3)
    ap.add_argument("--brute-records", type=int, default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial_dependence_pairs.txt"))
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
    pairs = list(itertools.combinations(cols, 2))
    bins = {c: list(range(int(spec.n_bins[c]))) + ([int(spec.missing_bin)] if spec.missing_bin >= 0 else [])
            for c in cols}
    cells = int(sum(len(bins[p]) * len(bins[q]) for p, q in pairs))
    nb = n if a.brute_records is None else max(1, min(n, a.brute_records))
    T = forest.n_trees
    res = {"model": f"OpXGBoostClassifier num_round={a.rounds} max_depth={a.depth} ({T} trees, "
                    f"{int((forest.nodes[:, 2] < 0).sum())} leaves)",
           "train_rows": a.rows, "vector_columns": d, "records": n, "pairs": [list(p) for p in pairs],
           "grid_width": NB, "grid_cells": cells, "device": str(dev),
           "gpu": torch.cuda.get_device_name(dev) if dev.type == "cuda" else None, "train_s": round(t_train, 2),
           "brute_records": nb, "brute_times_scaled_by": round(n / nb, 4)}
    pq = np.asarray(pairs, np.int64)

    def pairs_sum():
        return TE.forest_partial_dependence_pairs(forest, Xb, pq, NB, plan=plan)

    def per_record_sum():
        block = max(1, (256 << 20) // (len(pairs) * NB * NB * 8))
        tot = torch.zeros(len(pairs), NB, NB, 1, dtype=torch.float64, device=dev)
        for s in range(0, n, block):
            r = torch.arange(s, min(n, s + block), device=dev)
            tot += TE.forest_partial_dependence_pairs(forest, Xb, pq, NB, r, plan=plan, ice=True).sum(0)
        return tot

    all_trees = [list(range(T))]
    Xsub = Xb[:nb].contiguous()

    def brute():
        Xw = Xsub.clone()
        out = torch.zeros(len(pairs), NB, NB, 1, dtype=torch.float64, device=dev)
        for p, (ca, cb) in enumerate(pairs):
            keep_a, keep_b = Xw[:, ca].clone(), Xw[:, cb].clone()
            for i in bins[ca]:
                Xw[:, ca] = i
                for j in bins[cb]:
                    Xw[:, cb] = j
                    out[p, i, j, 0] = TE.forest_predict(forest, Xw, [None], all_trees,
                                                        tw)[0][:, 0].to(torch.float64).sum()
            Xw[:, ca], Xw[:, cb] = keep_a, keep_b
        return out

    paths = {"pairs": pairs_sum, "per_record": per_record_sum, "brute": brute}
    factor = {"pairs": 1.0, "per_record": 1.0, "brute": n / nb}
    out = {}
    for m, fn in paths.items():
        t, out[m] = _timed(fn, dev)
        res[f"{m}_warmup_s"] = round(t * factor[m], 4)
    times = {m: [] for m in paths}
    for _ in range(a.runs):                      # alternating: every path sees the same neighbours on the machine
        for m, fn in paths.items():
            times[m].append(_timed(fn, dev)[0] * factor[m])
    for m in paths:
        res[f"{m}_median_s"] = round(statistics.median(times[m]), 5)
        res[f"{m}_runs_s"] = [round(t, 5) for t in times[m]]
        print(f"{m}: median {res[f'{m}_median_s']} s", file=sys.stderr, flush=True)
    res["brute_over_pairs"] = round(res["brute_median_s"] / res["pairs_median_s"], 2)
    res["brute_over_per_record"] = round(res["brute_median_s"] / res["per_record_median_s"], 2)
    res["pairs_slowest_beats_brute_fastest"] = bool(
        max(times["pairs"] + times["per_record"]) < min(times["brute"]))
    res["per_record_sum_max_abs_diff"] = float((out["per_record"] - out["pairs"]).abs().max())
    mask = torch.zeros(len(pairs), NB, NB, dtype=torch.bool, device=dev)
    for p, (ca, cb) in enumerate(pairs):
        mask[p] = torch.zeros(NB, dtype=torch.bool, device=dev).index_fill_(
            0, torch.tensor(bins[ca], device=dev), True)[:, None] & torch.zeros(
            NB, dtype=torch.bool, device=dev).index_fill_(0, torch.tensor(bins[cb], device=dev), True)[None, :]
    ref = out["pairs"] if nb == n else TE.forest_partial_dependence_pairs(forest, Xsub, pq, NB, plan=plan)
    res["brute_fp32_max_abs_diff_per_record"] = float(((out["brute"] - ref)[mask]).abs().max()) / max(nb, 1)
    walks = np.zeros(3, np.int64)                 # counted by the host twin on the same rows
    TE.forest_partial_dependence_pairs(forest, Xb.cpu(), pq, NB, plan=plan, _walks=walks)
    res["pairs_base_walks"], res["pairs_anchor_searches"], res["pairs_rectangle_walks"] = (int(w) for w in walks)
    res["brute_walks"] = cells * n * T
    res["brute_walks_over_pairs_walks"] = round(res["brute_walks"] / max(1, int(walks.sum())), 1)
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        res["commit"] = os.environ.get("TMOG_COMMIT", "unknown")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("Two-way partial dependence: forest_partial_dependence_pairs vs brute-force rescoring "
                f"(benchmarks/bench_partial_dependence_pairs.py): median of {a.runs} device-synchronised runs, "
                "alternating, after one warm-up each"
                + ("" if nb == n else f"; brute force ran on {nb} of the {n} records, its times are scaled by "
                                      f"{n / nb:.4g}") + "\n")
        for k, v in res.items():
            f.write(f"{k}: {v}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
