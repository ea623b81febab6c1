"""SHAP interaction values against plain TreeSHAP on one XGBoost model of a headline grid point.

Trains one ``OpXGBoostClassifier`` (``--rounds`` rounds, depth ``--depth``) on ``--rows`` synthetic rows of the
headline table (200 predictors), then times on the same ``--records`` records (default: as many as keep the
``[n, U + 1, U + 1, C]`` result below ``--result-mb``, computed from the number ``U`` of columns the trees use):

* ``tmog_hip_forest_shap_interactions`` alone (device events around the launch, pair sums only),
* ``forest_shap_interactions`` on the device (kernel + ``forest_shap`` + the torch finishing step),
* ``forest_shap`` on the device,
* ``forest_shap_interactions`` on the host twin (one run: it is slow).

Device times are the median of ``--runs`` device-synchronised runs after one warm-up. The file records three
ratios: kernel / ``forest_shap``, that ratio beside the arithmetic ratio the recurrences predict -- per (record,
path) TreeSHAP runs ``2 m`` EXTEND / UNWOUND steps and the interactions ``m * 2 (m - 1)``, so
``sum m (m - 1) / sum m`` over the paths, close to the mean merged path length -- and host twin / kernel.
``forest_shap`` gives every workgroup 64 records, so the few hundred records whose interaction matrix fits do not
fill the GPU with it; its per-record cost is therefore also taken on ``--shap-records`` records, and the
per-record ratio is the one to hold against the arithmetic ratio.
Not part of any gate: no threshold, the file records what was found.
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


def _median(fn, dev, runs):
    _timed(fn, dev)
    return [_timed(fn, dev)[0] for _ in range(runs)]


def _kernel_only(te, fp, Xb, C, runs):
    """Seconds of the interaction kernel alone (device events), pair sums into a preallocated buffer."""
    N = te.N
    dev = Xb.device
    n, F, U = int(Xb.shape[0]), int(Xb.shape[1]), int(fp.used.size)
    d = fp.on(dev)
    tri = torch.empty(n, U, U, C, dtype=torch.float64, device=dev)

    def launch():
        N.check(N.hip().tmog_hip_forest_shap_interactions(
            N.ptr(Xb), F, n, None, U, N.ptr(d[0]), int(fp.p_out.size), N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]),
            int(fp.p_val.shape[1]), None, N.ptr(d[4]), N.ptr(d[5]), N.ptr(d[6]), fp.bin_off.ctypes.data,
            fp.missing_bin, C, fp.scale, N.ptr(tri), N.stream(dev)), "forest_shap_interactions")

    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--records", type=int, default=0, help="0: from U and --result-mb")
    ap.add_argument("--result-mb", type=int, default=512)
    ap.add_argument("--shap-records", type=int, default=20_000, help="records of the per-record forest_shap time")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host twin")
    ap.add_argument("--note", default="", help="a sentence on what the numbers show, appended to the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_interactions.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shap_interactions.py measures the HIP kernel: no GPU found")
    from transmogrifai_amd import config as CFG
    from transmogrifai_amd.dsl import transmogrify
    from transmogrifai_amd.models import tree_engine as te
    from transmogrifai_amd.models.trees import OpXGBoostClassifier
    from transmogrifai_amd.readers.base import InMemoryReader
    from transmogrifai_amd.testkit.synthetic import binary_table
    from transmogrifai_amd.workflow.workflow import OpWorkflow

    dev = torch.device("cuda")
    CFG.set_default_device(dev)
    ds, label, preds = binary_table(a.rows, device=dev)
    vec = transmogrify(preds)
    pred = OpXGBoostClassifier(num_round=a.rounds, max_depth=a.depth, eta=0.1).set_input(label, vec).get_output()
    t_train, wf = _timed(lambda: OpWorkflow().set_result_features(pred, vec).set_reader(InMemoryReader(ds)).train(),
                         dev)
    print(f"trained in {t_train:.1f} s", file=sys.stderr, flush=True)
    model = wf.get_origin_stage_of(pred)
    learner, state = model.learner, model.state
    scored = wf.score(keep_intermediate_features=True)
    X = scored[vec.name].values
    learner.shap_values(state, X[:8])                     # prepares and caches the paths
    fp = state["_shap_paths"]
    U, C = int(fp.used.size), 1
    n = a.records or max(8, (a.result_mb << 20) // ((U + 1) ** 2 * C * 8) // 8 * 8)
    n = min(n, int(X.shape[0]))
    forest, Xb = learner._binned_for(state, X[:n], None)
    Xb = Xb.contiguous()
    m = np.diff(fp.p_off).astype(np.float64)
    res = {"model": f"OpXGBoostClassifier num_round={a.rounds} max_depth={a.depth} ({forest.n_trees} trees, "
                    f"{m.size} leaves)",
           "train_rows": a.rows, "records": n, "used_columns": U, "result_mb": round(n * (U + 1) ** 2 * C * 8 / 2 ** 20, 1),
           "gpu": torch.cuda.get_device_name(dev), "train_s": round(t_train, 2),
           "mean_merged_path_length": round(float(m.mean()), 3), "max_merged_path_length": int(m.max()),
           "arithmetic_ratio": round(float((m * (m - 1)).sum() / m.sum()), 3)}
    t_shap = _median(lambda: te.forest_shap(forest, Xb, n_out=C, paths=fp), dev, a.runs)
    t_full = _median(lambda: te.forest_shap_interactions(forest, Xb, n_out=C, paths=fp), dev, a.runs)
    t_kern = _kernel_only(te, fp, Xb, C, a.runs)
    res.update(forest_shap_median_s=round(statistics.median(t_shap), 5), forest_shap_runs_s=[round(t, 5) for t in t_shap],
               kernel_median_s=round(statistics.median(t_kern), 5), kernel_runs_s=[round(t, 5) for t in t_kern],
               interactions_median_s=round(statistics.median(t_full), 5),
               interactions_runs_s=[round(t, 5) for t in t_full])
    print(f"forest_shap {res['forest_shap_median_s']} s, kernel {res['kernel_median_s']} s", file=sys.stderr, flush=True)
    res["kernel_over_forest_shap"] = round(res["kernel_median_s"] / res["forest_shap_median_s"], 2)
    # forest_shap gives a workgroup 64 records, so the few records an interaction matrix leaves room for do not
    # fill the GPU with it: the per-record cost the arithmetic ratio speaks of is taken at --shap-records
    ns = min(a.shap_records, int(X.shape[0]))
    Xs = learner._binned_for(state, X[:ns], None)[1].contiguous()
    t_sat = _median(lambda: te.forest_shap(forest, Xs, n_out=C, paths=fp), dev, a.runs)
    res.update(forest_shap_many_records=ns, forest_shap_many_median_s=round(statistics.median(t_sat), 5),
               forest_shap_many_runs_s=[round(t, 5) for t in t_sat])
    res["per_record_kernel_over_forest_shap"] = round(
        (res["kernel_median_s"] / n) / (res["forest_shap_many_median_s"] / ns), 2)
    res["kernel_over_forest_shap_vs_arithmetic"] = \
        f"{res['kernel_over_forest_shap']} on the same {n} records, {res['per_record_kernel_over_forest_shap']} per " \
        f"record against forest_shap on {ns} records; {res['arithmetic_ratio']} expected from the step counts " \
        f"(mean merged path length {res['mean_merged_path_length']})"
    # the stage on top: blocks of records, folding onto candidates, top-K pairs (rendering not included)
    from transmogrifai_amd.stages.insights.record_insights import RecordInsightsSHAPInteractions
    ns2 = min(4 * n, int(X.shape[0]))
    sub = scored.take(torch.arange(ns2)).select([vec.name])
    stage = RecordInsightsSHAPInteractions(model, top_k=20).set_input(vec)
    t_stage = _median(lambda: stage.transform(sub)[stage.get_output().name], dev, 3)
    res.update(stage_records=ns2, stage_median_s=round(statistics.median(t_stage), 4),
               stage_runs_s=[round(t, 4) for t in t_stage])
    if not a.no_host:
        Xh = Xb.cpu()
        t_host, want = _timed(lambda: te.forest_shap_interactions(forest, Xh, n_out=C, paths=fp)[0], torch.device("cpu"))
        got = te.forest_shap_interactions(forest, Xb, n_out=C, paths=fp)[0]
        res["host_twin_s"] = round(t_host, 3)
        res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()
        res["host_twin_over_kernel"] = round(t_host / res["kernel_median_s"], 1)
        res["max_abs_difference_over_S"] = float((got.cpu() - want).abs().max().item() / fp.S)
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        res["commit"] = os.environ.get("TMOG_COMMIT", "unknown")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("SHAP interaction values vs TreeSHAP (benchmarks/bench_shap_interactions.py): median of "
                f"{a.runs} device-synchronised runs after one warm-up\n")
        for k, v in res.items():
            f.write(f"{k}: {v}\n")
        if a.note:
            f.write(f"note: {a.note}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
