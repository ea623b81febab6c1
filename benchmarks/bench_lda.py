"""LDA: ``OpLDA`` fit plus transform through the dense torch E-step and through the sparse HIP E-step
(``ops/csrc/hip/lda_kernels.hip``) on one synthetic corpus.

The corpus has ``--docs`` documents over ``--terms`` columns, about ``--doc-terms`` distinct terms per document
(counts 1..5), as a dense fp32 matrix on the device. ``--docs`` is halved until the dense path fits in device memory;
the ``N`` used is reported, with the dense path's peak allocation and two extrapolations from it (peak bytes per
document at that ``N``, scaled; neither is probed): the ``N`` at which the allocation reaches the device's memory, and
the bytes the dense path would need at ``--big-docs`` documents, where one more row times the sparse path alone.
The two paths alternate in one process; every run is device-synchronised wall time, and the median of ``--runs`` runs
after one warm-up each is reported with all runs. The compiler's resource report of the kernels is appended. Writes
``--out`` and prints the result as one JSON line. Not part of any gate: no threshold, the file records what was found.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def corpus(n, terms, doc_terms, dev, seed=0, chunk=1 << 16):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.zeros(n, terms, dtype=torch.float32, device=dev)
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        cols = torch.randint(0, terms, (m, doc_terms), generator=g, device=dev)
        vals = torch.randint(1, 6, (m, doc_terms), generator=g, device=dev).to(torch.float32)
        X[a:a + m].scatter_(1, cols, vals)          # repeated columns collapse: a little under doc_terms distinct
    return X


def fit_transform(X, K, em_steps, sparse):
    from transmogrifai_amd.data.columns import VectorColumn
    from transmogrifai_amd.stages.feature.nlp_stages import OpLDA
    os.environ["TMOG_LDA_SPARSE"] = "1" if sparse else "0"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = OpLDA(k=K, max_iter=em_steps, seed=0).fit_columns(VectorColumn(X))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    theta = model._infer(X)
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t1, theta


def resource_report():
    """Registers, LDS and occupancy of the LDA kernels, from the compiler."""
    from transmogrifai_amd.ops import build as B
    src = B.CSRC / "hip" / "lda_kernels.hip"
    cmd = [B.hipcc_path(), f"--offload-arch={B.ARCH}", "--cuda-device-only"] + B.HIP_FLAGS + \
        [f"-I{B.CSRC}", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, str(src)]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    rows, name = [], None
    for m in re.finditer(r"remark: \S*\s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                         r"LDS Size \[bytes/block\]): (\S+)", text):
        if m[1] == "Function Name":
            name = subprocess.run(["c++filt", m[2]], stdout=subprocess.PIPE, text=True).stdout.strip()
            rows.append(name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0])
        elif name:
            rows[-1] += f"  {m[1]}={m[2]}"
    return [r for r in rows if "estep" in r or "sstats" in r or "fold" in r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--big-docs", type=int, default=2_500_000)
    ap.add_argument("--terms", type=int, default=4096)
    ap.add_argument("--doc-terms", type=int, default=30)
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--em-steps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lda_sparse.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lda.py measures on the GPU; no device found")
    dev = torch.device("cuda")
    total = torch.cuda.get_device_properties(dev).total_memory
    res = {"gpu": torch.cuda.get_device_name(dev), "device_memory_bytes": total, "terms": a.terms,
           "doc_terms": a.doc_terms, "topics": a.topics, "em_steps": a.em_steps, "runs": a.runs,
           "docs_asked": a.docs}
    n = a.docs
    while True:                                     # the dense path's warm-up doubles as the fit-in-memory probe
        X = corpus(n, a.terms, a.doc_terms, dev)
        torch.cuda.reset_peak_memory_stats(dev)
        try:
            dense_theta = fit_transform(X, a.topics, a.em_steps, sparse=False)[2]
            break
        except torch.cuda.OutOfMemoryError:
            del X
            torch.cuda.empty_cache()
            n //= 2
    peak = torch.cuda.max_memory_allocated(dev)
    res.update(docs_used=n, density=round(float((X != 0).float().mean()), 5), dense_peak_allocated_bytes=peak,
               dense_stops_fitting_at_docs_extrapolated=int(total / (peak / n)))
    sparse_theta = fit_transform(X, a.topics, a.em_steps, sparse=True)[2]
    res["theta_max_abs_diff_sparse_vs_dense"] = float((sparse_theta - dense_theta).abs().max())
    del dense_theta, sparse_theta
    times = {"dense": [], "sparse": []}
    for _ in range(a.runs):
        for name in times:
            times[name].append(fit_transform(X, a.topics, a.em_steps, sparse=name == "sparse")[:2])
    for name, t in times.items():
        res[f"{name}_fit_median_s"] = round(statistics.median(x[0] for x in t), 4)
        res[f"{name}_transform_median_s"] = round(statistics.median(x[1] for x in t), 4)
        res[f"{name}_fit_transform_runs_s"] = [[round(x[0], 4), round(x[1], 4)] for x in t]
    del X
    torch.cuda.empty_cache()
    X = corpus(a.big_docs, a.terms, a.doc_terms, dev)
    res.update(big_docs=a.big_docs, big_dense_needs_bytes_extrapolated=int(peak / n * a.big_docs))
    fit_transform(X, a.topics, a.em_steps, sparse=True)
    big = [fit_transform(X, a.topics, a.em_steps, sparse=True)[:2] for _ in range(a.runs)]
    res["big_sparse_fit_median_s"] = round(statistics.median(x[0] for x in big), 4)
    res["big_sparse_transform_median_s"] = round(statistics.median(x[1] for x in big), 4)
    res["big_sparse_fit_transform_runs_s"] = [[round(x[0], 4), round(x[1], 4)] for x in big]
    res["kernel_resources"] = resource_report()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("LDA fit + transform, dense torch E-step vs sparse HIP E-step (benchmarks/bench_lda.py): median of "
                f"{a.runs} device-synchronised runs, alternating, after one warm-up each\n")
        f.write("not measured: a padded LDS row pitch against the unpadded pitch K the kernel uses\n")
        for k, v in res.items():
            if k == "kernel_resources":
                f.write("kernel_resources:\n" + "".join(f"  {r}\n" for r in v))
            else:
                f.write(f"{k}: {v}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
