"""Word2Vec: ``OpWord2Vec`` fit through the pairs trainer (autograd over materialised pairs) and through the windows
trainer (``ops/csrc/hip/w2v_kernels.hip``) on one synthetic Zipf corpus.

The corpus has ``--tokens`` tokens in documents of ``--doc-len`` over ``--vocab`` words with Zipf frequencies, as
token lists in a dataset on the device. The two trainers alternate in one process; every run is device-synchronised
wall time of ``fit_columns`` (vocabulary and corpus building included), and the median of ``--runs`` runs after one
warm-up each is reported with all runs. ``--sweep`` sizes are timed the same way to find the crossover: the smallest
swept size from which the windows trainer's median stays below the pairs trainer's. ``--big-tokens`` is run through
the windows trainer alone. One step of the windows trainer at ``--batch`` windows is then split into its parts (the
window kernel, the two stable sorts, the two applies) with device events. The compiler's resource report of the
kernels is appended. Writes ``--out`` and prints the result as one JSON line. Not part of any gate: no threshold,
the file records what was found.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def corpus(tokens, doc_len, vocab, seed=0):
    """A dataset on the device with one token-list column, and that column."""
    from transmogrifai_amd.features import types as T
    from transmogrifai_amd.testkit.feature_builder import TestFeatureBuilder
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    ids = rng.choice(vocab, tokens, p=p / p.sum())
    words = np.array([f"w{i}" for i in range(vocab)], dtype=object)[ids]
    docs = [list(words[a:a + doc_len]) for a in range(0, tokens, doc_len)]
    ds, (t, _) = TestFeatureBuilder.of(("t", T.TextList, docs), ("x", T.Real, [0.0] * len(docs)), device="cuda")
    return ds, ds[t.name]


def fit(ds, col, trainer, a):
    from transmogrifai_amd.stages.feature.nlp_stages import OpWord2Vec
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    OpWord2Vec(vector_size=a.vector_size, min_count=1, max_iter=a.epochs, batch_size=a.batch, trainer=trainer,
               seed=0).fit_columns(col, ds=ds)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed(ds, col, trainers, a):
    """Median and all runs per trainer, alternating, after one warm-up each."""
    runs = {t: [] for t in trainers}
    for i in range(a.runs + 1):
        for t in trainers:
            s = fit(ds, col, t, a)
            if i:
                runs[t].append(round(s, 4))
    return {t: {"median_s": round(statistics.median(r), 4), "runs_s": r} for t, r in runs.items()}


def step_parts(a, reps=20):
    """Device-event milliseconds of the parts of one windows step at ``--batch`` windows, median of ``reps``."""
    from transmogrifai_amd.ops import word2vec as W2V
    rng = np.random.default_rng(1)
    p = 1.0 / np.arange(1, a.vocab + 1)
    T = max(a.tokens, a.batch)
    c = W2V.TokenCorpus(rng.choice(a.vocab, T, p=p / p.sum()), np.append(np.arange(0, T, a.doc_len), T), "cuda")
    Dp = W2V.padded(a.vector_size)
    ein, eout = torch.rand(a.vocab, Dp, device="cuda") - 0.5, torch.rand(a.vocab, Dp, device="cuda") - 0.5
    pos = torch.randperm(T, device="cuda")[:a.batch].to(torch.int32)
    neg = torch.randint(0, a.vocab, (a.batch, 5), device="cuda", dtype=torch.int32)
    n_pos = torch.tensor([a.batch * 10], dtype=torch.int32, device="cuda")
    parts = {"window_kernel": [], "two_sorts": [], "two_applies_with_sorts": []}
    for i in range(reps + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        gin, gout, kin, kout = W2V.window_grads(ein, eout, c, pos, neg, 5, n_pos, 1e-3)
        ev[1].record()
        torch.sort(kin.reshape(-1), stable=True), torch.sort(kout.reshape(-1), stable=True)
        ev[2].record()
        W2V.apply_rows(ein, gin, kin.reshape(-1)), W2V.apply_rows(eout, gout, kout.reshape(-1))
        ev[3].record()
        torch.cuda.synchronize()
        if i >= 2:
            for k, name in enumerate(parts):
                parts[name].append(ev[k].elapsed_time(ev[k + 1]))
    ms = {k: round(statistics.median(v), 4) for k, v in parts.items()}
    ms["two_applies"] = round(ms.pop("two_applies_with_sorts") - ms["two_sorts"], 4)
    total = sum(ms.values())
    slab_bytes = 2 * a.batch * 16 * Dp * 4
    return {"batch": a.batch, "Dp": Dp, "ms": ms, "share": {k: round(v / total, 3) for k, v in ms.items()},
            "window_kernel_slab_write_GBps": round(slab_bytes / ms["window_kernel"] / 1e6, 1)}


def resource_report():
    """Registers, LDS and occupancy of the word2vec kernels, from the compiler."""
    from transmogrifai_amd.ops import build as B
    src = B.CSRC / "hip" / "w2v_kernels.hip"
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
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=200_000)
    ap.add_argument("--big-tokens", type=int, default=4_000_000)
    ap.add_argument("--sweep", type=int, nargs="*", default=[1 << 10, 1 << 12, 1 << 14, 1 << 16])
    ap.add_argument("--doc-len", type=int, default=20)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--vector-size", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word2vec_windows.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_word2vec.py measures on the GPU; no device found")
    res = {"gpu": torch.cuda.get_device_name(0), "doc_len": a.doc_len, "vocab": a.vocab, "vector_size": a.vector_size,
           "batch": a.batch, "epochs": a.epochs, "runs": a.runs, "window_size": 5, "num_negative": 5}
    crossover = None
    for n in sorted(set(a.sweep + [a.tokens])):
        ds, col = corpus(n, a.doc_len, a.vocab)
        r = timed(ds, col, ("pairs", "windows"), a)
        res[f"tokens_{n}"] = r
        if r["windows"]["median_s"] >= r["pairs"]["median_s"]:
            crossover = None
        elif crossover is None:
            crossover = n
    res["crossover_tokens"] = crossover if crossover is not None else "not reached in the sweep"
    ds, col = corpus(a.big_tokens, a.doc_len, a.vocab)
    res[f"big_tokens_{a.big_tokens}"] = timed(ds, col, ("windows",), a)
    res["step_parts"] = step_parts(a)
    res["kernel_resources"] = resource_report()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("OpWord2Vec fit, pairs trainer vs windows trainer (benchmarks/bench_word2vec.py): median of "
                f"{a.runs} device-synchronised runs, alternating, after one warm-up each\n")
        f.write("not measured: the kernels' own times (no trace), a padded LDS pitch against the rotated one, "
                "whether the window kernel is bound by its row gathers\n")
        for k, v in res.items():
            if k == "kernel_resources":
                f.write("kernel_resources:\n" + "".join(f"  {r}\n" for r in v))
            else:
                f.write(f"{k}: {v}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
