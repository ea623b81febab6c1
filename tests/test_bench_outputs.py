"""bench.py ``--dump-outputs``: the last timed train's outputs land as float32 / float64 ``.npy`` files under the
size cap, two runs with the same arguments write the same arrays, ``--steps`` sets the number of timed steps and
``ms_per_step`` is one timed step's milliseconds; ``--full`` keeps the result line and adds the diagnostics."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--device", "cpu", "--rows", "3000",
           "--warmup", "0", "--models", "OpLogisticRegression", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT,
                         env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith('{"metric"')][-1])


def _load(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_steps_and_full(tmp_path):
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    res = _bench("--steps", "2", "--dump-outputs", a_dir)
    full = _bench("--steps", "1", "--dump-outputs", b_dir, "--full")
    # --steps is the number of timed steps, ms_per_step their mean in milliseconds (step_s is rounded to 1e-4 s)
    assert res["steps"] == 2 and len(res["step_s"]) == 2 and len(full["step_s"]) == 1
    assert abs(res["ms_per_step"] - 1000.0 * sum(res["step_s"]) / 2) <= 0.1 + 1e-9
    assert res["value"] * 1000.0 == res["ms_per_step"]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res and key in full
    assert "stage_timings" in full and "stage_timings" not in res
    a, b = _load(a_dir), _load(b_dir)
    assert {"cv_metrics.npy", "train_evaluation.npy", "holdout_evaluation.npy"} <= set(a)
    assert any(n.startswith("model") for n in a), sorted(a)
    assert a["cv_metrics.npy"].shape[0] == res["configs_evaluated"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    # seeded inputs: the same arguments give the same outputs, whatever the number of steps before the last one
    # (float32 design matrix: agreement to float32 resolution)
    assert sorted(a) == sorted(b)
    for n in a:
        assert a[n].shape == b[n].shape, n
        np.testing.assert_allclose(a[n], b[n], rtol=1e-6, atol=1e-9, equal_nan=True, err_msg=n)
    assert res["holdout_aupr"] in a["holdout_evaluation.npy"].tolist()


def test_write_outputs_samples_large_arrays(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    big = np.arange(10_000, dtype=np.int64).reshape(100, 100)
    arrays = {"big": big, "half/odd name": np.ones(7, np.float16)}
    bench.write_outputs(arrays, str(tmp_path / "o1"))
    bench.write_outputs(arrays, str(tmp_path / "o2"))
    o1, o2 = _load(str(tmp_path / "o1")), _load(str(tmp_path / "o2"))
    assert sorted(o1) == ["big.npy", "half_odd_name.npy"]
    assert sum(v.nbytes for v in o1.values()) <= 4000
    assert o1["big.npy"].dtype == np.float64 and o1["big.npy"].size == 2000 // 8
    s = o1["big.npy"]
    assert np.all(np.diff(s) > 0) and set(s.tolist()) <= set(range(10_000))     # a sorted sample of the elements
    for n in o1:
        np.testing.assert_array_equal(o1[n], o2[n])
    assert o1["half_odd_name.npy"].tolist() == [1.0] * 7
